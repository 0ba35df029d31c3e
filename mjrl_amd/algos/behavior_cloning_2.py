"""Behaviour cloning by regression with the API of mjrl/algos/behavior_cloning_2.py:11-77
(SURVEY.md §8f row f4): the mean-squared error of the policy mean against the
expert actions, minibatch Adam over policy.model.parameters(), the minibatch
steps on the GPU (algos/_device_sgd.py).

Same semantics as the reference: the constructor sets the policy's input /
output transformations from the expert data's mean / std (population std,
behavior_cloning_2.py:25-33), then sets log_std = log(std(actions) + 1e-12)
through get_param_values / set_param_values (the policy's log_std clamp applies)
and never trains it: Adam is built over the six tensors of the mean network
unless an optimizer is given.  train() logs epoch / loss / time before every
epoch and once after, draws int(N / batch_size) minibatches of
np.random.choice(N, batch_size) per epoch from numpy's global RNG, and ends with
set_param_values(params, set_new=True, set_old=True).  No progress bar: the
reference's tqdm wraps the epoch loop and changes nothing it computes.
The expert rows are staged to the device once per train() call.
fit_backend = "hip" (opt-in, per instance or on the class) runs the minibatch
steps as the fused kernel's MSE head (csrc/policy_fit.hip, mjrl_policy_mse_epoch;
batch_size <= 64, MLP policies up to 64 units wide, Adam over exactly
policy.model.parameters()); fit_backend = "hip_wide" as the sliced
kernels of csrc/policy_fit_wide.hip (mjrl_policy_mse_wide_epoch; hidden layers up to
256 units).
"""
import logging
import time as timer

import numpy as np
import torch

from ..utils.logger import DataLog
from ._device_sgd import DeviceTrainer, check_fit_backend, choice_batches, default_device

logging.disable(logging.CRITICAL)


class BC:
    # "torch": a captured graph of torch ops per minibatch step; "hip": the fused kernel of
    # csrc/policy_fit.hip (opt-in, per instance or on the class); "hip_wide": the sliced
    # kernels of csrc/policy_fit_wide.hip for hidden layers up to 256 units (opt-in too)
    fit_backend = "torch"

    def __init__(self, expert_paths, policy, epochs=5, batch_size=64, lr=1e-3, optimizer=None, device=None):
        self.policy = policy
        self.expert_paths = expert_paths
        self.epochs = epochs
        self.mb_size = batch_size
        self.logger = DataLog()
        observations = np.concatenate([path["observations"] for path in expert_paths])
        actions = np.concatenate([path["actions"] for path in expert_paths])
        in_shift, in_scale = np.mean(observations, axis=0), np.std(observations, axis=0)
        out_shift, out_scale = np.mean(actions, axis=0), np.std(actions, axis=0)
        self.policy.model.set_transformations(in_shift, in_scale, out_shift, out_scale)
        self.policy.old_model.set_transformations(in_shift, in_scale, out_shift, out_scale)
        # the exploration noise from the demonstrations' own spread
        params = self.policy.get_param_values()
        params[-self.policy.m:] = np.log(out_scale + 1e-12)
        self.policy.set_param_values(params)
        self.optimizer = torch.optim.Adam(self.policy.model.parameters(), lr=lr) if optimizer is None else optimizer
        self.loss_function = torch.nn.MSELoss()
        self._device = device
        self._trainer = None

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_trainer"] = None
        return d

    def trainer(self):
        if self._trainer is None:
            self._trainer = DeviceTrainer(self.policy, self.optimizer, default_device(self._device),
                                          params=list(self.policy.model.parameters()))
        return self._trainer

    def loss(self, obs, act):
        """MSE(policy.model(obs), act) at the current parameters
        (behavior_cloning_2.py:46-50), on the device; numpy inputs are staged first."""
        tr = self.trainer()
        tr.pull()
        o, a = self._stage(obs, act, tr.device)
        with torch.no_grad():
            return self.loss_function(tr.mean(o), a).cpu()

    @staticmethod
    def _stage(obs, act, dev):
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        return t(obs), t(act)

    def train(self):
        observations = np.concatenate([path["observations"] for path in self.expert_paths])
        actions = np.concatenate([path["actions"] for path in self.expert_paths])
        hip = check_fit_backend("BC", self.fit_backend, self.policy, self.optimizer, self.mb_size, self._device,
                                mean_only=True)
        tr = self.trainer()
        tr.pull()
        O, A = self._stage(observations, actions, tr.device)
        num_samples = observations.shape[0]

        def full_loss():
            with torch.no_grad():
                return float(self.loss_function(tr.mean(O), A).item())

        def mb_loss(idx):
            return self.loss_function(tr.mean(O.index_select(0, idx)), A.index_select(0, idx))

        ts = timer.time()
        # the captured step reads this call's O / A: a new key per call (an id() of a
        # freed tensor can come back for the next call's data)
        self._ncall = getattr(self, "_ncall", 0) + 1
        for ep in range(self.epochs):
            self.logger.log_kv("epoch", ep)
            self.logger.log_kv("loss", np.float32(full_loss()))
            self.logger.log_kv("time", timer.time() - ts)
            batches = choice_batches(num_samples, self.mb_size, tr.device)
            if hip:
                tr.fused_epoch("mse", O, A, batches, wide=self.fit_backend == "hip_wide")
            else:
                tr.epoch(("bc_mse", self._ncall), mb_loss, batches)
        tr.push()
        params_after_opt = self.policy.get_param_values()
        self.policy.set_param_values(params_after_opt, set_new=True, set_old=True)
        self.logger.log_kv("epoch", self.epochs)
        tr.pull()
        self.logger.log_kv("loss", np.float32(full_loss()))
        self.logger.log_kv("time", timer.time() - ts)
