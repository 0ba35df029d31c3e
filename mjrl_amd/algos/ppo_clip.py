"""PPO with the clipped surrogate, API of mjrl/algos/ppo_clip.py:23-120
(SURVEY.md §8f row f4).

train_from_paths keeps the reference's flow: whitened advantages
(adv - mean) / (std + 1e-6), path-return statistics, surr_before, `epochs`
passes of int(N / mb_size) minibatches drawn by np.random.choice from numpy's
global RNG, each an Adam step on -mean(min(LR adv, clip(LR, 1 +- c) adv))
(ppo_clip.py:47-54), then surr_after and the old/new KL, and
set_param_values(new, set_new=True, set_old=True).

Device work: the minibatch steps run on the GPU as replays of one captured step
(algos/_device_sgd.py; the likelihood ratio != 1 gradient the NPG path never
needs), with the old log-likelihoods computed once for all rows when the old
parameters are fixed during the call (see _old_on_device for when they are not).  surr_before / surr_after / kl_dist come
from the HIP engine's forward / evaluation passes (CPI_surrogate, kl_old_new).
train_step is BatchREINFORCE's (device GAE), handing the paths with their
advantages to train_from_paths.  fit_backend = "hip" (opt-in, per instance or on
the class) runs the minibatch steps as the fused kernel of csrc/policy_fit.hip
instead (mb_size <= 64, MLP policies up to 64 units wide), fit_backend =
"hip_wide" as the sliced kernels of csrc/policy_fit_wide.hip (hidden layers up to 256
units), fit_backend = "hip_rows" as the row-tiled kernels of csrc/policy_fit_rows.hip
(mb_size <= 16384, widths up to 64).  Single process: the minibatch order is global,
so a sharded PPO is not offered (comm must be local).

train_from_rollout (a step-major rollout already in GPU memory) is the base class's
ingest, carry and baseline fit around the same update with nothing on the host: the
engine's advantage stage leaves the whitened f32 advantages in HBM, the minibatch
steps read them and the packed batch's f32 rows in place (_update_from_batch).
minibatch_draw = "device" (opt-in, either route) draws each epoch's indices on the
GPU from the agent's own counter-based stream instead of numpy's global RNG
(csrc/minibatch.hip; _device_sgd.minibatch_indices_reference is the definition).
"""
import time as timer

import numpy as np
import torch

from .batch_reinforce import BatchREINFORCE
from ._device_sgd import (MINIBATCH_DRAWS, ROWS_BACKEND, DeviceTrainer, check_fit_backend, choice_batches,
                          default_device, device_choice_batches)
from ..utils.logger import DataLog


class PPO(BatchREINFORCE):
    _poolable = False   # the minibatch order is global: one process, even with MJRL_AMD_DEVICES set
    # "torch": a captured graph of torch ops per minibatch step; "hip": the fused kernel of
    # csrc/policy_fit.hip (opt-in, per instance or on the class); "hip_wide": the sliced
    # kernels of csrc/policy_fit_wide.hip for hidden layers up to 256 units (opt-in too); "hip_rows": the
    # row-tiled kernels of csrc/policy_fit_rows.hip for minibatches of up to 16384 rows (opt-in too)
    fit_backend = "torch"
    # where an epoch's minibatch indices are drawn: "numpy" (np.random.choice from numpy's global RNG on the
    # host, the reference's draws, uploaded per epoch) or "device" (opt-in, per instance or on the class:
    # the counter-based stream of csrc/minibatch.hip under the agent's seed, draw counter kept on the agent
    # and pickled with it; numpy's RNG is left untouched)
    minibatch_draw = "numpy"

    def __init__(self, env, policy, baseline, clip_coef=0.2, epochs=10, mb_size=64, learn_rate=3e-4, seed=0,
                 save_logs=False, device=None, comm=None):
        super().__init__(env, policy, baseline, learn_rate=learn_rate, seed=seed, save_logs=save_logs,
                         device=device, comm=comm)
        self.learn_rate = learn_rate
        self.clip_coef = clip_coef
        self.epochs = epochs
        self.mb_size = mb_size
        if save_logs:
            self.logger = DataLog()
        self.optimizer = torch.optim.Adam(self.policy.trainable_params, lr=learn_rate)
        self._trainer = None
        self._draw_first = 0   # minibatch_draw = "device": the next draw of the agent's stream

    def __getstate__(self):
        d = super().__getstate__()
        d["_trainer"] = None
        d["_step_rows"] = None   # device tensors
        # pickle gives every tensor a storage of its own: which old parameters share
        # theirs with the new ones (_old_on_device) is part of the agent's state
        d["_shared"] = self._aliasing()
        return d

    def __setstate__(self, d):
        d = dict(d)
        shared = d.pop("_shared", None) or []
        self.__dict__.update(d)
        for s, o, n in zip(shared, self.policy.old_params, self.policy.trainable_params):
            if s:
                o.data = n.data

    def trainer(self):
        if self._trainer is None:
            self._trainer = DeviceTrainer(self.policy, self.optimizer, self.engine().device)
        return self._trainer

    def _update(self, batch, paths, skip_gae=False, gamma=0.995, gae_lambda=None):
        # train_step -> train_from_samples: the device GAE wrote the advantages into
        # the path dicts; PPO's own train_from_paths takes it from there.  paths None
        # (train_from_rollout): there are no path dicts, the batch's rows are the data
        if paths is None:
            return self._update_from_batch(batch, gamma, gae_lambda)
        return self.train_from_paths(paths)

    def _check_draw(self):
        """minibatch_draw's value and, for "device", the trainer device, before
        anything touches the GPU library."""
        if self.minibatch_draw not in MINIBATCH_DRAWS:
            raise ValueError("PPO.minibatch_draw must be one of %s, not %r" % (MINIBATCH_DRAWS, self.minibatch_draw))
        if self.minibatch_draw == "device" and default_device(self._device).type != "cuda":
            raise ValueError('PPO.minibatch_draw = "device" draws on the GPU, not on the %s trainer device'
                             % default_device(self._device))

    def _epoch_batches(self, num_samples, dev):
        """One epoch's minibatch indices [nmb][mb] on the device: numpy's global RNG
        (choice_batches) or the agent's own stream (minibatch_draw = "device": seed
        self.seed, draws self._draw_first onwards)."""
        if self.minibatch_draw == "numpy":
            return choice_batches(num_samples, self.mb_size, dev)
        batches, self._draw_first = device_choice_batches(self.seed or 0, getattr(self, "_draw_first", 0),
                                                          num_samples, self.mb_size, dev)
        return batches

    def _old_on_device(self, tr):
        """The old parameters as the minibatch steps see them.  The reference's
        set_param_values(p, set_new=True, set_old=True) (gaussian_mlp.py:66-89)
        hands the same float32 array to the new and the old parameters, so after
        any previous update they share storage (log_std excepted: its clamp makes a
        new tensor) and the optimizer's in-place steps move the old mean network
        with the new one (the likelihood ratio then only sees the log_std change).
        The same aliasing exists in this package's policy classes; a shared tensor
        is mirrored as the live device parameter (detached: the old branch carries
        no gradient), any other as a frozen copy.  Returns (list, any aliased)."""
        out, aliased = [], False
        for i, (o, n) in enumerate(zip(self.policy.old_params, self.policy.trainable_params)):
            if o.data.data_ptr() == n.data.data_ptr() and o.data.shape == n.data.shape:
                out.append(tr.params[i].detach())
                aliased = True
            else:
                out.append(o.data.to(tr.device))
        return out, aliased

    def _aliasing(self):
        """Per parameter tensor: do the old and the new policy share storage (see
        _old_on_device)?  Host pointers only."""
        return [o.data.data_ptr() == n.data.data_ptr() and o.data.shape == n.data.shape
                for o, n in zip(self.policy.old_params, self.policy.trainable_params)]

    def _check_backend(self):
        hip = check_fit_backend("PPO", self.fit_backend, self.policy, self.optimizer, self.mb_size, self._device)
        if hip and self._aliasing() not in ([False] * 7, [True] * 6 + [False]):
            raise ValueError('PPO.fit_backend = "%s" takes old parameters that share no storage with the new ones, '
                             "or the six mean-network tensors shared and log_std not (what set_param_values "
                             "leaves), not %r" % (self.fit_backend, self._aliasing()))
        return hip

    def train_from_paths(self, paths):
        if self.comm().world_size > 1:
            raise NotImplementedError("PPO's minibatch order is global (ppo_clip.py:89-91): run it in one process")
        self._check_draw()
        hip = self._check_backend()
        observations = np.concatenate([path["observations"] for path in paths])
        actions = np.concatenate([path["actions"] for path in paths])
        advantages = np.concatenate([path["advantages"] for path in paths])
        advantages = (advantages - np.mean(advantages)) / (np.std(advantages) + 1e-6)
        path_returns = [sum(p["rewards"]) for p in paths]
        mean_return = np.mean(path_returns)
        std_return = np.std(path_returns)
        min_return = np.amin(path_returns)
        max_return = np.amax(path_returns)
        base_stats = [mean_return, std_return, min_return, max_return]
        self.running_score = mean_return if self.running_score is None else \
            0.9 * self.running_score + 0.1 * mean_return
        if self.save_logs:
            self.log_rollout_statistics(paths)

        surr_before = float(self.CPI_surrogate(observations, actions, advantages))
        ts = timer.time()
        dev = self.trainer().device
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        self._minibatch_steps(t(observations), t(actions), t(advantages), hip)   # adv f32 as ppo_clip.py:48
        params_after_opt = self.policy.get_param_values()
        surr_after = float(self.CPI_surrogate(observations, actions, advantages))
        kl_dist = float(self.kl_old_new(observations, actions))
        self.policy.set_param_values(params_after_opt, set_new=True, set_old=True)
        t_opt = timer.time() - ts
        if self.save_logs:
            self._log_opt(t_opt, kl_dist, surr_after - surr_before)
            self._log_success(paths)
        return base_stats

    def _log_opt(self, t_opt, kl_dist, surr_improvement):
        self.logger.log_kv("t_opt", t_opt)
        self.logger.log_kv("kl_dist", kl_dist)
        self.logger.log_kv("surr_improvement", surr_improvement)
        self.logger.log_kv("running_score", self.running_score)

    def _minibatch_steps(self, O, A, ADV, hip):
        """The epochs of minibatch Adam steps on this call's f32 device rows O [T][n],
        A [T][m], ADV [T] (ppo_clip.py:88-96): parameters and optimizer state to the
        device, epochs x int(T / mb_size) steps, both back to the CPU policy."""
        tr = self.trainer()
        tr.pull()
        dev = tr.device
        old_dev, aliased = self._old_on_device(tr)
        c = float(self.clip_coef)
        if not aliased:
            # the old parameters are fixed during the call: LL_old once for all rows
            with torch.no_grad():
                LL_old = tr.log_likelihood(O, A, old_dev)

        def mb_loss(idx):
            adv = ADV.index_select(0, idx)
            o, a = O.index_select(0, idx), A.index_select(0, idx)
            if aliased:
                with torch.no_grad():
                    ll_old = tr.log_likelihood(o, a, old_dev)
            else:
                ll_old = LL_old.index_select(0, idx)
            LR = torch.exp(tr.log_likelihood(o, a) - ll_old)
            LR_clip = torch.clamp(LR, min=1 - c, max=1 + c)
            return -torch.mean(torch.min(LR * adv, LR_clip * adv))

        num_samples = int(O.shape[0])
        # the captured step reads this call's O / A / ADV / LL_old: a new key per call
        self._ncall = getattr(self, "_ncall", 0) + 1
        for ep in range(self.epochs):
            batches = self._epoch_batches(num_samples, dev)
            if hip:
                tr.fused_epoch("ppo", O, A, batches, adv=ADV, ll_old=None if aliased else LL_old,
                               old_log_std=old_dev[-1].contiguous() if aliased else None, clip=c,
                               wide=self.fit_backend == "hip_wide", rows=self.fit_backend == ROWS_BACKEND)
            else:
                tr.epoch(("ppo", self._ncall), mb_loss, batches)
        tr.push()

    # ---- the device-rollout route ---------------------------------------------------
    def train_from_rollout(self, observations, actions, rewards, done, terminated=None, steps=None, gamma=0.995,
                           gae_lambda=0.98, fit_baseline=True, carry=None, bootstrap_returns=False):
        """BatchREINFORCE.train_from_rollout (the same arguments, baselines, carry,
        bootstrap_returns, LinearBaseline fit and episode_returns(): the base class's
        code) with PPO's update between the ingest and the fit, all on the device:
        the engine's advantage stage leaves the whitened f32 advantages in HBM, the
        minibatch steps read them and the packed batch's own f32 rows in place (an f64
        rollout is cast to f32 once on the device), surr_before / surr_after / kl_dist
        come from the engine's forward and evaluation passes over the same rows.  With
        minibatch_draw = "device" no host work is left per minibatch.  One GPU in
        this process; fit_backend's and minibatch_draw's limits are checked before
        anything touches the GPU library."""
        self._check_draw()
        self._check_backend()
        return super().train_from_rollout(observations, actions, rewards, done, terminated=terminated, steps=steps,
                                          gamma=gamma, gae_lambda=gae_lambda, fit_baseline=fit_baseline, carry=carry,
                                          bootstrap_returns=bootstrap_returns)

    def _check_rollout(self, *args):
        try:
            return super()._check_rollout(*args)
        except ValueError as e:   # the argument's name, under the class's
            raise ValueError("%s.train_from_rollout: %s" % (type(self).__name__, e)) from None

    def _update_from_batch(self, batch, gamma, gae_lambda):
        """train_from_paths' update on a batch that lies in HBM (no path dicts): see
        train_from_rollout.  Sets last_update (base_stats, surr_before, surr_after,
        kl_dist, T)."""
        hip = self._check_backend()
        eng = self.engine()
        # GAE, returns, moments, whitening (adv - mean) / (std + 1e-6) and the forward
        # pass at the old parameters: the engine's stages, as an NPG update runs them
        T = eng.load_batch(batch, self._theta(old=True), gamma, gae_lambda)
        surr_before, _ = eng.eval_pass(self._theta(), T)
        base_stats = eng.path_return_stats()
        mean_return = base_stats[0]
        self.running_score = mean_return if self.running_score is None else \
            0.9 * self.running_score + 0.1 * mean_return
        if self.save_logs:
            self.logger.log_kv("stoc_pol_mean", base_stats[0])
            self.logger.log_kv("stoc_pol_std", base_stats[1])
            self.logger.log_kv("stoc_pol_max", base_stats[3])
            self.logger.log_kv("stoc_pol_min", base_stats[2])
        ts = timer.time()
        O, A = batch.obs[:T], batch.act[:T]
        if O.dtype != torch.float32:   # an f64 rollout: one cast on the device, as t() on the host route
            O, A = O.float(), A.float()
        ADV = eng.ws["adv32"][:T]
        self._step_rows = (O, A, ADV)   # what the steps read (views of the batch and the workspace; for tests)
        self._minibatch_steps(O, A, ADV, hip)
        params_after_opt = self.policy.get_param_values()
        # CPI_surrogate and kl_old_new after the steps: one forward pass at the old
        # parameters (as they are now: _old_on_device) and one evaluation at the new
        eng.forward_pass(self._theta(old=True), T)
        surr_after, kl_dist = (float(v) for v in eng.eval_pass(self._theta(), T))
        self.policy.set_param_values(params_after_opt, set_new=True, set_old=True)
        t_opt = timer.time() - ts
        self.last_update = dict(base_stats=base_stats, surr_before=float(surr_before), surr_after=surr_after,
                                kl_dist=kl_dist, T=T)
        if self.save_logs:
            self._log_opt(t_opt, kl_dist, surr_after - float(surr_before))
        return base_stats
