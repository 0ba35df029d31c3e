"""Minibatch first-order training of a Gaussian policy on the GPU, shared by BC
(behavior_cloning.py) and PPO (ppo_clip.py) — SURVEY.md §8f row f4.

The CPU policy (mjrl_amd.policies.*) and the caller's CPU optimizer over
policy.trainable_params stay the source of truth, exactly the objects the
reference trains (behavior_cloning.py:37, ppo_clip.py:44).  Around a training
call, DeviceTrainer copies the parameters and the optimizer state to the device,
runs every minibatch step there, and copies both back, so pickling, CPU sampling
and a later call (Adam moments carried over, as the reference's optimizer
carries them) see the same state the reference would leave.

A minibatch step — gather the rows named by a device index buffer, the policy
mean (functional form of MuNet / LinearModel, gaussian_mlp.py:143-182), the
loss, backward, the optimizer step — is captured once as a hipGraph and replayed
per minibatch (capturable Adam); the minibatch indices come from numpy's global
RNG in the reference's order, drawn for a whole epoch up front and uploaded in one
copy (choice_batches), or, with PPO.minibatch_draw = "device", drawn on the device by
one launch per epoch from a counter-based stream of the agent's own (csrc/minibatch.hip,
device_choice_batches; minibatch_indices_reference states the draw in NumPy).
Optimizers without a capturable mode run the same step eagerly.

fit_backend = "hip" on BC / PPO (opt-in) replaces the graph replays of an epoch by
one mjrl_policy_fit_epoch call (csrc/policy_fit.hip) on the same device
parameters and the device optimizer's moments: DeviceTrainer.fused_epoch, limits
in check_fit_backend.  fit_backend = "hip_wide" (opt-in too) is the
same step sliced over workgroups for hidden layers up to 256 units wide
(csrc/policy_fit_wide.hip, mjrl_policy_fit_wide_epoch): fused_epoch(..., wide=True).
fit_backend = "hip_rows" (opt-in too) is the same step sliced over row tiles, one workgroup
per 64 rows, for minibatches of up to 16384 rows at the narrow backend's widths
(csrc/policy_fit_rows.hip, mjrl_policy_fit_rows_epoch): fused_epoch(..., rows=True).

MSE behaviour cloning (behavior_cloning_2.py) trains policy.model.parameters()
alone: DeviceTrainer(..., params=...) mirrors that list instead of
policy.trainable_params, and fused_epoch("mse", ...) is mjrl_policy_mse_epoch.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from .. import _device_fit as _fit
from .._device_fit import HIP_MAX_BATCH

# PPO's, BC's and behavior_cloning_2.BC's fit_backend (MLPBaseline keeps _device_fit.FIT_BACKENDS)
POLICY_FIT_BACKENDS = ("torch", "hip", "hip_wide")
# PPO's and BC's fourth: the row-tiled kernels of csrc/policy_fit_rows.hip (the MSE head has none)
ROWS_BACKEND = "hip_rows"
HIP_ROWS_MAX_BATCH = 16384   # rows of a minibatch they take (MJRL_POLICY_FIT_ROWS_MAX_BS)

LOG_2PI = float(np.log(2 * np.pi))


def default_device(device=None):
    if device is not None:
        return torch.device(device)
    if torch.cuda.is_available():
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cpu")


class DeviceTrainer:
    def __init__(self, policy, optimizer, device=None, params=None):
        """params: the CPU tensors this trainer mirrors and trains, policy.trainable_params
        unless given (behavior_cloning_2.py trains policy.model.parameters() alone)."""
        self.policy = policy
        self.cpu_opt = optimizer
        self.device = default_device(device)
        self._cpu_params = None if params is None else list(params)
        self.params = [torch.zeros(p.shape, dtype=torch.float32, device=self.device, requires_grad=True)
                       for p in self.cpu_params]
        self.graphable = self.device.type == "cuda" and "capturable" in optimizer.defaults
        kw = dict(optimizer.defaults)
        if self.graphable:
            kw["capturable"] = True
        self.opt = type(optimizer)(self.params, **kw)
        self._graphs = {}
        self._tf = None

    @property
    def cpu_params(self):
        return self.policy.trainable_params if self._cpu_params is None else self._cpu_params

    # ---- CPU <-> device ------------------------------------------------------
    def pull(self):
        """policy params + optimizer state (CPU) -> device."""
        with torch.no_grad():
            for d, c in zip(self.params, self.cpu_params):
                d.copy_(c.data)
        _fit.state_to_device(self.cpu_opt, self.cpu_params, self.opt, self.params, self.device,
                             self.graphable)
        for gd, gc in zip(self.opt.param_groups, self.cpu_opt.param_groups):
            for k, v in gc.items():
                if k not in ("params", "capturable", "foreach", "fused", "differentiable"):
                    gd[k] = v
        t = self.policy.model.transformations
        dev = self.device
        f = lambda v, fill, k: torch.from_numpy(np.float32(v)).to(dev) if v is not None else \
            torch.full((k,), float(fill), device=dev)
        tf = (f(t["in_shift"], 0.0, self.policy.n), f(t["in_scale"], 1.0, self.policy.n),
              f(t["out_shift"], 0.0, self.policy.m), f(t["out_scale"], 1.0, self.policy.m))
        if self._tf is None:
            self._tf = tf
        else:
            # copied into the existing buffers: a captured step reads them by address
            for d, s in zip(self._tf, tf):
                d.copy_(s)

    def push(self):
        """device params + optimizer state -> the CPU policy / optimizer (the
        Parameter objects keep their identity: the CPU optimizer stays bound)."""
        with torch.no_grad():
            for d, c in zip(self.params, self.cpu_params):
                c.data.copy_(d.detach().cpu())
        _fit.state_to_cpu(self.cpu_opt, self.cpu_params, self.opt, self.params)

    # ---- the policy on the device -----------------------------------------------
    def mean(self, obs, params=None):
        """policy.model(obs) for device rows (gaussian_mlp.py:168-182 / gaussian_linear.py)."""
        p = self.params if params is None else params
        ins, isc, osh, osc = self._tf
        h = (obs - ins) / (isc + 1e-8)
        if self.policy.hidden is None:
            out = F.linear(h, p[0], p[1])
        else:
            h = torch.tanh(F.linear(h, p[0], p[1]))
            h = torch.tanh(F.linear(h, p[2], p[3]))
            out = F.linear(h, p[4], p[5])
        return out * osc + osh

    def log_likelihood(self, obs, act, params=None):
        """mean_LL (gaussian_mlp.py:100-108): -0.5 sum z^2 - sum log_std - 0.5 m log 2 pi."""
        p = self.params if params is None else params
        log_std = p[-1]
        zs = (act - self.mean(obs, p)) / torch.exp(log_std)
        return -0.5 * torch.sum(zs ** 2, dim=1) + -torch.sum(log_std) + -0.5 * self.policy.m * LOG_2PI

    # ---- minibatch steps ------------------------------------------------------------
    def epoch(self, key, loss_fn, idx_batches):
        """One pass over idx_batches (device i64 [nmb][mb]): per row of it, the
        step zero_grad -> loss_fn(idx) -> backward -> optimizer step.  `key`
        names the captured graph: a replay re-reads the tensors loss_fn closed
        over at capture, so a caller gives every new set of data a new key."""
        nmb = int(idx_batches.shape[0])
        if nmb == 0:
            return
        mb = int(idx_batches.shape[1])
        g = self._graph(key, loss_fn, mb) if self.graphable else None
        for i in range(nmb):
            if g is not None:
                g[1].copy_(idx_batches[i])
                g[0].replay()
            else:
                self.opt.zero_grad()
                loss_fn(idx_batches[i]).backward()
                self.opt.step()

    def _graph(self, key, loss_fn, mb):
        hyper = tuple((k, v) for g in self.opt.param_groups for k, v in sorted(g.items())
                      if k != "params" and isinstance(v, (int, float, bool, tuple)))
        gkey = (key, mb, hyper)   # hyperparameters are baked into a captured step
        if gkey in self._graphs:
            return self._graphs[gkey]
        self._graphs.clear()   # a graph holds its closure's data buffers: keep only the live one
        dev = self.device
        idx = torch.zeros(mb, dtype=torch.int64, device=dev)

        def body():
            self.opt.zero_grad(set_to_none=False)
            loss_fn(idx).backward()
            self.opt.step()

        graph = _fit.capture_step(body, self.params, self.opt, dev)
        self._graphs[gkey] = (graph, idx)
        return self._graphs[gkey]

    # ---- the fused route (fit_backend = "hip") -------------------------------------------
    def fused_epoch(self, kind, obs, act, idx_batches, adv=None, ll_old=None, old_log_std=None, clip=0.0,
                    wide=False, rows=False):
        """epoch()'s steps as one mjrl_policy_fit_epoch call (csrc/policy_fit.hip) on
        the current stream: self.params and the device optimizer's exp_avg /
        exp_avg_sq are updated in place, then every step counter advances by nmb.
        kind: "bc" or "ppo"; obs / act / adv / ll_old: this call's f32 device rows;
        old_log_std: PPO's aliased form (PPO._old_on_device) instead of ll_old.
        kind "mse": mjrl_policy_mse_epoch on a trainer over the six tensors of
        policy.model.parameters() (behavior_cloning_2.py), obs / act alone.
        wide: the sliced kernels of csrc/policy_fit_wide.hip (hidden layers up to 256
        units; mjrl_policy_fit_wide_epoch / mjrl_policy_mse_wide_epoch) on the same
        parameters and moments, with a scratch of their own.
        rows: the row-tiled kernels of csrc/policy_fit_rows.hip (minibatches of up to 16384
        rows, "bc" and "ppo"; mjrl_policy_fit_rows_epoch), with a scratch of their own that
        grows with the minibatch."""
        from .. import _lib
        nmb, bs = int(idx_batches.shape[0]), int(idx_batches.shape[1])
        if nmb == 0:
            return
        dev = self.device
        _fit.ensure_adam_state(self.opt, self.params, dev)   # a fresh optimizer has no state yet
        given = [t for t in (obs, act, adv, ll_old, old_log_std) if t is not None]
        if any(t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev for t in given) \
                or obs.shape[1] != self.policy.n or act.shape[1] != self.policy.m:
            raise ValueError("the fused policy fit takes contiguous f32 rows obs [T][n], act [T][m] on the trainer's device")
        idx_batches = idx_batches.contiguous()
        mse = kind == "mse"
        if rows and (wide or mse):
            raise ValueError("the row-tiled policy fit has neither a wide nor an MSE form")
        K = _lib.calls()
        dims = (self.policy.n, self.policy.m, *self.policy.hidden, bs)
        if rows:
            # the slab of the tiles' gradients grows with bs: a later call may need a larger one
            skey, scratch = "_hip_rows_scratch", getattr(self, "_hip_rows_scratch", None)
            need = C.c_int64()
            K.mjrl_policy_fit_rows_scratch(*dims, need)
            if scratch is not None and scratch.numel() < need.value:
                scratch = None
            scratch = _fit.scratch(scratch, K.mjrl_policy_fit_rows_scratch, dims, dev)
        else:
            skey = "_hip_wide_scratch" if wide else "_hip_scratch"
            scratch = _fit.scratch(getattr(self, skey, None),
                                   K.mjrl_policy_fit_wide_scratch if wide else K.mjrl_policy_fit_scratch, dims, dev)
        setattr(self, skey, scratch)
        if len(self.params) != (6 if mse else 7):
            raise ValueError("the fused %s fit trains %s" % (kind, "policy.model.parameters()" if mse
                                                             else "policy.trainable_params"))
        net = _fit.fill_net(_lib.MeanNet() if mse else _lib.PolicyNet(), self.opt, self.params)
        ptr = lambda t: None if t is None else t.data_ptr()
        data = _lib.PolicyFitData(ptr(obs), ptr(act), ptr(adv), ptr(ll_old), ptr(old_log_std),
                                  *[t.data_ptr() for t in self._tf], int(obs.shape[0]), self.policy.n, self.policy.m,
                                  self.policy.hidden[0], self.policy.hidden[1],
                                  _lib.POLICY_FIT_PPO if kind == "ppo" else _lib.POLICY_FIT_BC, float(clip))
        hp = _fit.adam_hp(self.opt, self.params)
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(torch.cuda.current_stream(dev))
            if rows:
                K.mjrl_policy_fit_rows_epoch(data, idx_batches, nmb, bs, net, hp, scratch, None, None, stream)
            elif wide:
                (K.mjrl_policy_mse_wide_epoch if mse else K.mjrl_policy_fit_wide_epoch)(
                    data, idx_batches, nmb, bs, net, hp, scratch, None, None, stream)
            else:
                (K.mjrl_policy_mse_epoch if mse else K.mjrl_policy_fit_epoch)(
                    data, idx_batches, nmb, bs, net, hp, scratch, 0, None, None, stream)
        _fit.advance_steps(self.opt, self.params, nmb)


HIP_MAX_WIDTH = 64    # the fused kernel's largest hidden / action width (csrc/policy_fit.hip)
HIP_WIDE_MAX_WIDTH = 256   # the sliced kernels' largest hidden width (csrc/policy_fit_wide.hip); actions stay at 64


def check_fit_backend(who, backend, policy, optimizer, mb_size, device, mean_only=False):
    """The fused route's limits, each a ValueError naming it, before anything
    touches the GPU library.  Returns True when the backend is "hip", "hip_wide"
    (the same checks, hidden widths 1..256) or "hip_rows" (the same checks, minibatches of
    1..16384 rows; not with mean_only).
    mean_only: the MSE fit's net, the optimizer over policy.model.parameters() alone."""
    if backend not in POLICY_FIT_BACKENDS and backend != ROWS_BACKEND:
        raise ValueError("%s.fit_backend must be one of %s, not %r" % (who, POLICY_FIT_BACKENDS, backend)
                         + ("" if mean_only else ' (or "%s" for minibatches above %d rows)'
                            % (ROWS_BACKEND, HIP_MAX_BATCH)))
    if backend == "torch":
        return False
    pre = '%s.fit_backend = "%s"' % (who, backend)
    if backend == ROWS_BACKEND and mean_only:
        raise ValueError("%s: the MSE head has no row-tiled kernel (csrc/policy_fit_rows.hip builds the BC and "
                         "PPO heads); take \"hip\" or \"hip_wide\"" % pre)
    max_h = HIP_WIDE_MAX_WIDTH if backend == "hip_wide" else HIP_MAX_WIDTH
    max_b = HIP_ROWS_MAX_BATCH if backend == ROWS_BACKEND else HIP_MAX_BATCH
    if not 1 <= int(mb_size) <= max_b:
        raise ValueError("%s takes minibatches of 1..%d rows, not %d" % (pre, max_b, mb_size))
    hidden = policy.hidden
    if hidden is None:
        raise ValueError("%s trains the Gaussian MLP policy (two hidden layers), not a LinearPolicy" % pre)
    if len(hidden) != 2 or not all(1 <= int(h) <= max_h for h in hidden) or not 1 <= policy.m <= HIP_MAX_WIDTH:
        if max_h == HIP_MAX_WIDTH:
            raise ValueError("%s takes two hidden layers and an action width of 1..%d units each, not %r / %d"
                             % (pre, HIP_MAX_WIDTH, tuple(hidden), policy.m))
        raise ValueError("%s takes two hidden layers of 1..%d units each and an action width of 1..%d, not %r / %d"
                         % (pre, max_h, HIP_MAX_WIDTH, tuple(hidden), policy.m))
    if type(optimizer) is not torch.optim.Adam:
        raise ValueError("%s takes a torch.optim.Adam optimizer, not %s" % (pre, type(optimizer).__name__))
    if len(optimizer.param_groups) != 1:
        raise ValueError("%s takes an Adam optimizer with one parameter group, not %d"
                         % (pre, len(optimizer.param_groups)))
    g = optimizer.param_groups[0]
    if g.get("amsgrad", False) or g.get("maximize", False):
        raise ValueError("%s takes Adam with amsgrad=False and maximize=False" % pre)
    if mean_only:
        want, have = list(policy.model.parameters()), g["params"]
        if len(have) != len(want) or any(a is not b for a, b in zip(have, want)):
            raise ValueError("%s takes an Adam optimizer over exactly policy.model.parameters(), in their order "
                             "(log_std is not trained), not over %d tensors" % (pre, len(have)))
    if default_device(device).type != "cuda":
        raise ValueError("%s runs on the GPU, not on the %s trainer device" % (pre, default_device(device)))
    return True


def choice_batches(num_samples, mb_size, device):
    """int(num_samples / mb_size) draws of np.random.choice(num_samples, mb_size)
    from numpy's global RNG, in the reference's order (behavior_cloning.py:58-59,
    ppo_clip.py:90-91), as one device tensor [nmb][mb]."""
    nmb = int(num_samples / mb_size)
    if nmb == 0:
        return torch.zeros((0, mb_size), dtype=torch.int64, device=device)
    idx = np.stack([np.random.choice(num_samples, size=mb_size) for _ in range(nmb)]).astype(np.int64)
    return torch.from_numpy(idx).to(device)


# PPO.minibatch_draw: "numpy" is choice_batches above, "device" the counter-based
# stream of csrc/minibatch.hip (device_choice_batches)
MINIBATCH_DRAWS = ("numpy", "device")
DRAW_KEY_TAG = 0x4D425849   # "MBXI": keeps the draws' stream apart from the actor's noise under one seed
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhi64(u, t):
    """The high 64 bits of u * t, u a uint64 array and t an int in [0, 2^64), on
    32-bit limbs (every partial product and sum fits a uint64)."""
    ul, uh = u & _M32, u >> _S32
    tl, th = np.uint64(t & 0xFFFFFFFF), np.uint64(t >> 32)
    lh, hl = ul * th, uh * tl
    carry = ((ul * tl >> _S32) + (lh & _M32) + (hl & _M32)) >> _S32
    return uh * th + (lh >> _S32) + (hl >> _S32) + carry


def minibatch_indices_reference(seed, first, count, T):
    """The definition of mjrl_minibatch_indices (csrc/minibatch.hip) in NumPy: draws
    first .. first + count - 1 of the stream of `seed`, int64 [count], each uniform on
    [0, T) with replacement as np.random.choice(T, mb) is.  Draw g is a function of
    (seed, g, T) alone: block b = g >> 1 of Philox4x32-10 on the counter (b lo, b hi, 0,
    0) under the key (seed lo, seed hi ^ DRAW_KEY_TAG), u = x0 | x1 << 32 for even g and
    x2 | x3 << 32 for odd g, the index the high 64 bits of u T (bias at most T / 2^64).
    Never loads the GPU library."""
    from ..samplers.device_actor import philox4x32
    seed, first, count, T = int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(count), int(T)
    if T < 1 or first < 0 or count < 0 or first + count > 2 ** 63 - 1:
        raise ValueError("minibatch_indices_reference needs T >= 1, first >= 0, count >= 0 and draws below 2^63, "
                         "got %d, %d, %d" % (T, first, count))
    g = first + np.arange(count, dtype=np.int64)
    b = (g >> 1).astype(np.uint64)
    x = philox4x32((b & _M32, b >> _S32, 0 * b, 0 * b), (seed & 0xFFFFFFFF, (seed >> 32) ^ DRAW_KEY_TAG))
    odd = (g & 1).astype(bool)
    u = np.where(odd, x[2], x[0]).astype(np.uint64) | np.where(odd, x[3], x[1]).astype(np.uint64) << _S32
    return _mulhi64(u, T).astype(np.int64)


def device_choice_batches(seed, first, num_samples, mb_size, device):
    """choice_batches' [nmb][mb] device tensor for one epoch, drawn on the device
    (mjrl_minibatch_indices on the current stream: no host RNG, no upload): draws first
    .. first + nmb mb - 1 of the stream of `seed` (minibatch_indices_reference,
    reshaped).  Returns (the tensor, the next first)."""
    from .. import _lib
    device = torch.device(device)
    nmb = int(num_samples / mb_size)
    out = torch.empty((nmb, mb_size), dtype=torch.int64, device=device)
    if nmb:
        with torch.cuda.device(device):
            _lib.calls().mjrl_minibatch_indices(int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), nmb * mb_size,
                                                int(num_samples), out, _lib.stream_ptr())
    return out, int(first) + nmb * mb_size
