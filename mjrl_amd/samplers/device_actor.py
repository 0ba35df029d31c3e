"""The device actor: the policy's actions for the
environments of a batched GPU simulator, sampled where the observations lie.

policy.get_action (mjrl/policies/gaussian_mlp.py:91-98) is mean + exp(log_std) *
randn(m) per observation on the host.  mjrl_policy_act (csrc/act.hip) does the same
for [E][n] observations in GPU memory in one launch: the mean network on row tiles,
the Gaussian noise from a counter-based generator in the same kernel, and the
action (optionally also the mean, the noise and a copy of the observations) written
straight into the step-major slabs that DeviceBatch.from_rollout /
train_from_rollout take.  DeviceActor wraps that launch; DeviceRollout owns the
slabs of one H-step collection.

This module also states the noise in NumPy (philox4x32, noise_reference): the
definition the kernel is tested against.  The noise of env e at step t is a
function of (seed, t, e, column) alone, so sub-batches of environments and
rollouts split over several calls draw the same numbers.  Importing this module
never loads the GPU library; the argument checks run before it is loaded.
"""
import numpy as np

U32 = np.uint32
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_SHIFT = np.uint64(32)


def philox4x32(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al. 2011; Random123's philox4x32):
    counter = four and key = two uint32 words (scalars or arrays that broadcast).
    Returns the four output words as uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & _MASK for x in key]
    if len(c) != 4 or len(k) != 2:
        raise ValueError("philox4x32 takes a 4-word counter and a 2-word key")
    for r in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _SHIFT) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _SHIFT) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
    return tuple(x.astype(U32) for x in c)


def _box_muller(xa, xb):
    """Two f32 standard normals from two uint32 words: u1 = ((xa >> 8) + 1) 2^-24 in
    (0, 1], u2 = (xb >> 8) 2^-24 in [0, 1) (both exact in f32), r = sqrt(-2 log u1),
    th = f32(2 pi) u2, (r cos th, r sin th); every operation in f32."""
    f = np.float32
    u1 = ((xa >> U32(8)) + U32(1)).astype(f) * f(2.0 ** -24)
    u2 = (xb >> U32(8)).astype(f) * f(2.0 ** -24)
    r = np.sqrt(f(-2.0) * np.log(u1))
    th = f(6.283185307179586) * u2
    return (r * np.cos(th)).astype(f), (r * np.sin(th)).astype(f)


def noise_reference(seed, step, env0, E, m):
    """The standard normals mjrl_policy_act draws for envs env0 .. env0 + E - 1 at
    `step` under `seed`: float32 [E][m].  For env e and the block b = j >> 2 of four
    columns the counter is (step lo, step hi, (env0 + e) lo, b) and the key (seed lo,
    seed hi); the words (x0, x1) give columns 4b and 4b + 1, (x2, x3) columns 4b + 2
    and 4b + 3."""
    seed, step, env0, E, m = int(seed), int(step), int(env0), int(E), int(m)
    if step < 0 or E < 0 or m < 1:
        raise ValueError("noise_reference needs step >= 0, E >= 0 and m >= 1, got %d, %d, %d" % (step, E, m))
    nb = (m + 3) // 4
    env = ((env0 + np.arange(E, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint64)[:, None]
    blk = np.arange(nb, dtype=np.uint64)[None, :]
    x = philox4x32((step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, env + 0 * blk, blk + 0 * env),
                   (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    out = np.empty((E, nb, 4), dtype=np.float32)
    out[:, :, 0], out[:, :, 1] = _box_muller(x[0], x[1])
    out[:, :, 2], out[:, :, 3] = _box_muller(x[2], x[3])
    return np.ascontiguousarray(out.reshape(E, 4 * nb)[:, :m])


def _check_out(name, t, shape, dtype, obs):
    import torch
    if t is None:
        return
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch tensor on the GPU, got %s" % (name, type(t).__name__))
    if tuple(t.shape) != shape:
        raise ValueError("%s must be [%d][%d], got shape %r" % (name, shape[0], shape[1], tuple(t.shape)))
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.device != obs.device:
        raise ValueError("%s is on %s, obs on %s: one device" % (name, t.device, obs.device))
    if not t.is_contiguous():
        raise ValueError("%s must be C-contiguous" % name)


def check_act(n, m, obs, out=None, mean_out=None, eps_out=None, obs_out=None, step=None, env0=0, device=None):
    """The argument checks of DeviceActor.act, made before the GPU library is
    loaded: obs a C-contiguous [E][n] float32 or float64 tensor on the GPU (on
    `device` when given); out [E][m] and obs_out [E][n] in obs's dtype, mean_out
    and eps_out [E][m] float32, all C-contiguous on obs's device; step (when given)
    and env0 non-negative integers.  Returns E; raises ValueError naming the
    argument."""
    import torch
    if not isinstance(obs, torch.Tensor):
        raise ValueError("obs must be a torch tensor on the GPU, got %s" % type(obs).__name__)
    if obs.dim() != 2 or obs.shape[1] != n:
        raise ValueError("obs must be [E][n = %d], got shape %r" % (n, tuple(obs.shape)))
    if obs.dtype not in (torch.float32, torch.float64):
        raise ValueError("obs must be float32 or float64, got %s" % obs.dtype)
    if not obs.is_cuda:
        raise ValueError("obs is a CPU tensor: the device actor reads observations already in GPU memory "
                         "(host observations go through sample_paths_vectorized)")
    if device is not None:
        d = torch.device(device)
        if d.type != obs.device.type or (d.index is not None and d.index != obs.device.index):
            raise ValueError("obs is on %s, the actor on %s: one device" % (obs.device, d))
    if not obs.is_contiguous():
        raise ValueError("obs must be C-contiguous")
    E = int(obs.shape[0])
    _check_out("out", out, (E, m), obs.dtype, obs)
    _check_out("mean_out", mean_out, (E, m), torch.float32, obs)
    _check_out("eps_out", eps_out, (E, m), torch.float32, obs)
    _check_out("obs_out", obs_out, (E, n), obs.dtype, obs)
    for name, v in (("step", step), ("env0", env0)):
        if v is not None and (int(v) != v or v < 0 or v >= 2 ** 63):
            raise ValueError("%s must be a non-negative integer below 2^63, got %r" % (name, v))
    return E


class DeviceActor:
    """get_action for [E][n] observations in GPU memory: one mjrl_policy_act launch
    per call on the current stream, no host synchronisation.  Composes the vector
    sampler's BatchedPolicy for the packed parameters and the transformations
    (built at the first launch, so the argument checks need no GPU)."""

    def __init__(self, policy, device=None, seed=0):
        if int(seed) != seed or not 0 <= seed < 2 ** 64:
            raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
        self.policy, self.seed, self.step = policy, int(seed), 0
        self.device = device
        self._bp = None
        self.sigma = None

    def _batched(self, device):
        if self._bp is None:
            import torch
            from .vector_sampler import BatchedPolicy
            self.device = torch.device(device)
            self._bp = BatchedPolicy(self.policy, self.device)
            self._set_sigma()
        return self._bp

    def _set_sigma(self):
        import torch
        # float32(exp(log_std)) of the clamped log_std: get_action's np.exp(log_std_val)
        ls = np.maximum(self._bp.log_std_val, np.float64(self.policy.min_log_std))
        self.sigma = torch.from_numpy(np.exp(ls).astype(np.float32)).to(self.device)

    def refresh(self):
        """Re-packs the policy's parameters and transformations after an update and
        recomputes sigma.  The step counter keeps running."""
        if self._bp is not None:
            self._bp.refresh()
            self._set_sigma()

    def act(self, obs, out=None, mean_out=None, eps_out=None, obs_out=None, step=None, env0=0, evaluation=False):
        """The actions [E][m] (obs's dtype; `out` when given) for obs [E][n]:
        mean + sigma * eps with eps the noise of (seed, step, env0 + e, column), or the
        mean itself with evaluation=True.  mean_out / eps_out (float32 [E][m]) and
        obs_out ([E][n], a verbatim copy of obs) are filled when given.  step=None
        uses the actor's counter self.step and advances it."""
        import torch
        from .. import _lib
        n, m = self.policy.n, self.policy.m
        E = check_act(n, m, obs, out, mean_out, eps_out, obs_out, step, env0, self.device)
        bp = self._batched(obs.device)
        if step is None:
            step = self.step
            self.step += 1
        eng = bp.eng
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty((E, m), dtype=obs.dtype, device=self.device)
            ins, isc, osh, osc = eng.transforms
            eng.K.mjrl_policy_act(eng.shape, obs, int(obs.dtype == torch.float64), E, bp.packed, ins, isc, osh, osc,
                                  None if evaluation else self.sigma, self.seed, int(step), int(env0), out, mean_out,
                                  eps_out, obs_out, _lib.stream_ptr())
        return out


class DeviceRollout:
    """The step-major slabs of one H-step collection on E environments, filled in
    place: observations [H][E][n] and actions [H][E][m] (dtype), rewards [H][E]
    (reward_dtype), done and terminated [H][E] uint8.

        for t in range(H):
            a = ro.act(obs)                    # one launch: stores obs, writes and returns actions[t]
            obs, r, d, term = sim.step(a)
            ro.record(r, d, term)
        agent.train_from_rollout(*ro.tensors(), carry=carry)
        ro.refresh(); ro.reset()
    """

    def __init__(self, policy, E, H, device=None, seed=0, dtype=None, reward_dtype=None):
        import torch
        dtype = torch.float32 if dtype is None else dtype
        reward_dtype = torch.float64 if reward_dtype is None else reward_dtype
        if int(E) != E or int(H) != H or E < 1 or H < 1:
            raise ValueError("DeviceRollout needs E >= 1 environments and H >= 1 steps, got E = %r, H = %r" % (E, H))
        floats = (torch.float32, torch.float64)
        if dtype not in floats or reward_dtype not in floats:
            raise ValueError("dtype and reward_dtype must be float32 or float64, got %s, %s" % (dtype, reward_dtype))
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("mjrl_amd device rollouts live in GPU memory; no GPU is visible")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.E, self.H, self.dtype = int(E), int(H), dtype
        self.actor = DeviceActor(policy, self.device, seed)
        n, m = policy.n, policy.m
        self.observations = torch.zeros((self.H, self.E, n), dtype=dtype, device=self.device)
        self.actions = torch.zeros((self.H, self.E, m), dtype=dtype, device=self.device)
        self.rewards = torch.zeros((self.H, self.E), dtype=reward_dtype, device=self.device)
        self.done = torch.zeros((self.H, self.E), dtype=torch.uint8, device=self.device)
        self.terminated = torch.zeros((self.H, self.E), dtype=torch.uint8, device=self.device)
        self.t, self._acted = 0, False

    def act(self, obs, evaluation=False):
        """actions[t] for the observations obs [E][n] of step t, which are stored in
        observations[t] by the same launch."""
        if self.t >= self.H:
            raise ValueError("act: the rollout is full (t == H = %d); call tensors() and reset()" % self.H)
        if self._acted:
            raise ValueError("act: step %d already has its actions; record(rewards, done) comes next" % self.t)
        import torch
        if isinstance(obs, torch.Tensor) and obs.dim() == 2 and obs.shape[0] != self.E:
            raise ValueError("obs must be [E = %d][n = %d], got shape %r"
                             % (self.E, self.actor.policy.n, tuple(obs.shape)))
        if isinstance(obs, torch.Tensor) and obs.dtype != self.dtype:
            raise ValueError("obs must be %s (the rollout's dtype), got %s" % (self.dtype, obs.dtype))
        a = self.actor.act(obs, out=self.actions[self.t], obs_out=self.observations[self.t], evaluation=evaluation)
        self._acted = True
        return a

    def record(self, rewards, done, terminated=None):
        """The simulator's answer to actions[t]: rewards [E], done [E] and terminated
        [E] (None: every end is a true termination) into row t; t advances."""
        if not self._acted:
            raise ValueError("record: step %d has no actions yet; act(obs) comes first" % self.t)
        import torch
        named = [("rewards", rewards, self.rewards), ("done", done, self.done),
                 ("terminated", done if terminated is None else terminated, self.terminated)]
        for name, v, _ in named:
            if not isinstance(v, torch.Tensor) or tuple(v.shape) != (self.E,):
                raise ValueError("%s must be a torch tensor [E = %d], got %s" %
                                 (name, self.E, tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__))
            if v.device != self.device:
                raise ValueError("%s is on %s, the rollout on %s: one device" % (name, v.device, self.device))
        for _, v, slab in named:
            slab[self.t].copy_(v)
        self.t += 1
        self._acted = False

    def tensors(self):
        """(observations, actions, rewards, done, terminated) of the full rollout, as
        train_from_rollout takes them."""
        if self.t != self.H or self._acted:
            raise ValueError("tensors: the rollout has %d of H = %d steps recorded" % (self.t, self.H))
        return self.observations, self.actions, self.rewards, self.done, self.terminated

    def reset(self):
        """Starts the next collection at t = 0.  The noise step counter keeps running."""
        self.t, self._acted = 0, False

    def refresh(self):
        self.actor.refresh()
