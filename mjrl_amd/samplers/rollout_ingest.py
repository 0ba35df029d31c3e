"""Step-major rollouts of auto-reset environments, cut into trajectories.

A batched simulator steps E environments together for H steps and leaves
observations [H][E][n], actions [H][E][m], rewards [H][E] and done [H][E]; an
environment whose episode ends resets itself and goes on.  The update reads
path-major rows (np.concatenate over the sampler's paths, mjrl/algos/npg_cg.py:87-89).
DeviceBatch.from_rollout (mjrl_amd/engine.py) makes that batch on the device
(csrc/ingest.hip); this module is the host side: the same cut in NumPy
(segment_rollout_reference: what tests and documentation compare the kernels
with), the equivalent list of sampler-format paths (rollout_to_paths: for
logging, and as the comparison route), and the argument checks.  It never loads
the GPU library.

The cut, as csrc/ingest.hip states it: env e has steps[e] valid steps (H when
steps is None); a cell (t, e) with t >= steps[e] is never read.  Env e's valid
steps are cut after every cell with done != 0; such a path's `terminated` is
terminated[t][e] != 0 (True when terminated is None: every end is a true
termination, bootstrap 0; a time limit is a done cell with terminated 0,
bootstrap b[-1], as process_samples.py:24-27 tells them apart).  A non-empty
remainder is a last path with terminated False.  Paths are ordered env-ascending,
then time-ascending, so the row of cell (t, e) is R[e] + t with R the exclusive
prefix sum of steps.

The carry: batched simulators step thousands of auto-reset environments for a few
dozen steps per update, so an env's first path is usually the middle of an episode
and its last one an open fragment.  Per env e, c[e] >= 0 (`episode_steps`) is the
number of steps its running episode had taken before cell (0, e).  The cut itself
does not change; beside it:
  path_t0[p] = c[e] when p is env e's path that starts at t = 0, else 0: the time
    origin of the baselines' time features, (arange(L) + t0) / 1000;
  env_path [E + 1]: the index of env e's first path, env_path[E] = P (an env with
    no steps has env_path[e] == env_path[e + 1]);
  c_next[e] (`episode_steps_next`), with t0 the start of the env's last path: c[e]
    if steps[e] == 0; 0 if cell (steps[e] - 1, e) is done; else (steps[e] - t0) +
    (c[e] if t0 == 0 else 0).
Cutting a board at any step and feeding the first part's c_next into the second
gives every row the episode time it has on the uncut board, and the same final
c_next.  Without a carry (None: zeros) every path is a trajectory of its own, its
time features starting at 0, as before.  RolloutCarry holds c (and the return each
running episode has collected) on the device between calls.
"""
import numpy as np


def _host(a):
    """A NumPy view / copy of a NumPy array or a torch tensor (any device)."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def check_steps(steps, H, E):
    """`steps` as int64 [E] (None: every env has H steps), each in [0, H]."""
    if steps is None:
        return np.full(E, H, dtype=np.int64)
    s = np.asarray(_host(steps))
    if s.shape != (E,) or s.dtype.kind not in "iu":
        raise ValueError("steps must be a sequence of %d integers (one per env), got shape %r dtype %s"
                         % (E, s.shape, s.dtype))
    s = s.astype(np.int64)
    if s.size and (s.min() < 0 or s.max() > H):
        raise ValueError("steps must lie in [0, H = %d], got [%d, %d]" % (H, s.min(), s.max()))
    return s


def check_episode_steps(episode_steps, E):
    """The carry as int64 [E] (None: zeros), each >= 0."""
    if episode_steps is None:
        return np.zeros(E, dtype=np.int64)
    c = np.asarray(_host(episode_steps))
    if c.shape != (E,) or c.dtype.kind not in "iu":
        raise ValueError("episode_steps must be %d integers (one per env), got shape %r dtype %s"
                         % (E, c.shape, c.dtype))
    c = c.astype(np.int64)
    if c.size and c.min() < 0:
        raise ValueError("episode_steps must be >= 0, got a minimum of %d" % c.min())
    return c


def segment_rollout_reference(done, terminated=None, steps=None, episode_steps=None):
    """The cut of a [H][E] done board, in NumPy.  Returns a dict:
    P, T; paths: list of (env, t0, length, terminated) in path order; path_off
    int64 [P + 1]; path_term uint8 [P]; R int64 [E + 1] (the first row of each
    env; R[E] = T); and with the carry episode_steps (int64 [E], None: zeros):
    path_t0 int64 [P], env_path int64 [E + 1], episode_steps_next int64 [E]."""
    done = _host(done)
    if done.ndim != 2:
        raise ValueError("done must be [H][E], got shape %r" % (done.shape,))
    H, E = done.shape
    term = None if terminated is None else _host(terminated)
    if term is not None and term.shape != done.shape:
        raise ValueError("terminated must have done's shape %r, got %r" % (done.shape, term.shape))
    s = check_steps(steps, H, E)
    c = check_episode_steps(episode_steps, E)
    R = np.concatenate([[0], np.cumsum(s)]).astype(np.int64)
    paths, env_path, c_next = [], [0], np.zeros(E, dtype=np.int64)
    for e in range(E):
        t0 = 0
        for t in range(int(s[e])):
            if done[t, e]:
                paths.append((e, t0, t + 1 - t0, bool(term[t, e]) if term is not None else True))
                t0 = t + 1
        if t0 < s[e]:
            paths.append((e, t0, int(s[e]) - t0, False))
        c_next[e] = c[e] if s[e] == 0 else (0 if t0 == s[e] else (s[e] - t0) + (c[e] if t0 == 0 else 0))
        env_path.append(len(paths))
    off = np.array([R[e] + t0 for e, t0, _, _ in paths] + [R[E]], dtype=np.int64)
    return dict(P=len(paths), T=int(R[E]), paths=paths, path_off=off,
                path_term=np.array([p[3] for p in paths], dtype=np.uint8), R=R,
                path_t0=np.array([c[e] if t0 == 0 else 0 for e, t0, _, _ in paths], dtype=np.int64),
                env_path=np.array(env_path, dtype=np.int64), episode_steps_next=c_next)


def rollout_rows(x, steps):
    """The valid cells of a step-major array x [H][E][...] in row order
    (env-ascending, then time-ascending): [T][...]."""
    x = _host(x)
    s = check_steps(steps, x.shape[0], x.shape[1])
    parts = [x[:int(s[e]), e] for e in range(x.shape[1])]
    return np.concatenate(parts) if parts else x.reshape((0,) + x.shape[2:])


def rollout_to_paths(observations, actions, rewards, done, terminated=None, steps=None, episode_steps=None):
    """The rollout as the list of sampler-format paths DeviceBatch.from_rollout cuts
    it into (mjrl/samplers/base_sampler.py:76-83: observations [L][n], actions
    [L][m], rewards [L] as float64, agent_infos, env_infos, terminated).  With a
    carry (episode_steps int64 [E], zeros included) every path also has "t0": the
    steps its episode had taken before its first row (episode_steps[e] for env e's
    path that starts at t = 0, else 0), which LinearBaseline's time features start
    from; without one the dicts are the sampler's, key for key.  Host NumPy; takes
    NumPy arrays or torch tensors of any device."""
    obs, act, rew = _host(observations), _host(actions), _host(rewards)
    seg = segment_rollout_reference(done, terminated, steps, episode_steps)
    if obs.ndim != 3 or act.ndim != 3 or obs.shape[:2] != rew.shape or act.shape[:2] != rew.shape \
            or rew.shape != _host(done).shape:
        raise ValueError("observations [H][E][n], actions [H][E][m], rewards [H][E] and done [H][E] must agree, got "
                         "%r %r %r %r" % (obs.shape, act.shape, rew.shape, _host(done).shape))
    paths = [dict(observations=np.array(obs[t0:t0 + L, e], dtype=np.float64),
                  actions=np.array(act[t0:t0 + L, e], dtype=np.float64),
                  rewards=np.array(rew[t0:t0 + L, e], dtype=np.float64),
                  agent_infos={}, env_infos={}, terminated=bool(term))
             for e, t0, L, term in seg["paths"]]
    if episode_steps is not None:
        for p, c in zip(paths, seg["path_t0"]):
            p["t0"] = int(c)
    return paths


class RolloutCarry:
    """What E auto-reset environments carry from one rollout to the next, on the
    device: episode_steps int64 [E], the steps each env's running episode has taken
    (DeviceBatch.from_rollout(carry=) reads it and updates it in place), and
    episode_return float64 [E], the rewards that episode has collected
    (train_from_rollout(carry=) updates it).  Both start at zero: every env at the
    start of an episode."""

    def __init__(self, E, device):
        import torch
        if int(E) != E or E < 0:
            raise ValueError("RolloutCarry: E must be a non-negative integer, got %r" % (E,))
        self.E, self.device = int(E), torch.device(device)
        self.episode_steps = torch.zeros(self.E, dtype=torch.int64, device=self.device)
        self.episode_return = torch.zeros(self.E, dtype=torch.float64, device=self.device)

    def reset(self, mask=None):
        """Back to the start of an episode: every env, or those where mask [E] (a
        bool tensor or array) is set — environments the caller reset by hand."""
        if mask is None:
            self.episode_steps.zero_()
            self.episode_return.zero_()
            return
        import torch
        m = torch.as_tensor(_host(mask) if not isinstance(mask, torch.Tensor) else mask)
        if tuple(m.shape) != (self.E,):
            raise ValueError("RolloutCarry.reset: mask must be [E = %d], got shape %r" % (self.E, tuple(m.shape)))
        m = m.to(self.device).bool()
        self.episode_steps.masked_fill_(m, 0)
        self.episode_return.masked_fill_(m, 0.0)


def check_carry(carry, E, device):
    """from_rollout's checks of its carry: a RolloutCarry of E envs whose tensors
    are int64 / float64 [E] on the rollout's device.  Raises ValueError naming the
    argument."""
    import torch
    if carry is None:
        return None
    if not isinstance(carry, RolloutCarry):
        raise ValueError("carry must be a RolloutCarry (samplers.rollout_ingest), got %s" % type(carry).__name__)
    for name, tdt in (("episode_steps", torch.int64), ("episode_return", torch.float64)):
        t = getattr(carry, name)
        if not isinstance(t, torch.Tensor):
            raise ValueError("carry.%s must be a torch tensor, got %s" % (name, type(t).__name__))
        if tuple(t.shape) != (E,):
            raise ValueError("carry.%s holds %r envs, the rollout has E = %d" % (name, tuple(t.shape), E))
        if t.device != device:
            raise ValueError("carry.%s is on %s, the rollout on %s: one device" % (name, t.device, device))
        if t.dtype != tdt:
            raise ValueError("carry.%s must be %s, got %s" % (name, tdt, t.dtype))
        if not t.is_contiguous():
            raise ValueError("carry.%s must be C-contiguous" % name)
    return carry


def check_rollout(observations, actions, rewards, done, terminated=None, steps=None, carry=None):
    """The argument checks of DeviceBatch.from_rollout, made before the GPU library
    is loaded (shapes, dtypes, steps, then devices): C-contiguous torch tensors on
    one GPU, observations [H][E][n] and actions [H][E][m] of one floating dtype
    (float32 or float64), rewards [H][E] float32 or float64, done (and
    terminated) [H][E] uint8 or bool, steps E integers in [0, H] or None, carry a
    RolloutCarry of E envs on the same device or None.  Returns
    (H, E, n, m, steps as int64 [E]); raises ValueError naming the argument."""
    import torch
    named = [("observations", observations), ("actions", actions), ("rewards", rewards), ("done", done)]
    if terminated is not None:
        named.append(("terminated", terminated))
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a torch tensor on the GPU, got %s" % (name, type(t).__name__))
    if observations.dim() != 3 or observations.shape[2] < 1:
        raise ValueError("observations must be [H][E][n], got shape %r" % (tuple(observations.shape),))
    H, E, n = (int(v) for v in observations.shape)
    if actions.dim() != 3 or tuple(actions.shape[:2]) != (H, E) or actions.shape[2] < 1:
        raise ValueError("actions must be [H = %d][E = %d][m], got shape %r" % (H, E, tuple(actions.shape)))
    for name, t in named[2:]:
        if tuple(t.shape) != (H, E):
            raise ValueError("%s must be [H = %d][E = %d], got shape %r" % (name, H, E, tuple(t.shape)))
    floats = (torch.float32, torch.float64)
    if observations.dtype not in floats:
        raise ValueError("observations must be float32 or float64, got %s" % observations.dtype)
    if actions.dtype != observations.dtype:
        raise ValueError("actions are %s, observations %s: the engine takes both in one dtype"
                         % (actions.dtype, observations.dtype))
    if rewards.dtype not in floats:
        raise ValueError("rewards must be float32 or float64, got %s" % rewards.dtype)
    for name, t in named[3:]:
        if t.dtype not in (torch.uint8, torch.bool):
            raise ValueError("%s must be uint8 or bool, got %s" % (name, t.dtype))
    steps = check_steps(steps, H, E)
    check_carry(carry, E, observations.device)
    for name, t in named:
        if t.device != observations.device:
            raise ValueError("%s is on %s, observations on %s: one device" % (name, t.device, observations.device))
    for name, t in named:
        if not t.is_cuda:
            raise ValueError("%s is a CPU tensor: from_rollout takes rollouts already in GPU memory "
                             "(host paths go through DeviceBatch.from_paths)" % name)
        if not t.is_contiguous():
            raise ValueError("%s must be C-contiguous" % name)
    return H, E, n, int(actions.shape[2]), steps
