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

Every path is a trajectory of its own: the baselines' time features restart at 0
in each one, in the first path of a rollout too.  A rollout that continues an
episode of the previous call is therefore out of scope.
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


def segment_rollout_reference(done, terminated=None, steps=None):
    """The cut of a [H][E] done board, in NumPy.  Returns a dict:
    P, T; paths: list of (env, t0, length, terminated) in path order; path_off
    int64 [P + 1]; path_term uint8 [P]; R int64 [E + 1] (the first row of each
    env; R[E] = T)."""
    done = _host(done)
    if done.ndim != 2:
        raise ValueError("done must be [H][E], got shape %r" % (done.shape,))
    H, E = done.shape
    term = None if terminated is None else _host(terminated)
    if term is not None and term.shape != done.shape:
        raise ValueError("terminated must have done's shape %r, got %r" % (done.shape, term.shape))
    s = check_steps(steps, H, E)
    R = np.concatenate([[0], np.cumsum(s)]).astype(np.int64)
    paths = []
    for e in range(E):
        t0 = 0
        for t in range(int(s[e])):
            if done[t, e]:
                paths.append((e, t0, t + 1 - t0, bool(term[t, e]) if term is not None else True))
                t0 = t + 1
        if t0 < s[e]:
            paths.append((e, t0, int(s[e]) - t0, False))
    off = np.array([R[e] + t0 for e, t0, _, _ in paths] + [R[E]], dtype=np.int64)
    return dict(P=len(paths), T=int(R[E]), paths=paths, path_off=off,
                path_term=np.array([p[3] for p in paths], dtype=np.uint8), R=R)


def rollout_rows(x, steps):
    """The valid cells of a step-major array x [H][E][...] in row order
    (env-ascending, then time-ascending): [T][...]."""
    x = _host(x)
    s = check_steps(steps, x.shape[0], x.shape[1])
    parts = [x[:int(s[e]), e] for e in range(x.shape[1])]
    return np.concatenate(parts) if parts else x.reshape((0,) + x.shape[2:])


def rollout_to_paths(observations, actions, rewards, done, terminated=None, steps=None):
    """The rollout as the list of sampler-format paths DeviceBatch.from_rollout cuts
    it into (mjrl/samplers/base_sampler.py:76-83: observations [L][n], actions
    [L][m], rewards [L] as float64, agent_infos, env_infos, terminated).  Host
    NumPy; takes NumPy arrays or torch tensors of any device."""
    obs, act, rew = _host(observations), _host(actions), _host(rewards)
    seg = segment_rollout_reference(done, terminated, steps)
    if obs.ndim != 3 or act.ndim != 3 or obs.shape[:2] != rew.shape or act.shape[:2] != rew.shape \
            or rew.shape != _host(done).shape:
        raise ValueError("observations [H][E][n], actions [H][E][m], rewards [H][E] and done [H][E] must agree, got "
                         "%r %r %r %r" % (obs.shape, act.shape, rew.shape, _host(done).shape))
    return [dict(observations=np.array(obs[t0:t0 + L, e], dtype=np.float64),
                 actions=np.array(act[t0:t0 + L, e], dtype=np.float64),
                 rewards=np.array(rew[t0:t0 + L, e], dtype=np.float64),
                 agent_infos={}, env_infos={}, terminated=bool(term))
            for e, t0, L, term in seg["paths"]]


def check_rollout(observations, actions, rewards, done, terminated=None, steps=None):
    """The argument checks of DeviceBatch.from_rollout, made before the GPU library
    is loaded (shapes, dtypes, steps, then devices): C-contiguous torch tensors on
    one GPU, observations [H][E][n] and actions [H][E][m] of one floating dtype
    (float32 or float64), rewards [H][E] float32 or float64, done (and
    terminated) [H][E] uint8 or bool, steps E integers in [0, H] or None.  Returns
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
