"""Vectorised trajectory sampling: N environments stepped
in lock step, the policy's mean action for all of them from one device launch
per step (mjrl_policy_mean, csrc/rollout.hip) instead of N per-observation CPU
forwards (policy.get_action, mjrl/policies/gaussian_mlp.py:92-98).  The
environments (MuJoCo) stay on the CPU.

Each trajectory is the one mjrl/samplers/base_sampler.py:do_rollout (:39-83)
produces for the same pegasus seed: trajectory ep seeds its environment with
seed + ep, draws its action noise exp(log_std) * randn(m) per step from its own
numpy stream seeded with seed + ep (the reference re-seeds numpy's global RNG
per trajectory and draws nothing else from it inside the loop), resets under
that stream (env resets that use the global RNG see the state the reference's
would), stops at done or T = min(T, env.horizon) steps, and is returned in the
sampler wire format (observations, actions, rewards, agent_infos, env_infos,
terminated).  Paths come back in trajectory order; numpy's global RNG is left
as the reference leaves it (the last trajectory's stream).  The mean action is
the f32 MuNet forward (index-order f32 sums: equal to the CPU forward up to f32
rounding).  With num_workers >= 1 the environments are stepped by worker
processes (env_workers.py) and the forward reads their observation board
(mjrl_policy_mean_slots); the trajectories are the same.
"""
import numpy as np
import torch

from .. import _lib
from ..engine import UpdateEngine
from .samples_schedule import SamplesSchedule


class BatchedPolicy:
    """The policy's mean network on the device for a batch of observations."""

    def __init__(self, policy, device=None):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("mjrl_amd batched sampling runs the policy forward on the GPU; none is visible")
            device = torch.device("cuda", torch.cuda.current_device())
        self.policy = policy
        self.device = torch.device(device)
        self.eng = UpdateEngine(policy.n, policy.m, policy.hidden, device=self.device,
                                min_log_std=policy.min_log_std)
        self.packed = torch.zeros(self.eng.shape.packed, dtype=torch.float32, device=self.device)
        self.refresh()

    def refresh(self):
        """Re-packs the policy's current (new) parameters and transformations."""
        eng = self.eng
        with torch.cuda.device(self.device):
            eng.set_transformations(*self.policy.transformations())
            theta = torch.from_numpy(np.ascontiguousarray(self.policy.get_param_values(), dtype=np.float32))
            theta = eng._pad(theta.to(self.device), "act")
            eng.K.mjrl_pack_params(eng.shape, theta, self.packed, 0, eng.min_log_std, _lib.stream_ptr())
        self.log_std_val = np.float64(self.policy.log_std.data.numpy().ravel())

    def means(self, observations):
        """f32 [N][m] mean actions for observations [N][n] (numpy)."""
        eng = self.eng
        N = int(observations.shape[0])
        with torch.cuda.device(self.device):
            obs = torch.from_numpy(np.ascontiguousarray(observations, dtype=np.float32)).to(self.device)
            out = torch.empty((N, self.policy.m), dtype=torch.float32, device=self.device)
            ins, isc, osh, osc = eng.transforms
            eng.K.mjrl_policy_mean(eng.shape, obs, N, self.packed, ins, isc, osh, osc, out, _lib.stream_ptr())
            return out.cpu().numpy()

    def _board_set(self, S):
        """The device and pinned buffers of means_slots for S slots, kept across steps."""
        b = getattr(self, "_boards", None)
        if b is None or b[0].shape[0] != S:
            with torch.cuda.device(self.device):
                b = self._boards = (
                    torch.empty((S, self.policy.n), dtype=torch.float64, device=self.device),
                    torch.empty((S,), dtype=torch.int32, device=self.device),
                    torch.empty((S, self.policy.m), dtype=torch.float32, device=self.device),
                    torch.empty((S,), dtype=torch.int32).pin_memory(),
                    torch.empty((S, self.policy.m), dtype=torch.float32).pin_memory())
        return b

    def obs_board(self, S):
        """The device copy of the observation board (f64 [S][n]) that means_slots
        fills every lock step on the current stream: after a means_slots call it
        holds that step's observations until the next call's copy, which is
        ordered behind whatever was queued on that stream in between (a
        StreamSink forms the value features from it: attach_board)."""
        return self._board_set(int(S))[0]

    def means_slots(self, obs_board, live, out=None):
        """The mean actions of the environment slots `live` (distinct indices < S)
        of an observation board obs_board [S][n] (f64 numpy; a view of registered
        host memory is copied by DMA): f32 [S][m] (numpy, `out` when given) whose
        rows live[i] are bitwise means(float32(obs_board[live])) and whose other
        rows are not defined.  The board goes to a device buffer with an async
        copy and the kernel (mjrl_policy_mean_slots) reads that buffer; when this
        returns the copy out of obs_board has completed."""
        eng = self.eng
        S, E = int(obs_board.shape[0]), len(live)
        if out is None:
            out = np.empty((S, self.policy.m), np.float32)
        if E == 0:
            return out
        with torch.cuda.device(self.device):
            d_obs, d_live, d_mean, h_live, h_mean = self._board_set(S)
            h_live[:E] = torch.from_numpy(np.asarray(live, dtype=np.int32))
            d_obs.copy_(torch.from_numpy(np.ascontiguousarray(obs_board, dtype=np.float64)), non_blocking=True)
            d_live[:E].copy_(h_live[:E], non_blocking=True)
            ins, isc, osh, osc = eng.transforms
            eng.K.mjrl_policy_mean_slots(eng.shape, d_obs, d_live, E, S, self.packed, ins, isc, osh, osc, d_mean,
                                         _lib.stream_ptr())
            h_mean.copy_(d_mean, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            out[live] = h_mean.numpy()[live]
        return out


def _seed_env(env, seed):
    try:
        env.env._seed(seed)
    except AttributeError:
        env.env.seed(seed)


def _stack(dicts):
    """tensor_utils.stack_tensor_dict_list: a list of (nested) dicts -> a dict of arrays."""
    if not dicts:
        return {}
    out = {}
    for k, v in dicts[0].items():
        vals = [d[k] for d in dicts]
        out[k] = _stack(vals) if isinstance(v, dict) else np.array(vals)
    return out


class _Slot:
    __slots__ = ("env", "ep", "rs", "o", "t", "obs", "act", "rew", "ainfo", "einfo", "idx")


def _with_board(sink, bp, S):
    """The sink (or sink factory) of a worker-stepped sampling call, given the
    device observation board of bp.means_slots when it can use one (a sink with
    an attach_board method); any other sink is passed on as it is."""
    if sink is None:
        return None
    if callable(sink):
        def make(*args):
            s = sink(*args)
            if hasattr(s, "attach_board"):
                s.attach_board(bp.obs_board(S))
            return s
        return make
    if hasattr(sink, "attach_board"):
        sink.attach_board(bp.obs_board(S))
    return sink


def sample_paths_vectorized(N, policy, T=1e6, env=None, env_name=None, pegasus_seed=None, num_envs=64,
                            device=None, sink=None, num_workers=0, worker_timeout=900.0,
                            sample_mode="trajectories"):
    """N trajectories on min(num_envs, N) lock-stepped environments.

    sample_mode="samples": N is a number of timesteps, and the paths returned are
    those of the reference's one-core loop (batch_sampler.py:58-103), whatever
    num_envs and num_workers are: trajectory k is the rollout seeded s0 + k (s0 =
    pegasus_seed, or 0 when it is None), and the list is the shortest prefix 0..K
    whose lengths sum to >= N ([] for N <= 0).  samples_schedule.py holds the rule
    by which trajectories start and sampling stops; a live trajectory with an
    index above K is abandoned (sink.abandon(slot)), and numpy's global RNG is left
    as trajectory K left it.  The sink is then one sized by rows
    (stream_staging.ChunkSink; the factory receives N timesteps).

    env: an environment factory (called once per slot) or None with env_name
    (mjrl.utils.get_environment, the reference's registry).  sink: a
    samplers.stream_staging.StreamSink (built with nslots >= min(num_envs, N)
    and horizon >= the trajectories' length) that receives every observation /
    action row as it is produced and stages each trajectory to HBM when it ends
    (sink.batch(paths) afterwards), or a factory sink(N, horizon, slots) that
    builds one.  The paths returned are the same either way.  With workers, a sink
    that has an attach_board method is handed the device observation board of the
    policy forward (BatchedPolicy.obs_board).

    num_workers: 0 steps every environment in this process; K >= 1 steps them in
    min(K, slots) worker processes (samplers/env_workers.py: the policy forward,
    the trajectory assignment and the sink stay here; the pool is kept for the
    next call).  env must then be env_name or a picklable factory (a
    module-level callable or a functools.partial of one).  The paths have the
    same keys, dtypes and shapes either way; with workers the observations are
    the f64 [H][n] rows np.asarray(o, float64).ravel() and the rewards f64,
    which is what num_workers=0 returns for environments whose observations
    are 1-D f64 arrays and whose rewards are Python floats (other dtypes and
    shapes are kept as they are by num_workers=0 only).  worker_timeout: the
    seconds any wait for the workers may take before the pool is torn down."""
    if sample_mode not in ("trajectories", "samples"):
        raise ValueError("sample_mode must be 'trajectories' or 'samples', got %r" % (sample_mode,))
    samples = sample_mode == "samples"
    if samples and pegasus_seed is None:
        pegasus_seed = 0   # batch_sampler.py:87
    if num_workers:
        if env is None and env_name is None:
            raise ValueError("sample_paths_vectorized needs env (a factory) or env_name")
        if N <= 0:
            return []
        from . import env_workers
        pool = env_workers.get_env_pool(env if env is not None else env_name, num_workers, min(int(num_envs), int(N)),
                                        policy.n, policy.m, worker_timeout)
        bp = BatchedPolicy(policy, device)
        pool.register_host()
        return env_workers.sample_paths(pool, N, bp.means_slots, bp.log_std_val, T, pegasus_seed,
                                        _with_board(sink, bp, pool.S), sample_mode=sample_mode)
    if env is None:
        if env_name is None:
            raise ValueError("sample_paths_vectorized needs env (a factory) or env_name")
        from mjrl.utils.get_environment import get_environment
        env = lambda: get_environment(env_name)   # noqa: E731
    if N <= 0:
        return []
    bp = BatchedPolicy(policy, device)
    scale = np.exp(bp.log_std_val)
    m = policy.m
    slots = []
    for _ in range(min(int(num_envs), int(N))):
        s = _Slot()
        s.env = env()
        slots.append(s)
    horizon = min(T, slots[0].env.horizon)
    if callable(sink):   # a factory: sink(N, horizon, slots)
        sink = sink(N, int(horizon), len(slots))
    if sink is not None and (sink.N != N or sink.H < horizon or len(sink.buf) < len(slots)):
        raise ValueError("StreamSink sized for %d paths x %d steps on %d slots; sampling %d x %d on %d"
                         % (sink.N, sink.H, len(sink.buf), N, horizon, len(slots)))
    for i, s in enumerate(slots):
        s.idx = i
    # samples mode: the paths and the streams' final states by trajectory index,
    # until the schedule knows which prefix is the batch
    sched = SamplesSchedule(N) if samples else None
    paths = {} if samples else [None] * N
    states = {}
    last_state = [None]
    next_ep = [0]

    def start(s):
        if sched is not None:
            if not sched.may_start():
                s.ep = None
                return
            s.ep = ep = sched.start()
        else:
            if next_ep[0] >= N:
                s.ep = None
                return
            s.ep = ep = next_ep[0]
            next_ep[0] += 1
        if pegasus_seed is not None:
            _seed_env(s.env, pegasus_seed + ep)
            s.rs = np.random.RandomState(pegasus_seed + ep)
        else:
            s.rs = np.random.RandomState()
        # the reset sees the trajectory's stream as numpy's global RNG (base_sampler.py:48-58)
        saved = np.random.get_state()
        np.random.set_state(s.rs.get_state())
        s.o = s.env.reset()
        s.rs.set_state(np.random.get_state())
        np.random.set_state(saved)
        s.t = 0
        s.obs, s.act, s.rew, s.ainfo, s.einfo = [], [], [], [], []
        if sink is not None:
            sink.begin(s.idx, ep)

    def finish(s, done):
        if sink is not None:
            sink.finish(s.idx, s.t, bool(done))
        paths[s.ep] = dict(observations=np.array(s.obs), actions=np.array(s.act), rewards=np.array(s.rew),
                           agent_infos=_stack(s.ainfo), env_infos=_stack(s.einfo), terminated=done)
        if sched is not None:
            states[s.ep] = s.rs.get_state()
            sched.end(s.ep)
        elif s.ep == N - 1:
            last_state[0] = s.rs.get_state()
        start(s)

    for s in slots:
        start(s)
    while True:
        live = [s for s in slots if s.ep is not None]
        if not live:
            break
        O = np.stack([np.asarray(s.o, dtype=np.float64).ravel() for s in live])
        means = bp.means(O)
        # every slot's action from its own stream (the draw order within a slot is
        # the reference's), then the environments step
        acts = [mean + scale * s.rs.randn(m) for s, mean in zip(live, means)]
        if sink is not None:
            idx, ts = [s.idx for s in live], [s.t for s in live]
            sink.rows(idx, O, ts)
            sink.actions(idx, np.stack(acts), ts)
        for s, mean, a in zip(live, means, acts):
            next_o, r, done, info = s.env.step(a)
            if sink is not None:
                sink.reward(s.idx, s.t, r)
            s.obs.append(s.o)
            s.act.append(a)
            s.rew.append(r)
            s.ainfo.append({"mean": mean, "log_std": bp.log_std_val, "evaluation": mean})
            s.einfo.append(info)
            s.o = next_o
            s.t += 1
            if sched is not None:
                sched.step(s.ep)
            if done == True or s.t >= horizon:   # noqa: E712 (base_sampler.py:61: done != True)
                finish(s, done)
        if sched is not None and sched.done:
            break
    if sched is not None:
        # the prefix 0..K is the batch; what is still live lies above K
        for s in slots:
            if s.ep is not None and sink is not None:
                sink.abandon(s.idx)
        paths = [paths[k] for k in range(sched.accepted)]
        last_state[0] = states[sched.K]
    if last_state[0] is not None:
        np.random.set_state(last_state[0])
    return paths
