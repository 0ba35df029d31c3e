"""Environment worker processes of the vector sampler (samplers/env_workers.py),
without a GPU: the mean provider is a row-wise CPU forward of the policy.  The
paths must be bitwise the ones a single-process lock-step loop produces with the
same provider, whatever the worker count; a failing environment tears the pool
down (no process, no segment) and the next call starts a fresh one; a worker
never imports torch."""
import functools
import subprocess
import time
from multiprocessing import shared_memory

import numpy as np
import pytest

from stub_env import StubEnv

N, SEED, NUM_ENVS = 37, 7, 8


class _FailInner:
    def __init__(self):
        self.rs = np.random.RandomState(0)
        self.seeded = None

    def seed(self, s):
        self.rs = np.random.RandomState(s)
        self.seeded = s


class FailingEnv(StubEnv):
    """StubEnv whose third step of the trajectory seeded `fail_seed` raises."""

    def __init__(self, fail_seed):
        super().__init__()
        self.env = _FailInner()
        self.fail_seed, self.k = fail_seed, 0

    def reset(self):
        self.k = 0
        return super().reset()

    def step(self, a):
        self.k += 1
        if self.env.seeded == self.fail_seed and self.k == 3:
            raise ArithmeticError("stub failure in trajectory seeded %d" % self.fail_seed)
        return super().step(a)


def _policy():
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    return MLP(EnvSpec(6, 2, 40, 1), hidden_sizes=(32, 32), seed=4, init_log_std=-0.5)


def _cpu_means(policy):
    """means(obs [S][n] f64, live, out [S][m] f32): one CPU forward per row (a row's
    result does not depend on which other rows are live)."""
    import torch

    def means(O, live, out):
        for s in live:
            with torch.no_grad():
                out[s] = policy.model(torch.from_numpy(np.float32(O[s].reshape(1, -1)))).numpy().ravel()
        return out
    return means


def _single_process(N, policy, env_fn, seed, num_envs, means):
    """The lock-step loop in this process: slot s takes the next trajectory when
    its last one ends (slot order), per-trajectory streams as
    base_sampler.do_rollout seeds them."""
    S, m = min(num_envs, N), policy.m
    envs = [env_fn() for _ in range(S)]
    horizon = envs[0].horizon
    scale, log_std = np.exp(policy.log_std_val), policy.log_std_val
    board, mean_b = np.zeros((S, policy.n)), np.zeros((S, m), np.float32)
    ep, rs, rec = [None] * S, [None] * S, [None] * S
    paths, nxt, last = [None] * N, 0, None

    def start(s):
        nonlocal nxt
        if nxt >= N:
            ep[s] = None
            return
        ep[s], nxt = nxt, nxt + 1
        envs[s].env.seed(seed + ep[s])
        rs[s] = np.random.RandomState(seed + ep[s])
        saved = np.random.get_state()
        np.random.set_state(rs[s].get_state())
        board[s] = envs[s].reset()
        rs[s].set_state(np.random.get_state())
        np.random.set_state(saved)
        rec[s] = dict(o=[], a=[], r=[], mean=[], info=[])

    for s in range(S):
        start(s)
    while any(e is not None for e in ep):
        live = np.array([s for s in range(S) if ep[s] is not None], np.int32)
        means(board, live, mean_b)
        for s in live:
            mean = mean_b[s].copy()
            a = mean + scale * rs[s].randn(m)
            o2, r, done, info = envs[s].step(a)
            R = rec[s]
            R["o"].append(board[s].copy()), R["a"].append(a), R["r"].append(r), R["mean"].append(mean)
            R["info"].append(info["norm"])
            board[s] = o2
            if done == True or len(R["r"]) >= horizon:   # noqa: E712
                L = len(R["r"])
                paths[ep[s]] = dict(observations=np.array(R["o"]), actions=np.array(R["a"]), rewards=np.array(R["r"]),
                                    agent_infos=dict(mean=np.array(R["mean"]), log_std=np.array([log_std] * L),
                                                     evaluation=np.array(R["mean"])),
                                    env_infos=dict(norm=np.array(R["info"])), terminated=done)
                if ep[s] == N - 1:
                    last = rs[s].get_state()
                start(s)
    np.random.set_state(last)
    return paths


def _same_tree(a, b, where=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), where
        for k in a:
            _same_tree(a[k], b[k], where + "/" + k)
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, where
        assert a.tobytes() == b.tobytes(), where
    else:
        assert type(a) is type(b) and a == b, where


def _same_paths(got, ref):
    assert len(got) == len(ref)
    for i, (p, q) in enumerate(zip(got, ref)):
        _same_tree(p, q, "path %d" % i)


def _rng_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.fixture(scope="module")
def policy():
    return _policy()


@pytest.fixture(scope="module", autouse=True)
def _close_pools():
    yield
    from mjrl_amd.samplers import env_workers
    env_workers.close_env_pools()


@pytest.fixture(scope="module")
def reference(policy):
    """The single-process paths for N = 37 on 8 slots and numpy's state after them."""
    np.random.seed(99)
    paths = _single_process(N, policy, StubEnv, SEED, NUM_ENVS, _cpu_means(policy))
    return paths, np.random.get_state()


def _run(policy, n_paths, workers, env=StubEnv, timeout=60.0):
    from mjrl_amd.samplers import env_workers
    pool = env_workers.get_env_pool(env, workers, min(NUM_ENVS, n_paths), policy.n, policy.m, timeout)
    return pool, env_workers.sample_paths(pool, n_paths, _cpu_means(policy), policy.log_std_val, 1e6, SEED)


def test_reference_batch_is_ragged(reference):
    paths, _ = reference
    assert any(p["terminated"] for p in paths) and any(len(p["rewards"]) == 40 and not p["terminated"] for p in paths)
    p = paths[0]
    assert p["observations"].dtype == np.float64 and p["agent_infos"]["mean"].dtype == np.float32
    assert p["agent_infos"]["log_std"].shape == p["actions"].shape


@pytest.mark.parametrize("workers,world", [(1, 1), (3, 3), (20, 8)])
def test_paths_are_bitwise_equal_across_worker_counts(policy, reference, workers, world):
    ref, rng = reference
    np.random.seed(99)
    pool, got = _run(policy, N, workers)
    assert pool.world == world   # contiguous ranges, as even as they go
    assert [hi - lo for lo, hi in pool.bounds] == [len(b) for b in np.array_split(range(8), world)]
    _same_paths(got, ref)
    assert _rng_equal(np.random.get_state(), rng)
    # the pool is kept: a second call reuses the same processes and gives the same paths
    pids = [h["pid"] for h in pool.hello]
    pool2, again = _run(policy, N, workers)
    assert pool2 is pool and [p.pid for p in pool._procs] == pids
    _same_paths(again, ref)


def test_fewer_trajectories_than_slots(policy):
    """N = 5 on num_envs = 8 with 3 workers: 5 slots, every one idle after its
    single trajectory."""
    ref = _single_process(5, policy, StubEnv, SEED, NUM_ENVS, _cpu_means(policy))
    rng = np.random.get_state()
    np.random.seed(1)
    pool, got = _run(policy, 5, 3)
    assert pool.S == 5 and pool.world == 3
    _same_paths(got, ref)
    assert _rng_equal(np.random.get_state(), rng)


def test_full_length_paths(policy):
    env = functools.partial(StubEnv, radius=1e9)
    ref = _single_process(11, policy, env, SEED, NUM_ENVS, _cpu_means(policy))
    _, got = _run(policy, 11, 3, env=env)
    assert all(len(p["rewards"]) == 40 and not p["terminated"] for p in got)
    _same_paths(got, ref)


def test_sink_sees_the_in_process_calls(policy, reference):
    """The sink protocol (begin, rows, actions, reward, finish) carries every row
    of every trajectory once, at its path index."""
    ref, _ = reference

    class Sink:
        def __init__(self, n_paths, H, S):
            self.N, self.H, self.buf = n_paths, H, [0] * S
            self.ep = [None] * S
            self.obs, self.act, self.rew, self.len = {}, {}, {}, {}

        def begin(self, slot, ep):
            assert self.ep[slot] is None
            self.ep[slot] = ep

        def rows(self, slots, obs, t):
            for s, o, k in zip(slots, obs, t):
                self.obs[(self.ep[s], int(k))] = o.copy()

        def actions(self, slots, act, t):
            for s, a, k in zip(slots, act, t):
                self.act[(self.ep[s], int(k))] = a.copy()

        def reward(self, slot, t, r):
            self.rew[(self.ep[slot], int(t))] = r

        def finish(self, slot, length, terminated=False):
            self.len[self.ep[slot]] = (length, terminated)
            self.ep[slot] = None

    from mjrl_amd.samplers import env_workers
    sinks = []

    def make(*a):
        sinks.append(Sink(*a))
        return sinks[-1]
    pool = env_workers.get_env_pool(StubEnv, 3, NUM_ENVS, policy.n, policy.m, 60.0)
    got = env_workers.sample_paths(pool, N, _cpu_means(policy), policy.log_std_val, 1e6, SEED, sink=make)
    _same_paths(got, ref)
    s = sinks[0]
    assert len(s.obs) == len(s.act) == len(s.rew) == sum(len(p["rewards"]) for p in ref)
    for ep, p in enumerate(ref):
        assert s.len[ep] == (len(p["rewards"]), bool(p["terminated"]))
        for k in range(len(p["rewards"])):
            assert np.array_equal(s.obs[(ep, k)], p["observations"][k])
            assert np.array_equal(s.act[(ep, k)], p["actions"][k]) and s.rew[(ep, k)] == p["rewards"][k]


def test_failing_environment_tears_the_pool_down(policy):
    from mjrl_amd.samplers import env_workers
    env = functools.partial(FailingEnv, SEED + 11)
    pool = env_workers.get_env_pool(env, 3, NUM_ENVS, policy.n, policy.m, 20.0)
    procs, name = list(pool._procs), pool.shm_name
    t0 = time.time()
    with pytest.raises(RuntimeError, match=r"env worker \d+ failed in step \(slot \d+, trajectory 11\)") as e:
        env_workers.sample_paths(pool, N, _cpu_means(policy), policy.log_std_val, 1e6, SEED)
    assert time.time() - t0 < 20.0
    assert "ArithmeticError: stub failure in trajectory seeded %d" % (SEED + 11) in str(e.value)   # remote traceback
    assert "Traceback" in str(e.value)
    assert all(p.poll() is not None for p in procs)
    with pytest.raises(FileNotFoundError):
        shared_memory.SharedMemory(name=name)
    assert pool not in env_workers._POOLS.values()
    # the next call starts a fresh pool for the same key (8 trajectories: the failing one is not reached)
    ref = _single_process(8, policy, env, SEED, NUM_ENVS, _cpu_means(policy))
    fresh = env_workers.get_env_pool(env, 3, NUM_ENVS, policy.n, policy.m, 20.0)
    assert fresh is not pool and fresh.alive()
    _same_paths(env_workers.sample_paths(fresh, 8, _cpu_means(policy), policy.log_std_val, 1e6, SEED), ref)


def test_dead_worker_is_reported(policy):
    from mjrl_amd.samplers import env_workers
    pool = env_workers.get_env_pool(StubEnv, 2, NUM_ENVS, policy.n, policy.m, 20.0)
    procs, name = list(pool._procs), pool.shm_name
    procs[1].kill()
    procs[1].wait()
    with pytest.raises(RuntimeError, match="env worker 1"):
        env_workers.sample_paths(pool, N, _cpu_means(policy), policy.log_std_val, 1e6, SEED)
    assert all(p.poll() is not None for p in procs)
    with pytest.raises(FileNotFoundError):
        shared_memory.SharedMemory(name=name)


def test_workers_do_not_import_torch(policy):
    pool, _ = _run(policy, 8, 2)
    assert [h["torch"] for h in pool.hello] == [False, False]
    assert [h["slots"] for h in pool.hello] == [(0, 4), (4, 8)]
    assert pool.horizon == 40


def test_lambda_factory_is_refused_before_any_process_starts(policy, monkeypatch):
    from mjrl_amd.samplers import env_workers
    env_workers.close_env_pools()
    started = []
    real = subprocess.Popen
    monkeypatch.setattr(subprocess, "Popen", lambda *a, **k: started.append(a) or real(*a, **k))
    with pytest.raises(ValueError, match="does not pickle"):
        env_workers.get_env_pool(lambda: StubEnv(), 2, NUM_ENVS, policy.n, policy.m)
    with pytest.raises(ValueError, match="does not pickle"):
        env_workers.EnvWorkerPool(lambda: StubEnv(), 2, NUM_ENVS, policy.n, policy.m)
    assert not started and not env_workers._POOLS


def test_policy_mean_slots_validates_before_any_launch():
    """The EINVAL cases of mjrl_policy_mean_slots and E == 0 return before a
    launch: no GPU needed."""
    import ctypes as C
    import os
    from mjrl_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    s = C.byref(_lib.make_shape(8, 2, 64, 64))
    p = C.c_void_p(64)
    f = lib.mjrl_policy_mean_slots
    ok = (s, p, p, 3, 8, p, None, None, None, None, p, None)

    def call(**kw):
        names = ("s", "obs", "live", "E", "S", "theta", "ish", "isc", "osh", "osc", "mean", "stream")
        return f(*[kw.get(k, v) for k, v in zip(names, ok)])
    for bad in (dict(s=None), dict(theta=None), dict(mean=None), dict(E=-1), dict(E=9), dict(S=-1, E=0),
                dict(obs=None), dict(live=None), dict(ish=p), dict(isc=p), dict(osh=p), dict(osc=p)):
        assert call(**bad) == _lib.MJRL_EINVAL, bad
    assert call(E=0) == _lib.MJRL_OK
    assert call(E=0, obs=None, live=None) == _lib.MJRL_OK
