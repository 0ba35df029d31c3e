"""sample_mode="samples" on the vector sampler, without a GPU: the scheduler
(samplers/samples_schedule.py) alone on scripted length sequences, and the
environment-worker route with a row-wise CPU mean provider against the reference's
one-core loop (batch_sampler.py:58-103): serial_rollout(1, ..., seed + k) for
k = 0, 1, ... until the lengths sum to >= N.  Paths bitwise, numpy's global RNG
left as the last accepted trajectory left it, whatever the worker count."""
import numpy as np
import pytest

from stub_env import StubEnv, serial_rollout
from test_env_workers import _cpu_means, _policy, _rng_equal

SEED, NUM_ENVS = 7, 8


# ---- the scheduler alone ---------------------------------------------------------
def _lockstep(lengths, N, S):
    """Drives SamplesSchedule as a lock-stepped sampler with S slots would, with
    trajectory k ending after lengths[k] rows.  Returns the schedule and a log of
    (event, trajectory, rows started so far)."""
    from mjrl_amd.samplers.samples_schedule import SamplesSchedule
    sched = SamplesSchedule(N)
    live, log = [None] * S, []

    def fill():
        for s in range(S):
            if live[s] is None and sched.may_start():
                live[s] = sched.start()
                log.append(("start", live[s], sched.rows))

    fill()
    steps = 0
    while not sched.done:
        assert any(k is not None for k in live), "stalled before the prefix closed"
        ended = []
        for s in range(S):
            k = live[s]
            if k is None:
                continue
            sched.step(k)
            if sched.length[k] == lengths[k]:
                ended.append(s)
        for s in ended:
            sched.end(live[s])
            log.append(("end", live[s], sched.rows))
            live[s] = None
            # done exactly from the end() call that closes the prefix 0..K
            over = {k for e, k, _ in log if e == "end"}
            assert sched.done == all(k in over for k in range(_expected_K(lengths, N) + 1))
        steps += 1
        if not sched.done:
            fill()
    return sched, log, [k for k in live if k is not None], steps


def _expected_K(lengths, N):
    return int(np.searchsorted(np.cumsum(lengths), N))   # the first k with prefix sum >= N


@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("lengths,N", [
    ([5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5], 12),          # equal lengths
    ([40, 1, 1, 1, 40, 2, 40, 40, 3, 40, 40, 40], 45),   # short ones end first; a long one closes the prefix
    ([1, 40, 1, 40, 1, 40, 1, 40, 1, 40, 1, 40], 1),     # one row is enough
    ([3, 9, 4, 7, 40, 2, 6, 40, 40, 5, 8, 40], 23),      # N equal to a prefix sum (3 + 9 + 4 + 7)
    ([3, 9, 4, 7, 40, 2, 6, 40, 40, 5, 8, 40], 24),      # ... and one more
    ([7] * 60, 300),                                       # more trajectories than slots
])
def test_scheduler_accepts_the_minimal_prefix(lengths, N, S):
    lengths = list(lengths) + [40] * 16   # what may start beyond the scripted ones
    sched, log, live, steps = _lockstep(lengths, N, S)
    K = _expected_K(lengths, N)
    assert sched.K == K and sched.accepted == K + 1
    assert sum(lengths[:K + 1]) >= N > sum(lengths[:K])            # minimal
    # trajectories start in index order, none after the started rows reached N
    starts = [e for e in log if e[0] == "start"]
    assert [k for _, k, _ in starts] == list(range(len(starts)))
    assert all(rows < N for _, _, rows in starts)
    assert len(starts) > K
    ended = {k for e, k, _ in log if e == "end"}
    assert set(range(K + 1)) <= ended
    last_needed = max(i for i, (e, k, _) in enumerate(log) if e == "end" and k <= K)
    assert all(e == "end" for e, _, _ in log[last_needed:])        # nothing started after it
    # abandoned: exactly the started trajectories that are still live, all above K
    assert sorted(sched.abandoned()) == sorted(live)
    assert all(k > K for k in live)
    assert set(range(len(starts))) == ended | set(live)


def test_scheduler_stops_as_soon_as_the_prefix_closes():
    """Slots 3: trajectories 0 (4 rows), 1 (2), 2 (9).  N = 5: 0 and 1 make 6 rows;
    the prefix closes when 0 ends in lock step 4, while 2 is live at 4 rows."""
    sched, log, live, steps = _lockstep([4, 2, 9, 9, 9], 5, 3)
    assert sched.K == 1 and steps == 4
    # when 1 ended, 2 + 2 + 2 = 6 >= 5 rows were started: trajectory 3 never starts
    assert [k for e, k, _ in log if e == "start"] == [0, 1, 2]
    assert sorted(live) == [2] and sched.abandoned() == [2]
    assert sched.length[2] == 4


def test_scheduler_nothing_starts_once_the_rows_are_there():
    """Two slots, N = 10: after trajectory 0 (3 rows) ends with trajectory 1 at 3 rows,
    6 < 10 rows are started and trajectory 2 starts; when 1 ends at 6 rows, 3 + 6 + 3
    = 12 >= 10 rows are started and the slot stays idle."""
    sched, log, live, _ = _lockstep([3, 6, 30, 30], 10, 2)
    assert [k for e, k, _ in log if e == "start"] == [0, 1, 2]
    assert sched.K == 2 and live == []


def test_scheduler_zero_and_negative_N():
    from mjrl_amd.samplers.samples_schedule import SamplesSchedule
    for N in (0, -3):
        s = SamplesSchedule(N)
        assert s.done and not s.may_start() and s.accepted == 0 and s.abandoned() == []
        with pytest.raises(RuntimeError):
            s.start()


# ---- the worker route ----------------------------------------------------------------
@pytest.fixture(scope="module")
def policy():
    return _policy()


@pytest.fixture(scope="module", autouse=True)
def _close_pools():
    yield
    from mjrl_amd.samplers import env_workers
    env_workers.close_env_pools()


@pytest.fixture(scope="module")
def serial(policy):
    """The reference's trajectories seeded SEED + k for k < 40, one call each as the
    one-core loop makes them, with numpy's state after each (computed once)."""
    saved = np.random.get_state()
    out = []
    for k in range(40):
        p = serial_rollout(1, policy, 1e6, StubEnv, SEED + k)[0]
        out.append((p, np.random.get_state()))
    np.random.set_state(saved)
    return out


def _reference(serial, N):
    paths, total = [], 0
    while total < N:
        paths.append(serial[len(paths)])
        total += len(paths[-1][0]["rewards"])
    return [p for p, _ in paths], (paths[-1][1] if paths else None)


def _same_as_serial(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        for k in ("observations", "actions", "rewards"):
            assert g[k].dtype == r[k].dtype and g[k].shape == r[k].shape, k
            assert g[k].tobytes() == r[k].tobytes(), k
        assert g["agent_infos"]["mean"].tobytes() == r["mean"].tobytes()
        assert g["env_infos"]["norm"].tobytes() == r["norm"].tobytes()
        assert bool(g["terminated"]) == bool(r["terminated"])


class Recorder:
    """A sink that records the protocol: which trajectories began, finished and
    were abandoned, and how many rows of each it was handed."""

    def __init__(self, N, H, S):
        self.N, self.H, self.buf = N, H, [0] * S
        self.ep = [None] * S
        self.began, self.finished, self.abandoned, self.nrows = [], {}, [], {}

    def begin(self, slot, ep):
        assert self.ep[slot] is None
        self.ep[slot] = ep
        self.began.append(ep)
        self.nrows[ep] = 0

    def rows(self, slots, obs, t):
        for s, k in zip(slots, t):
            assert self.nrows[self.ep[s]] == k
            self.nrows[self.ep[s]] += 1

    def actions(self, slots, act, t):
        pass

    def reward(self, slot, t, r):
        pass

    def finish(self, slot, length, terminated=False):
        self.finished[self.ep[slot]] = length
        self.ep[slot] = None

    def abandon(self, slot):
        assert self.ep[slot] is not None
        self.abandoned.append(self.ep[slot])
        self.ep[slot] = None


def _run(policy, N, workers, sink=None, **kw):
    from mjrl_amd.samplers import env_workers
    pool = env_workers.get_env_pool(StubEnv, workers, min(NUM_ENVS, max(N, 1)), policy.n, policy.m, 60.0)
    return env_workers.sample_paths(pool, N, _cpu_means(policy), policy.log_std_val, 1e6, SEED, sink=sink, **kw)


def _cases(serial):
    lengths = [len(p["rewards"]) for p, _ in serial]
    pre = int(np.cumsum(lengths)[3])   # a prefix sum of the reference lengths
    return lengths, [(1, 1), (pre, 4), (pre + 1, 5), (300, None)]


@pytest.mark.parametrize("workers", [1, 3])
def test_samples_mode_paths_are_the_serial_reference(policy, serial, workers):
    lengths, cases = _cases(serial)
    assert len(set(lengths)) > 1   # ragged
    for N, count in cases:
        ref, rng = _reference(serial, N)
        if count is not None:
            assert len(ref) == count
        sinks = []

        def make(*a):
            sinks.append(Recorder(*a))
            return sinks[-1]
        np.random.seed(99)
        got = _run(policy, N, workers, sink=make, sample_mode="samples")
        _same_as_serial(got, ref)
        assert sum(len(p["rewards"]) for p in got) >= N > sum(len(p["rewards"]) for p in got[:-1])
        assert _rng_equal(np.random.get_state(), rng)
        s = sinks[0]
        K = len(ref) - 1
        assert s.began == list(range(len(s.began))) and all(s.finished[k] == lengths[k] for k in range(K + 1))
        assert sorted(s.abandoned) == sorted(set(s.began) - set(s.finished)) and all(k > K for k in s.abandoned)
        assert all(e is None for e in s.ep)
        if N == 300:
            # the case the sink tests rest on: more paths than slots, and rows of
            # trajectories that are not part of the batch reached the sink
            assert len(ref) > NUM_ENVS
            assert len(s.abandoned) >= 1 and any(s.nrows[k] > 0 for k in s.abandoned)


def test_samples_mode_zero_timesteps(policy):
    before = np.random.get_state()
    assert _run(policy, 0, 3, sample_mode="samples") == []
    assert _rng_equal(np.random.get_state(), before)


def test_samples_mode_without_a_seed_starts_at_zero(policy):
    """pegasus_seed=None: the one-core loop seeds trajectory k with k (batch_sampler.py:87)."""
    from mjrl_amd.samplers import env_workers
    ref = [serial_rollout(1, policy, 1e6, StubEnv, k)[0] for k in range(2)]
    N = len(ref[0]["rewards"]) + 1
    pool = env_workers.get_env_pool(StubEnv, 3, min(NUM_ENVS, N), policy.n, policy.m, 60.0)
    got = env_workers.sample_paths(pool, N, _cpu_means(policy), policy.log_std_val, 1e6, None, sample_mode="samples")
    _same_as_serial(got, ref)


def test_trajectories_mode_is_unchanged(policy, serial):
    """The default and sample_mode="trajectories" return the N trajectories they
    return today (bitwise the serial ones), and an unknown mode is refused."""
    ref = [p for p, _ in serial[:11]]
    np.random.seed(5)
    a = _run(policy, 11, 3)
    rng = np.random.get_state()
    np.random.seed(5)
    b = _run(policy, 11, 3, sample_mode="trajectories")
    assert _rng_equal(np.random.get_state(), rng) and _rng_equal(rng, serial[10][1])
    _same_as_serial(a, ref)
    _same_as_serial(b, ref)
    with pytest.raises(ValueError, match="sample_mode"):
        _run(policy, 11, 3, sample_mode="steps")


# ---- the per-slot ranges of the sink's native row call -----------------------------------
@pytest.mark.parametrize("n", [6, 19])
def test_rows_slots_call_equals_the_one_table_call_per_slot(n):
    """mjrl_host_stage_rows_slots_f64x: the f32 rows and predictions of
    mjrl_host_stage_rows_f64x, and for every slot the range and flag the one-table
    call gives on that slot's rows alone (NaNs skipped, a flag only where a value is
    not a float32)."""
    import ctypes as C
    from mjrl_amd import _lib
    S = _lib.stage_calls()
    rs = np.random.RandomState(n)
    E, nslots = 23, 5
    src = rs.randn(E, n) * 4
    slot = rs.randint(0, nslots, E).astype(np.int64)
    exact = int(slot[0])                                      # this slot's values are float32s
    src[slot == exact] = src[slot == exact].astype(np.float32)
    src[3, 1], src[7, 0] = np.nan, 1e300
    coeffs, t = rs.randn(n + 4), rs.randint(0, 40, E).astype(np.int64)
    out = np.zeros((E, n), np.float32)
    ptrs = (C.c_void_p * E)(*[out.ctypes.data + 4 * n * i for i in range(E)])
    lo, hi = np.full((nslots, n), np.inf, np.float32), np.full((nslots, n), -np.inf, np.float32)
    flag, pred = np.zeros(nslots, np.int32), np.zeros(E)
    S.mjrl_host_stage_rows_slots_f64x(src, E, n, ptrs, slot, nslots, lo, hi, coeffs, t, pred, flag)
    for s in range(nslots):
        rows = np.nonzero(slot == s)[0]
        o1 = np.zeros((len(rows), n), np.float32)
        p1 = (C.c_void_p * len(rows))(*[o1.ctypes.data + 4 * n * i for i in range(len(rows))])
        l1, h1 = np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)
        f1, pr1 = np.zeros(1, np.int32), np.zeros(len(rows))
        S.mjrl_host_stage_rows_f64x(np.ascontiguousarray(src[rows]), len(rows), n, p1, l1, h1, coeffs,
                                    np.ascontiguousarray(t[rows]), pr1, f1)
        assert out[rows].tobytes() == o1.tobytes() and pred[rows].tobytes() == pr1.tobytes()
        assert lo[s].tobytes() == l1.tobytes() and hi[s].tobytes() == h1.tobytes() and flag[s] == f1[0]
    assert flag[exact] == (1 if np.isnan(src[slot == exact]).any() or np.isinf(out[slot == exact]).any() else 0)
    assert flag.sum() >= 1
    with pytest.raises(_lib.MjrlError, match="mjrl_host_stage_rows_slots_f64x"):
        S.mjrl_host_stage_rows_slots_f64x(src, E, n, ptrs, slot, int(slot.max()), lo, hi, coeffs, t, pred, flag)
    with pytest.raises(_lib.MjrlError, match="mjrl_host_stage_rows_slots_f64x"):
        S.mjrl_host_stage_rows_slots_f64x(src, E, n, ptrs, slot, nslots, None, hi, coeffs, t, pred, flag)
