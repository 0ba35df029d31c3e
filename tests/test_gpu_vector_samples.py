"""sample_mode="samples" on the vector sampler, on the device: the two run-table
kernels (mjrl_copy_runs, mjrl_value_features_finish_runs) bit for bit against torch
indexing and against the indexed kernels they stand next to, ChunkSink.batch against
DeviceBatch.from_paths on the same paths (in process and with environment workers,
with rows of abandoned trajectories in the sink), the overflow fall-back, and
train_step with the sink on and off."""
import numpy as np
import pytest
import torch

from test_gpu_stream_staging import _same_batch

pytestmark = pytest.mark.gpu
CANARY = 0x5EADBEEF


@pytest.fixture(scope="module", autouse=True)
def _close_pools():
    yield
    from mjrl_amd.samplers import env_workers
    env_workers.close_env_pools()


def _dev():
    return torch.device("cuda:0")


def _K():
    from mjrl_amd import _lib
    return _lib.calls(), _lib.stream_ptr


# ---- mjrl_copy_runs --------------------------------------------------------------------
def _run_table(rs, src_rows, dst_rows, first=(1, 3, 7, 40)):
    """Runs that do not overlap in dst: the given lengths first, each at an odd
    dst_row, then random ones with random gaps, from random places of src."""
    runs, d = [], 1
    lengths = list(first)
    while True:
        L = lengths.pop(0) if lengths else int(rs.randint(1, 24))
        if d % 2 == 0 and len(runs) < len(first):
            d += 1
        if d + L > dst_rows:
            break
        runs.append((int(rs.randint(0, src_rows - L + 1)), d, L, int(rs.randint(0, 5))))
        d += L + int(rs.randint(0, 3))
    return np.array(runs, np.int64).reshape(-1, 4)


def _apply(runs, src, dst, src_rows, dst_rows):
    """torch indexing: the valid runs of the table applied to dst."""
    for s, d, L, _ in runs.tolist():
        if L > 0 and s >= 0 and d >= 0 and s + L <= src_rows and d + L <= dst_rows:
            dst[d:d + L] = src[s:s + L]
    return dst


@pytest.mark.parametrize("row_bytes", [20, 24, 32, 8])
def test_copy_runs_equals_torch_indexing(row_bytes):
    K, st = _K()
    dev, w = _dev(), row_bytes // 4
    rs = np.random.RandomState(row_bytes)
    src_rows, dst_rows = 173, 211
    src = torch.from_numpy(rs.randint(-2 ** 31, 2 ** 31, (src_rows, w)).astype(np.int32)).to(dev)
    runs = _run_table(rs, src_rows, dst_rows)
    assert [r[2] for r in runs[:4].tolist()] == [1, 3, 7, 40] and all(r[1] % 2 == 1 for r in runs[:4].tolist())
    assert len(runs) > 8
    with torch.cuda.device(dev):
        buf = torch.full((dst_rows + 2, w), CANARY, dtype=torch.int32, device=dev)   # a canary row each side
        want = _apply(runs, src, torch.full((dst_rows, w), CANARY, dtype=torch.int32, device=dev), src_rows, dst_rows)
        K.mjrl_copy_runs(src, row_bytes, torch.from_numpy(runs).to(dev), len(runs), src_rows, dst_rows, buf[1:], st())
        torch.cuda.synchronize()
    assert torch.equal(buf[1:-1], want)
    assert bool((buf[[0, -1]] == CANARY).all())
    assert bool((want != CANARY).any())


def test_copy_runs_every_width_in_one_table():
    """24-byte rows: a run at even rows with an even length moves as 16-byte words,
    one at an odd row as 8-byte words; 20-byte rows: 4-byte words unless rows and
    length are multiples of 4.  One table holds all of them."""
    K, st = _K()
    dev = _dev()
    for row_bytes in (24, 20):
        w = row_bytes // 4
        src = torch.arange(64 * w, dtype=torch.int32, device=dev).view(64, w)
        runs = np.array([[0, 0, 4, 0], [5, 5, 3, 0], [8, 8, 8, 0], [17, 16, 5, 0], [32, 24, 16, 0]], np.int64)
        with torch.cuda.device(dev):
            dst = torch.full((48, w), CANARY, dtype=torch.int32, device=dev)
            want = _apply(runs, src, dst.clone(), 64, 48)
            K.mjrl_copy_runs(src, row_bytes, torch.from_numpy(runs).to(dev), len(runs), 64, 48, dst, st())
            torch.cuda.synchronize()
        assert torch.equal(dst, want)


def test_copy_runs_skips_runs_out_of_range():
    K, st = _K()
    dev, w, src_rows, dst_rows = _dev(), 6, 50, 60
    big = 2 ** 62
    runs = np.array([[0, 0, 5, 0],                 # valid
                     [48, 10, 3, 0],               # leaves src at the end
                     [-1, 10, 3, 0],               # starts before src
                     [0, 58, 3, 0],                # leaves dst at the end
                     [0, -2, 3, 0],                # starts before dst
                     [0, 20, 0, 0], [0, 20, -4, 0],   # empty, negative
                     [big, 20, 3, 0], [0, big, 3, 0], [0, 20, big, 0], [big, big, big, 0],   # no wrap-around
                     [45, 55, 5, 0]],              # valid, the last rows of both
                    np.int64)
    src = torch.arange(src_rows * w, dtype=torch.int32, device=dev).view(src_rows, w)
    with torch.cuda.device(dev):
        buf = torch.full((dst_rows + 2, w), CANARY, dtype=torch.int32, device=dev)
        want = torch.full((dst_rows, w), CANARY, dtype=torch.int32, device=dev)
        want[0:5], want[55:60] = src[0:5], src[45:50]
        K.mjrl_copy_runs(src, 4 * w, torch.from_numpy(runs).to(dev), len(runs), src_rows, dst_rows, buf[1:], st())
        torch.cuda.synchronize()
    assert torch.equal(buf[1:-1], want)
    assert bool((buf[[0, -1]] == CANARY).all())


def test_copy_runs_refusals_come_before_any_launch():
    from mjrl_amd import _lib
    K, st = _K()
    dev = _dev()
    src = torch.arange(40, dtype=torch.int32, device=dev).view(10, 4)
    runs = torch.tensor([[0, 0, 10, 0]], dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        dst = torch.full((10, 4), CANARY, dtype=torch.int32, device=dev)
        for args in [(src, 6, runs, 1, 10, 10, dst), (src, 0, runs, 1, 10, 10, dst), (src, -16, runs, 1, 10, 10, dst),
                     (src, 16, runs, -1, 10, 10, dst), (src, 16, runs, 1, -1, 10, dst), (src, 16, runs, 1, 10, -1, dst),
                     (None, 16, runs, 1, 10, 10, dst), (src, 16, None, 1, 10, 10, dst),
                     (src, 16, runs, 1, 10, 10, None)]:
            with pytest.raises(_lib.MjrlError, match=r"^mjrl_copy_runs failed: invalid argument$"):
                K.mjrl_copy_runs(*args, st())
        assert K.mjrl_copy_runs(None, 16, None, 0, 0, 0, None, st()) == _lib.MJRL_OK   # R == 0: nothing to do
        assert K.mjrl_copy_runs(src, 16, runs, 0, 10, 10, dst, st()) == _lib.MJRL_OK
        torch.cuda.synchronize()
    assert bool((dst == CANARY).all())


# ---- mjrl_value_features_finish_runs -----------------------------------------------------
def _mlp(n, seed=0, **kw):
    from mjrl_amd.baselines.mlp_baseline import MLPBaseline
    from mjrl_amd.utils.gym_env import EnvSpec
    torch.manual_seed(seed)
    return MLPBaseline(EnvSpec(n, 2, 40, 1), **kw)


@pytest.mark.parametrize("n", [5, 6, 8])   # rows of 4-, 8- and 16-byte words
def test_finish_runs_equals_finish_on_the_padded_layout(n):
    """The same feature rows laid out padded ([P H][n], row ep H + t) through
    mjrl_value_features_finish with its index, and in a pool of 16-row chunks taken
    in a shuffled order through the run kernel: the same [T][n + 4] bits.  The runs
    are cut inside chunks too, so their t0 lie off and across chunk boundaries."""
    K, st = _K()
    dev, H, CH = _dev(), 40, 16
    rs = np.random.RandomState(n)
    lengths = [1, 40, 17, 40, 3, 39, 16, 2, 25, 32]
    P, T = len(lengths), sum(lengths)
    feat = [rs.randn(L, n).astype(np.float32) for L in lengths]
    pad = np.zeros((P * H, n), np.float32)
    idx = np.concatenate([ep * H + np.arange(L, dtype=np.int64) for ep, L in enumerate(lengths)])
    nchunks = sum(-(-L // CH) for L in lengths)
    order = rs.permutation(nchunks + 3).tolist()   # three chunks stay unused
    pool = np.full(((nchunks + 3) * CH, n), np.nan, np.float32)
    runs, off = [], 0
    for ep, L in enumerate(lengths):
        pad[ep * H:ep * H + L] = feat[ep]
        for j in range(-(-L // CH)):
            c, a, e = order.pop(), j * CH, min(L, (j + 1) * CH)
            pool[c * CH:c * CH + e - a] = feat[ep][a:e]
            cut = a + int(rs.randint(1, e - a)) if e - a > 1 else e   # two runs a chunk: t0 = a and t0 = cut
            for r0, r1 in ((a, cut), (cut, e)):
                if r1 > r0:
                    runs.append((c * CH + r0 - a, off + r0, r1 - r0, r0))
        off += L
    runs = np.array(runs, np.int64)
    assert any(t0 % CH for t0 in runs[:, 3].tolist()) and any(t0 >= CH for t0 in runs[:, 3].tolist())
    mb = _mlp(n)
    with torch.cuda.device(dev):
        tab = mb.time_table(H, dev)
        want = torch.zeros((T, n + 4), dtype=torch.float32, device=dev)
        K.mjrl_value_features_finish(torch.from_numpy(pad).to(dev), torch.from_numpy(idx).to(dev), T, n, P * H, H, tab,
                                     want, st())
        buf = torch.full((T + 2, n + 4), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
        K.mjrl_value_features_finish_runs(torch.from_numpy(pool).to(dev), torch.from_numpy(runs).to(dev), len(runs), n,
                                          len(pool), T, H, tab, buf[1:], st())
        torch.cuda.synchronize()
    assert torch.equal(buf[1:-1].view(torch.int32), want.view(torch.int32))
    assert bool((buf[[0, -1]].view(torch.int32) == CANARY).all())


@pytest.mark.parametrize("n", [5, 8])
def test_finish_runs_skips_runs_past_the_horizon_and_out_of_range(n):
    from mjrl_amd import _lib
    K, st = _K()
    dev, H, T, src_rows = _dev(), 40, 30, 64
    big = 2 ** 62
    runs = np.array([[0, 0, 10, 30],        # t0 + nrows == H: valid
                     [10, 10, 10, 31],      # t0 + nrows > H: skipped
                     [10, 10, 5, -1],       # t0 < 0
                     [60, 10, 5, 0],        # leaves the pool
                     [0, 28, 3, 0],         # leaves out
                     [0, 10, big, 0], [0, 10, 3, big], [big, 10, 3, 0],
                     [20, 20, 10, 0]], np.int64)
    feat = torch.from_numpy(np.random.RandomState(1).randn(src_rows, n).astype(np.float32)).to(dev)
    mb = _mlp(n)
    with torch.cuda.device(dev):
        tab = mb.time_table(H, dev)
        buf = torch.full((T + 2, n + 4), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
        K.mjrl_value_features_finish_runs(feat, torch.from_numpy(runs).to(dev), len(runs), n, src_rows, T, H, tab,
                                          buf[1:], st())
        torch.cuda.synchronize()
        want = torch.full((T, n + 4), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
        want[0:10] = torch.cat([feat[0:10], tab[30:40]], 1)
        want[20:30] = torch.cat([feat[20:30], tab[0:10]], 1)
        assert torch.equal(buf[1:-1].view(torch.int32), want.view(torch.int32))
        assert bool((buf[[0, -1]].view(torch.int32) == CANARY).all())
        d_runs = torch.from_numpy(runs).to(dev)
        out = buf[1:]
        for args in [(feat, d_runs, -1, n, src_rows, T, H, tab, out), (feat, d_runs, 1, 0, src_rows, T, H, tab, out),
                     (feat, d_runs, 1, n, -1, T, H, tab, out), (feat, d_runs, 1, n, src_rows, -1, H, tab, out),
                     (feat, d_runs, 1, n, src_rows, T, 0, tab, out), (None, d_runs, 1, n, src_rows, T, H, tab, out),
                     (feat, None, 1, n, src_rows, T, H, tab, out), (feat, d_runs, 1, n, src_rows, T, H, None, out),
                     (feat, d_runs, 1, n, src_rows, T, H, tab, None)]:
            with pytest.raises(_lib.MjrlError, match=r"^mjrl_value_features_finish_runs failed: invalid argument$"):
                K.mjrl_value_features_finish_runs(*args, st())
        assert K.mjrl_value_features_finish_runs(None, None, 0, n, 0, 0, H, None, None, st()) == _lib.MJRL_OK


# ---- the sink ----------------------------------------------------------------------------
N_SAMPLES, SEED, NUM_ENVS = 300, 7, 8


def _policy():
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    spec = EnvSpec(6, 2, 40, 1)
    return spec, MLP(spec, hidden_sizes=(32, 32), seed=4, init_log_std=-0.5)


def _recording_sink():
    from mjrl_amd.samplers.stream_staging import ChunkSink

    class Rec(ChunkSink):
        """ChunkSink that notes, per abandoned trajectory, how many chunks it held."""

        def abandon(self, slot):
            self.__dict__.setdefault("dropped", []).append(len(self.slot_chunks[slot]))
            ChunkSink.abandon(self, slot)
    return Rec


def _sample(base, workers, sinks=None, N=N_SAMPLES, **kw):
    from mjrl_amd.samplers.vector_sampler import sample_paths_vectorized
    from stub_env import StubEnv
    _, policy = _policy()
    Rec = _recording_sink()

    def make(n_steps, H, S):
        sinks.append(Rec(6, 2, H, n_steps, _dev(), baseline=base, nslots=S, **kw))
        return sinks[-1]
    return sample_paths_vectorized(N, policy, 1e6, env=StubEnv, pegasus_seed=SEED, num_envs=NUM_ENVS,
                                   sink=None if sinks is None else make, num_workers=workers, worker_timeout=60.0,
                                   sample_mode="samples")


def _check_prefix(paths, N):
    lengths = [len(p["rewards"]) for p in paths]
    assert sum(lengths) >= N > sum(lengths[:-1])   # the shortest prefix with >= N rows
    assert len(set(lengths)) > 1 and len(paths) > NUM_ENVS   # ragged, more paths than slots
    return lengths


@pytest.mark.parametrize("workers", [0, 2])
@pytest.mark.parametrize("flush", [256, 7])
@pytest.mark.parametrize("fitted", [False, True])
def test_chunk_sink_batch_equals_from_paths(fitted, flush, workers, monkeypatch):
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.engine import DeviceBatch
    from mjrl_amd.samplers.stream_staging import StreamSink
    monkeypatch.setattr(StreamSink, "FLUSH_ROWS", flush)   # 7: chunks of 7 rows, several a trajectory
    dev = _dev()
    spec, _ = _policy()
    base = LinearBaseline(spec)
    if fitted:
        base._coeffs = np.random.RandomState(1).randn(6 + 4)
    plain = _sample(base, workers)
    sinks = []
    paths = _sample(base, workers, sinks)
    _check_prefix(paths, N_SAMPLES)
    assert len(paths) == len(plain)
    for p, q in zip(paths, plain):
        assert np.array_equal(p["observations"], q["observations"]) and np.array_equal(p["actions"], q["actions"])
        assert np.array_equal(p["rewards"], q["rewards"]) and p["terminated"] == q["terminated"]
    sink = sinks[0]
    assert sink.CH == min(flush, 40)
    # rows of trajectories that are not part of the batch reached the sink
    assert any(c > 0 for c in sink.__dict__.get("dropped", []))
    assert not sink.overflowed   # the default budget
    ref = DeviceBatch.from_paths(paths, dev, baseline=base, reuse=False)
    got = sink.batch(paths, reuse=False)
    torch.cuda.synchronize()
    _same_batch(got, ref)
    assert got.obs_inexact   # the stub's observations are f64
    with pytest.raises(ValueError, match="prefix"):
        sink.batch(paths[:-1], reuse=False)


@pytest.mark.parametrize("workers", [0, 2])
def test_chunk_sink_value_features_equal_the_route_without_a_sink(workers, monkeypatch):
    from mjrl_amd.engine import DeviceBatch
    from mjrl_amd.samplers.stream_staging import StreamSink
    from test_gpu_value_features import _fitted_mlp
    monkeypatch.setattr(StreamSink, "FLUSH_ROWS", 7)
    dev = _dev()
    mb = _fitted_mlp(3)
    sinks = []
    paths = _sample(mb, workers, sinks, value_features=True)
    _check_prefix(paths, N_SAMPLES)
    sink = sinks[0]
    assert (sink._board is not None) == (workers > 0)
    assert any(c > 0 for c in sink.__dict__.get("dropped", [])) and not sink.overflowed
    got = sink.batch(paths, reuse=False)
    f32 = DeviceBatch.from_paths(paths, dev, baseline=None, reuse=False)
    for k in ("obs", "act", "rewards", "path_off", "terminated", "obs_range"):
        x, y = getattr(got, k), getattr(f32, k)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), k
    assert got.obs_inexact == f32.obs_inexact is True and np.array_equal(got.lengths, f32.lengths)
    f64 = DeviceBatch.from_paths(paths, dev, baseline=mb, obs_dtype=np.float64, reuse=False)
    want = mb.features_device(f64.obs, f64.path_off, f64.lengths)
    assert got.value_feat.dtype == torch.float32 and got.value_feat.shape == want.shape
    assert torch.equal(got.value_feat.view(torch.int32), want.view(torch.int32))
    assert got.baseline.dtype == torch.float64 and torch.equal(got.baseline, f64.baseline)


def test_chunk_sink_overflow_sets_the_flag_and_batch_refuses(monkeypatch):
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.samplers.stream_staging import StreamSink
    monkeypatch.setattr(StreamSink, "FLUSH_ROWS", 7)
    spec, _ = _policy()
    sinks = []
    paths = _sample(LinearBaseline(spec), 0, sinks, rows_cap=14)   # two chunks
    plain = _sample(LinearBaseline(spec), 0)
    sink = sinks[0]
    assert sink.C == 2 and sink.overflowed
    assert len(paths) == len(plain) and all(np.array_equal(p["observations"], q["observations"])
                                            for p, q in zip(paths, plain))
    with pytest.raises(RuntimeError, match="overflowed"):
        sink.batch(paths, reuse=False)


# ---- train_step ----------------------------------------------------------------------------
def _train(stream, monkeypatch, rows_cap=None, workers=0, iters=2):
    from mjrl_amd.algos.npg_cg import NPG
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.samplers import stream_staging
    from mjrl_amd.utils.gym_env import EnvSpec
    from stub_env import StubEnv
    made = []
    Real = getattr(stream_staging.ChunkSink, "_real", stream_staging.ChunkSink)   # not an earlier call's Spy

    class Spy(Real):
        _real = Real
        ROWS_CAP = rows_cap

        def __init__(self, *a, **kw):
            Real.__init__(self, *a, **kw)
            made.append(self)
    monkeypatch.setattr(stream_staging, "ChunkSink", Spy)

    class Env:
        env_id = "stub-v0"
    spec = EnvSpec(6, 2, 40, 1)
    agent = NPG(Env(), MLP(spec, hidden_sizes=(64, 64), seed=3, init_log_std=-1.0), LinearBaseline(spec),
                normalized_step_size=0.05, seed=200, save_logs=True)
    agent.sampler, agent.env_factory, agent.num_envs, agent.stream_staging = "vector", StubEnv, 16, stream
    agent.sampler_workers = workers
    stats = [agent.train_step(N=600, sample_mode="samples", gamma=0.99, gae_lambda=0.95) for _ in range(iters)]
    assert agent.seed == 200 + 600 * iters   # the seed advances by N, as in the reference
    return (stats, agent.policy.get_param_values(), agent.baseline._coeffs.copy()), made


def test_train_step_samples_mode_stream_on_equals_off(monkeypatch):
    """Two iterations of train_step(N=600, sample_mode="samples") with the vector
    sampler, the sink on and off: identical statistics, parameters and baseline
    coefficients (the second iteration stages predictions of the fitted baseline)."""
    (s1, th1, c1), made = _train(True, monkeypatch)
    assert len(made) == 2 and all(s.done and not s.overflowed for s in made)   # the batches came from the sinks
    (s0, th0, c0), none = _train(False, monkeypatch)
    assert none == []
    assert s1 == s0 and s1[0][-1] == 600
    assert np.array_equal(th1, th0) and np.array_equal(c1, c0)


def test_train_step_with_an_overflowed_sink_stages_from_the_paths(monkeypatch):
    (s1, th1, c1), made = _train(True, monkeypatch, rows_cap=80)   # two chunks of 40 rows
    assert len(made) == 2 and all(s.C == 2 and s.overflowed and not s.done for s in made)
    (s0, th0, c0), _ = _train(False, monkeypatch)
    assert s1 == s0
    assert np.array_equal(th1, th0) and np.array_equal(c1, c0)
