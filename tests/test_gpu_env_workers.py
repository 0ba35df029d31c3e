"""The vector sampler with environment worker processes, on the GPU:
mjrl_policy_mean_slots (the batched forward reading the workers' f64 observation
board) is bitwise mjrl_policy_mean of the f32-rounded rows; sampling with
num_workers >= 1 returns bitwise the paths of num_workers = 0, feeds the
StreamSink to the same device batch, and leaves train_step's update unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = 70   # environment slots of the kernel test's boards


@pytest.fixture(scope="module", autouse=True)
def _close_pools():
    yield
    from mjrl_amd.samplers import env_workers
    env_workers.close_env_pools()


def _make_policy(kind):
    from mjrl_amd.policies.gaussian_linear import LinearPolicy
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    if kind == "linear":
        pol = LinearPolicy(EnvSpec(6, 2, 10, 1), seed=3)
    else:
        n, m, h = kind
        pol = MLP(EnvSpec(n, m, 10, 1), hidden_sizes=(h, h), seed=1)
    rs = np.random.RandomState(5)
    th = pol.get_param_values()
    pol.set_param_values(th + 0.1 * rs.randn(th.size).astype(np.float32))
    return pol


@pytest.mark.parametrize("transform", [False, True])
@pytest.mark.parametrize("kind", ["linear", (8, 2, 64), (376, 17, 64), (17, 6, 128)])
def test_policy_mean_slots_is_bitwise_policy_mean(kind, transform):
    from mjrl_amd import _lib
    from mjrl_amd.samplers.vector_sampler import BatchedPolicy
    pol = _make_policy(kind)
    n, m = pol.n, pol.m
    rs = np.random.RandomState(11)
    if transform:
        pol.model.set_transformations(rs.randn(n) * 0.1, rs.rand(n) + 0.5, rs.randn(m), rs.rand(m) + 0.5)
    dev = torch.device("cuda:0")
    bp = BatchedPolicy(pol, dev)
    eng = bp.eng
    ins, isc, osh, osc = eng.transforms
    assert (ins is not None) == transform
    obs64 = rs.randn(S, n) * 2
    assert not np.array_equal(obs64, obs64.astype(np.float32))   # not f32-representable
    d_obs = torch.from_numpy(obs64).to(dev)
    with torch.cuda.device(dev):
        for E in (1, 3, 5, 64, 67):
            live = rs.permutation(S)[:E].astype(np.int32)
            d_live = torch.from_numpy(live).to(dev)
            mean = torch.full((S, m), -77.0, dtype=torch.float32, device=dev)
            eng.K.mjrl_policy_mean_slots(eng.shape, d_obs, d_live, E, S, bp.packed, ins, isc, osh, osc, mean,
                                         _lib.stream_ptr())
            rows = torch.from_numpy(obs64[live].astype(np.float32)).to(dev)
            ref = torch.empty((E, m), dtype=torch.float32, device=dev)
            eng.K.mjrl_policy_mean(eng.shape, rows, E, bp.packed, ins, isc, osh, osc, ref, _lib.stream_ptr())
            torch.cuda.synchronize()
            got = mean.cpu().numpy()
            assert got[live].tobytes() == ref.cpu().numpy().tobytes(), E
            rest = np.setdiff1d(np.arange(S), live)
            assert np.all(got[rest] == -77.0), E
            # and the wrapper the sampler calls
            out = bp.means_slots(obs64, live)
            assert out[live].tobytes() == got[live].tobytes(), E


def test_policy_mean_slots_refuses_bad_arguments_without_a_launch():
    from mjrl_amd import _lib
    lib = _lib.lib()
    s = C.byref(_lib.make_shape(8, 2, 64, 64))
    p = C.c_void_p(64)
    names = ("s", "obs", "live", "E", "S", "theta", "ish", "isc", "osh", "osc", "mean", "stream")
    ok = (s, p, p, 3, 8, p, None, None, None, None, p, None)

    def call(**kw):
        return lib.mjrl_policy_mean_slots(*[kw.get(k, v) for k, v in zip(names, ok)])
    for bad in (dict(s=None), dict(theta=None), dict(mean=None), dict(E=-1), dict(E=9), dict(S=-1, E=0),
                dict(obs=None), dict(live=None), dict(ish=p), dict(isc=p), dict(osh=p), dict(osc=p)):
        assert call(**bad) == _lib.MJRL_EINVAL, bad
    assert call(E=0) == _lib.MJRL_OK
    assert call(E=0, obs=None, live=None) == _lib.MJRL_OK
    with pytest.raises(_lib.MjrlError, match=r"^mjrl_policy_mean_slots failed: invalid argument$"):
        _lib.calls().mjrl_policy_mean_slots(_lib.make_shape(8, 2, 64, 64), None, None, 3, 8, p, None, None, None, None,
                                            p, None)


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


def _same_batch(a, b):
    for k in ("obs", "act", "rewards", "baseline", "path_off", "terminated"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert torch.equal(x, y), k
    assert torch.equal(a.obs_range, b.obs_range)
    assert a.obs_inexact == b.obs_inexact and np.array_equal(a.lengths, b.lengths)


def _stub_policy():
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    spec = EnvSpec(6, 2, 40, 1)
    return spec, MLP(spec, hidden_sizes=(32, 32), seed=4, init_log_std=-0.5)


def _stub_env(ragged):
    from stub_env import StubEnv
    return StubEnv if ragged else functools.partial(StubEnv, radius=1e9)


@pytest.mark.parametrize("ragged", [True, False])
def test_worker_paths_equal_in_process_paths(ragged):
    from mjrl_amd.samplers.vector_sampler import sample_paths_vectorized
    _, policy = _stub_policy()
    env = _stub_env(ragged)
    np.random.seed(5)
    plain = sample_paths_vectorized(37, policy, 1e6, env=env, pegasus_seed=7, num_envs=8)
    rng = np.random.get_state()
    np.random.seed(6)
    got = sample_paths_vectorized(37, policy, 1e6, env=env, pegasus_seed=7, num_envs=8, num_workers=3,
                                  worker_timeout=60.0)
    after = np.random.get_state()
    assert np.array_equal(after[1], rng[1]) and after[2:] == rng[2:]
    assert len(got) == len(plain) == 37
    for i, (p, q) in enumerate(zip(got, plain)):
        _same_tree(p, q, "path %d" % i)
    lengths = [len(p["rewards"]) for p in got]
    assert (len(set(lengths)) > 1) == ragged
    if ragged:
        assert any(p["terminated"] for p in got) and any(n == 40 for n in lengths)


@pytest.mark.parametrize("flush", [256, 7])
@pytest.mark.parametrize("ragged", [True, False])
def test_worker_stream_batch_equals_from_paths(ragged, flush, monkeypatch):
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.engine import DeviceBatch
    from mjrl_amd.samplers.stream_staging import StreamSink
    from mjrl_amd.samplers.vector_sampler import sample_paths_vectorized
    monkeypatch.setattr(StreamSink, "FLUSH_ROWS", flush)
    dev = torch.device("cuda:0")
    spec, policy = _stub_policy()
    base = LinearBaseline(spec)
    base._coeffs = np.random.RandomState(1).randn(6 + 4)
    sinks = []

    def make(N, H, nslots):
        sinks.append(StreamSink(6, 2, H, N, dev, baseline=base, nslots=nslots))
        return sinks[-1]
    paths = sample_paths_vectorized(37, policy, 1e6, env=_stub_env(ragged), pegasus_seed=7, num_envs=8, sink=make,
                                    num_workers=3, worker_timeout=60.0)
    ref = DeviceBatch.from_paths(paths, dev, baseline=base, reuse=False)
    got = sinks[0].batch(paths, reuse=False)
    torch.cuda.synchronize()
    _same_batch(got, ref)
    assert got.obs_inexact   # the stub's observations are f64


def test_train_step_with_workers_equals_without():
    """Two iterations of train_step with the vector sampler, sampler_workers 4 and
    0: equal statistics, parameters and baseline coefficients."""
    from mjrl_amd.algos.npg_cg import NPG
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    from stub_env import StubEnv

    class Env:
        env_id = "stub-v0"
    out = []
    for workers in (4, 0):
        spec = EnvSpec(6, 2, 40, 1)
        agent = NPG(Env(), MLP(spec, hidden_sizes=(64, 64), seed=3, init_log_std=-1.0), LinearBaseline(spec),
                    normalized_step_size=0.05, seed=200, save_logs=True)
        agent.sampler, agent.env_factory, agent.num_envs, agent.sampler_workers = "vector", StubEnv, 16, workers
        stats = [agent.train_step(N=60, gamma=0.99, gae_lambda=0.95) for _ in range(2)]
        out.append((stats, agent.policy.get_param_values(), agent.baseline._coeffs.copy()))
    (s1, th1, c1), (s0, th0, c0) = out
    assert s1 == s0
    assert np.array_equal(th1, th0) and np.array_equal(c1, c0)
