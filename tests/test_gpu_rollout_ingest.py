"""Device rollout ingest on the GPU: the segmentation and pack kernels of
csrc/ingest.hip against the NumPy reference (samplers/rollout_ingest.py),
DeviceBatch.from_rollout against DeviceBatch.from_paths on the equivalent host
paths, train_from_rollout against train_from_samples, bit for bit; the baseline
fit and predict from the packed rows within the bars of tests/test_gpu_f64obs.py
(the same device fit and predict on data whose float32 images are exact)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mjrl_amd.samplers import rollout_ingest as RI
from test_rollout_ingest import hand_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _boards(H, E, seed, with_term, with_steps, p=0.2):
    """Random done / terminated boards and step counts (some of them 0)."""
    if (H, E) == (5, 3):
        done, term, steps = hand_case()
        return done, term if with_term else None, steps if with_steps else None
    rs = np.random.RandomState(seed)
    done = (rs.rand(H, E) < p).astype(np.uint8)
    term = (rs.rand(H, E) < 0.5).astype(np.uint8) if with_term else None
    steps = None
    if with_steps:
        steps = rs.randint(0, H + 1, size=E)
        steps[rs.rand(E) < 0.15] = 0
        steps = [int(s) for s in steps]
    return done, term, steps


# ---- 1. the segments kernel ----

@pytest.mark.parametrize("with_steps", [False, True], ids=["full", "steps"])
@pytest.mark.parametrize("with_term", [False, True], ids=["done", "term"])
@pytest.mark.parametrize("H,E", [(1, 1), (5, 3), (7, 64), (3, 65), (2, 257), (33, 1000)])
def test_segments_match_the_reference(H, E, with_term, with_steps):
    from mjrl_amd import _lib
    K = _lib.calls()
    done, term, steps = _boards(H, E, 11 * H + E, with_term, with_steps)
    ref = RI.segment_rollout_reference(done, term, steps)
    P, T = ref["P"], ref["T"]
    nw = C.c_int64()
    K.mjrl_rollout_segments_scratch(E, nw)
    assert nw.value >= 0
    i64 = dict(dtype=torch.int64, device=DEV)
    env_row = torch.full((E + 1,), -7, **i64)
    path_off = torch.full((T + 1,), -7, **i64)
    path_term = torch.full((max(T, 1),), 0xAB, dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -7, **i64)
    scratch = torch.zeros(max(nw.value, 1), **i64)
    # bool boards on the odd seeds: one byte per cell either way
    d_done = _dev(done).bool() if (H + E) % 2 else _dev(done)
    d_term = None if term is None else _dev(term)
    d_steps = None if steps is None else _dev(np.asarray(steps, np.int64))
    K.mjrl_rollout_segments(d_done, d_term, d_steps, H, E, T, env_row, path_off, path_term, counts, scratch,
                            _lib.stream_ptr())
    torch.cuda.synchronize()
    assert counts.tolist() == [P, T]
    assert np.array_equal(env_row.cpu().numpy(), ref["R"])
    off, pt = path_off.cpu().numpy(), path_term.cpu().numpy()
    assert np.array_equal(off[:P + 1], ref["path_off"])
    assert np.array_equal(pt[:P], ref["path_term"])
    assert np.all(off[P + 1:] == -7) and np.all(pt[P:] == 0xAB)   # the sentinel survives past the table


def test_segments_refuse_to_write_past_path_cap():
    """A path_cap below P: the entries up to it are written, nothing at or beyond it."""
    from mjrl_amd import _lib
    K = _lib.calls()
    done, term, steps = hand_case()
    ref = RI.segment_rollout_reference(done, term, steps)
    cap = 2
    i64 = dict(dtype=torch.int64, device=DEV)
    env_row, counts = torch.zeros(4, **i64), torch.zeros(2, **i64)
    path_off = torch.full((ref["T"] + 1,), -7, **i64)
    path_term = torch.full((ref["T"],), 0xAB, dtype=torch.uint8, device=DEV)
    K.mjrl_rollout_segments(_dev(done), _dev(term), _dev(np.asarray(steps, np.int64)), 5, 3, cap, env_row, path_off,
                            path_term, counts, torch.zeros(9, **i64), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert counts.tolist() == [ref["P"], ref["T"]]
    assert path_off.tolist()[:cap] == ref["path_off"].tolist()[:cap] and path_off.tolist()[cap:] == [-7] * 7
    assert path_term.tolist()[:cap] == ref["path_term"].tolist()[:cap] and set(path_term.tolist()[cap:]) == {0xAB}


# ---- 2. the pack kernel ----

PACK_HE = (7, 65)


def _pack_case(dtype, n, m, rdtype, with_steps=True, seed=5):
    H, E = PACK_HE
    rs = np.random.RandomState(seed + 31 * n + m)
    obs = (rs.randn(H, E, n) * 3).astype(dtype)
    act = rs.randn(H, E, m).astype(dtype)
    rew = rs.randn(H, E).astype(rdtype)
    _, _, steps = _boards(H, E, seed, False, with_steps)
    if steps is not None:
        for e, s in enumerate(steps):   # cells past an env's steps must never be read
            obs[s:, e] = np.nan
            act[s:, e] = np.nan
            rew[s:, e] = np.nan
    return obs, act, rew, steps


def _run_pack(obs, act, rew, steps, offset=0):
    """mjrl_rollout_pack on its own (env_row from the reference); `offset`: elements the
    observation output is shifted by, to take the narrower word widths."""
    from mjrl_amd import _lib
    K = _lib.calls()
    H, E, n = obs.shape
    m = act.shape[2]
    s = RI.check_steps(steps, H, E)
    R = np.concatenate([[0], np.cumsum(s)]).astype(np.int64)
    T = int(R[-1])
    tdt = torch.float32 if obs.dtype == np.float32 else torch.float64
    o_buf = torch.full((T * n + offset,), -1.0, dtype=tdt, device=DEV)
    o = o_buf[offset:].view(T, n)
    a = torch.full((T, m), -1.0, dtype=tdt, device=DEV)
    r = torch.full((T,), -1.0, dtype=torch.float64, device=DEV)
    rng = part = None
    if obs.dtype == np.float32:
        nf = C.c_int64()
        K.mjrl_rollout_pack_scratch(T, n, nf)
        rng = torch.zeros((2, n), dtype=torch.float32, device=DEV)
        part = torch.zeros(max(nf.value, 1), dtype=torch.float32, device=DEV)
    K.mjrl_rollout_pack(_dev(obs), _dev(act), _dev(rew), int(obs.dtype == np.float64), int(rew.dtype == np.float64),
                        None if steps is None else _dev(s), _dev(R), H, E, n, m, T, o, a, r, rng, part,
                        _lib.stream_ptr())
    torch.cuda.synchronize()
    return o.cpu().numpy(), a.cpu().numpy(), r.cpu().numpy(), None if rng is None else rng.cpu().numpy()


def _check_pack(obs, act, rew, steps, got):
    o, a, r, rng = got
    want_o, want_a = RI.rollout_rows(obs, steps), RI.rollout_rows(act, steps)
    want_r = RI.rollout_rows(rew, steps).astype(np.float64)
    assert o.tobytes() == want_o.tobytes() and a.tobytes() == want_a.tobytes() and r.tobytes() == want_r.tobytes()
    assert not (np.isnan(o).any() or np.isnan(a).any() or np.isnan(r).any())
    if obs.dtype == np.float32:
        assert rng.tobytes() == np.stack([want_o.min(axis=0), want_o.max(axis=0)]).tobytes()
        assert not np.isnan(rng).any()
    else:
        assert rng is None


@pytest.mark.parametrize("rdtype", [np.float32, np.float64], ids=["rew32", "rew64"])
@pytest.mark.parametrize("m", [1, 6])
@pytest.mark.parametrize("n", [1, 3, 8, 17])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_pack_matches_numpy_gather(dtype, n, m, rdtype):
    obs, act, rew, steps = _pack_case(dtype, n, m, rdtype)
    _check_pack(obs, act, rew, steps, _run_pack(obs, act, rew, steps))


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("n", [8, 72 * 4 + 8])
def test_pack_without_steps_and_on_narrow_words(n, offset):
    """steps None (row r is cell (r % H, r / H), no bisection), an output shifted by
    one or two floats (8- and 4-byte words), and a row wider than 64 sixteen-byte
    words (a second block of the row)."""
    obs, act, rew, steps = _pack_case(np.float32, n, 2, np.float64, with_steps=False)
    _check_pack(obs, act, rew, steps, _run_pack(obs, act, rew, steps, offset))


def test_pack_range_skips_nan_as_the_host_pass_does():
    """The ranges are the host staging pass's (mjrl_host_stage_f32) on the same rows,
    a NaN among the valid cells included: it is skipped, an all-NaN column stays
    (+inf, -inf)."""
    from mjrl_amd import _lib
    obs, act, rew, steps = _pack_case(np.float32, 8, 2, np.float64)
    obs[0, 0, 3] = np.nan if steps[0] > 0 else obs[0, 0, 3]
    obs[:, :, 5] = np.nan
    o, _, _, rng = _run_pack(obs, act, rew, steps)
    rows = RI.rollout_rows(obs, steps)
    assert o.tobytes() == rows.tobytes()
    dst = np.zeros_like(rows)
    lo, hi = np.full(8, np.inf, np.float32), np.full(8, -np.inf, np.float32)
    _lib.stage_calls().mjrl_host_stage_f32(rows, rows.shape[0], 8, dst, lo, hi)
    assert rng.tobytes() == np.stack([lo, hi]).tobytes()
    assert rng[0, 5] == np.inf and rng[1, 5] == -np.inf


# ---- 3. from_rollout against from_paths ----

def _rollout(H, E, n, m, seed, dtype=np.float32, with_steps=True, p=0.2):
    rs = np.random.RandomState(seed)
    done, term, steps = _boards(H, E, seed, True, with_steps, p)
    obs = (rs.randn(H, E, n) * 2).astype(dtype)
    act = rs.randn(H, E, m).astype(dtype)
    rew = rs.randn(H, E)
    host = dict(observations=obs, actions=act, rewards=rew, done=done, terminated=term, steps=steps)
    dev = {k: (v if k == "steps" else _dev(v)) for k, v in host.items()}
    return host, dev


def _spec(n, m):
    from mjrl_amd.utils.gym_env import EnvSpec
    return EnvSpec(n, m, 1000, 1)


def test_from_rollout_equals_from_paths():
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.engine import DeviceBatch
    n, m = 8, 2
    host, dev = _rollout(40, 6, n, m, seed=2)
    paths = RI.rollout_to_paths(**host)
    want = DeviceBatch.from_paths(paths, torch.device(DEV), baseline=LinearBaseline(_spec(n, m)), obs_dtype=np.float32)
    got = DeviceBatch.from_rollout(baseline=LinearBaseline(_spec(n, m)), **dev)
    assert (got.T, got.P, got.T_demo) == (want.T, want.P, 0) and got.P == len(paths) > 6
    assert np.array_equal(got.lengths, want.lengths) and not got.obs_inexact
    for f in ("obs", "act", "rewards", "path_off", "terminated", "obs_range", "baseline"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f
    assert not got.baseline.any()   # an unfitted LinearBaseline predicts zeros
    # fresh tensors on request, the same bits
    own = DeviceBatch.from_rollout(reuse=False, **dev)
    assert own.obs.data_ptr() != got.obs.data_ptr() and torch.equal(own.obs, got.obs)
    assert torch.equal(own.path_off, got.path_off) and not own.baseline.any()
    # f64 rollouts keep their dtype and have no ranges
    host64, dev64 = _rollout(9, 5, 3, 1, seed=4, dtype=np.float64)
    b64 = DeviceBatch.from_rollout(**dev64)
    assert b64.obs.dtype == b64.act.dtype == torch.float64 and b64.obs_range is None
    assert np.array_equal(b64.obs.cpu().numpy(), RI.rollout_rows(host64["observations"], host64["steps"]))
    # a device mix is refused by name
    with pytest.raises(ValueError, match="rewards is on cpu"):
        DeviceBatch.from_rollout(**dict(dev, rewards=dev["rewards"].cpu()))
    wrong = LinearBaseline(_spec(n + 2, m))
    wrong._coeffs = np.zeros(n + 6)
    with pytest.raises(ValueError, match="LinearBaseline"):
        DeviceBatch.from_rollout(baseline=wrong, **dev)


# ---- 4. end to end ----

class _Env:
    env_id = "rollout-v0"


def _agent(algo, n, m, hidden):
    from mjrl_amd.algos.npg_cg import NPG
    from mjrl_amd.algos.trpo import TRPO
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    spec = _spec(n, m)
    cls = {"npg": NPG, "trpo": TRPO}[algo]
    return cls(_Env(), MLP(spec, hidden_sizes=hidden, seed=0), LinearBaseline(spec), seed=1, device=DEV)


@pytest.mark.parametrize("algo,n,m,hidden,H,E", [("npg", 8, 2, (64, 64), 40, 6), ("trpo", 17, 6, (128, 128), 24, 5),
                                                 ("npg", 376, 17, (64, 64), 8, 5)],
                         ids=["npg-swimmer", "trpo-halfcheetah", "npg-humanoid-split"])
def test_train_from_rollout_equals_train_from_samples(algo, n, m, hidden, H, E):
    host, dev = _rollout(H, E, n, m, seed=7, with_steps=(n != 8))
    gamma, lam = 0.995, 0.97
    a, b = _agent(algo, n, m, hidden), _agent(algo, n, m, hidden)
    if n == 376:
        assert a.engine().split   # the column ranges and the fused pack are on this route
    want = a.train_from_samples(RI.rollout_to_paths(**host), gamma, lam)
    got = b.train_from_rollout(gamma=gamma, gae_lambda=lam, fit_baseline=False, **dev)
    assert got == want and len(got) == 4
    pa, pb = a.policy.get_param_values(), b.policy.get_param_values()
    assert pa.tobytes() == pb.tobytes()
    assert not np.array_equal(pa, _agent(algo, n, m, hidden).policy.get_param_values())   # an update happened
    assert b.running_score == a.running_score and b.baseline._coeffs is None


# ---- 5. the baseline from the packed rows ----

def test_baseline_fit_and_predict_from_the_rollout():
    """H = 400: the time features t / 1000 .. (t / 1000)^3 of paths of a few hundred
    steps are as well conditioned as the sampler's own; float32 observations, so the
    packed rows hold the values the host fit reads."""
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.engine import DeviceBatch
    from mjrl_amd.utils import process_samples
    n, m, gamma = 8, 2, 0.995
    host, dev = _rollout(400, 6, n, m, seed=9, p=0.006)
    agent = _agent("npg", n, m, (64, 64))
    agent.train_from_rollout(gamma=gamma, gae_lambda=0.97, fit_baseline=True, **dev)
    paths = RI.rollout_to_paths(**host)
    process_samples.compute_returns(paths, gamma)
    ref = LinearBaseline(_spec(n, m))
    ref.fit(paths)
    err = np.linalg.norm(agent.baseline._coeffs - ref._coeffs)
    print("fit: |c - c_ref| = %.3e, bound %.3e" % (err, 1e-10 * np.linalg.norm(ref._coeffs)))
    assert err <= 1e-10 * np.linalg.norm(ref._coeffs)
    # the next call's predictions, from the fitted coefficients
    batch = DeviceBatch.from_rollout(baseline=agent.baseline, **dev)
    pred = batch.baseline.cpu().numpy()
    want = np.concatenate([agent.baseline.predict(p) for p in paths])
    bound = np.concatenate([np.abs(agent.baseline._features(p)).dot(np.abs(agent.baseline._coeffs)) for p in paths])
    print("predict: max |d| / bound = %.3e" % np.max(np.abs(pred - want) / bound))
    assert np.all(np.abs(pred - want) <= 1e-12 * bound)


# ---- 6. steady state ----

def test_no_allocation_in_steady_state():
    n, m = 8, 2
    _, dev = _rollout(40, 6, n, m, seed=3)
    agent = _agent("npg", n, m, (64, 64))
    agent.train_from_rollout(**dev)
    agent.train_from_rollout(**dev)
    torch.cuda.synchronize()
    second = torch.cuda.memory_allocated()
    agent.train_from_rollout(**dev)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == second


def test_logs_without_paths():
    """save_logs: the keys _update writes, the fit's, and no success rate."""
    n, m = 8, 2
    _, dev = _rollout(40, 6, n, m, seed=3)
    agent = _agent("npg", n, m, (64, 64))
    agent.save_logs = True
    from mjrl_amd.utils.logger import DataLog
    agent.logger = DataLog()
    agent.train_from_rollout(**dev)
    keys = set(agent.logger.log)
    assert {"stoc_pol_mean", "stoc_pol_std", "stoc_pol_max", "stoc_pol_min", "running_score", "kl_dist",
            "time_VF", "VF_error_before", "VF_error_after"} <= keys and "success_rate" not in keys
