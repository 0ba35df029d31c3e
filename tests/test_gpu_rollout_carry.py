"""Carried device rollouts on the GPU: mjrl_rollout_segments_carry against the NumPy
reference (samplers/rollout_ingest.py), the LinearBaseline predict and fit with a time
origin per path against the host class on the "t0" paths, two halves of a rollout
with a carry against the uncut rollout, mjrl_returns_seeded bit for bit against
discount_sum(terminal=), and train_from_rollout(carry=, bootstrap_returns=) end to
end."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mjrl_amd.samplers import rollout_ingest as RI
from test_gpu_rollout_ingest import DEV, _agent, _boards, _dev, _rollout, _spec
from test_rollout_carry import reference_discount_sum
from test_rollout_ingest import hand_case

pytestmark = pytest.mark.gpu
I64 = dict(dtype=torch.int64, device=DEV)


def _segments(done, term, steps, cap, carry=None, alias=False, plain=False):
    """One call of mjrl_rollout_segments_carry (plain: of mjrl_rollout_segments) on
    sentinel-filled outputs; returns them as NumPy, whole buffers."""
    from mjrl_amd import _lib
    K = _lib.calls()
    H, E = done.shape
    T = int(RI.check_steps(steps, H, E).sum())
    nw = C.c_int64()
    K.mjrl_rollout_segments_scratch(E, nw)
    out = dict(env_row=torch.full((E + 1,), -7, **I64), path_off=torch.full((T + 1,), -7, **I64),
               path_term=torch.full((max(T, 1),), 0xAB, dtype=torch.uint8, device=DEV),
               counts=torch.full((2,), -7, **I64), path_t0=torch.full((max(T, 1),), -7, **I64),
               env_path=torch.full((E + 1,), -7, **I64), c_next=torch.full((E,), -7, **I64))
    scratch = torch.zeros(max(nw.value, 1), **I64)
    d_done = _dev(done).bool() if (H + E) % 2 else _dev(done)
    d_term = None if term is None else _dev(term)
    d_steps = None if steps is None else _dev(np.asarray(steps, np.int64))
    if plain:
        K.mjrl_rollout_segments(d_done, d_term, d_steps, H, E, cap, out["env_row"], out["path_off"], out["path_term"],
                                out["counts"], scratch, _lib.stream_ptr())
    else:
        c_in = None if carry is None else _dev(np.asarray(carry, np.int64))
        if alias:
            out["c_next"] = c_in
        K.mjrl_rollout_segments_carry(d_done, d_term, d_steps, H, E, cap, c_in, out["env_row"], out["path_off"],
                                      out["path_term"], out["path_t0"], out["env_path"], out["c_next"], out["counts"],
                                      scratch, _lib.stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1. the segments kernel with a carry ----

@pytest.mark.parametrize("with_steps", [False, True], ids=["full", "steps"])
@pytest.mark.parametrize("with_term", [False, True], ids=["done", "term"])
@pytest.mark.parametrize("H,E", [(1, 1), (5, 3), (7, 64), (3, 65), (2, 257), (33, 1000)])
def test_segments_carry_matches_the_reference(H, E, with_term, with_steps):
    done, term, steps = _boards(H, E, 11 * H + E, with_term, with_steps)
    rs = np.random.RandomState(H + 3 * E)
    carry = rs.randint(0, 901, size=E).astype(np.int64)
    carry[rs.rand(E) < 0.3] = 0
    carry[0] = 900
    ref = RI.segment_rollout_reference(done, term, steps, carry)
    P, T = ref["P"], ref["T"]
    got = _segments(done, term, steps, T, carry)
    assert got["counts"].tolist() == [P, T]
    assert np.array_equal(got["env_row"], ref["R"])
    assert np.array_equal(got["path_off"][:P + 1], ref["path_off"])
    assert np.array_equal(got["path_term"][:P], ref["path_term"])
    assert np.array_equal(got["path_t0"][:P], ref["path_t0"])
    assert np.array_equal(got["env_path"], ref["env_path"])
    assert np.array_equal(got["c_next"], ref["episode_steps_next"])
    # the sentinels survive past the tables
    assert np.all(got["path_off"][P + 1:] == -7) and np.all(got["path_term"][P:] == 0xAB)
    assert np.all(got["path_t0"][P:] == -7)
    # episode_steps_out over episode_steps_in: the same values
    inplace = _segments(done, term, steps, T, carry, alias=True)
    assert np.array_equal(inplace["c_next"], ref["episode_steps_next"])
    assert np.array_equal(inplace["path_t0"][:P], ref["path_t0"])
    # a null carry: the old entry's bits in every output they share, zeros as the origin
    old = _segments(done, term, steps, T, plain=True)
    null = _segments(done, term, steps, T, None)
    for k in ("env_row", "path_off", "path_term", "counts"):
        assert null[k].tobytes() == old[k].tobytes() == got[k].tobytes(), k
    assert not null["path_t0"][:P].any()
    assert np.array_equal(null["c_next"], RI.segment_rollout_reference(done, term, steps)["episode_steps_next"])


def test_segments_carry_edges():
    """A path_cap below P (nothing at or beyond it is written, path_t0 included), a
    negative carry (clamped to 0), and every new array null (the old entry)."""
    from mjrl_amd import _lib
    K = _lib.calls()
    done, term, steps = hand_case()
    ref = RI.segment_rollout_reference(done, term, steps, [7, 11, 13])
    got = _segments(done, term, steps, 2, [7, 11, 13])
    assert got["counts"].tolist() == [ref["P"], ref["T"]]
    assert got["path_t0"].tolist() == ref["path_t0"].tolist()[:2] + [-7] * (ref["T"] - 2)
    assert got["path_off"].tolist()[:2] == ref["path_off"].tolist()[:2] and set(got["path_off"].tolist()[2:]) == {-7}
    assert got["env_path"].tolist() == ref["env_path"].tolist()
    assert got["c_next"].tolist() == ref["episode_steps_next"].tolist()
    neg = _segments(done, term, steps, ref["T"], [-5, -1, 13])
    zero = RI.segment_rollout_reference(done, term, steps, [0, 0, 13])
    assert neg["path_t0"][:ref["P"]].tolist() == zero["path_t0"].tolist()
    assert neg["c_next"].tolist() == zero["episode_steps_next"].tolist()
    old = _segments(done, term, steps, ref["T"], plain=True)
    env_row, counts = torch.full((4,), -7, **I64), torch.full((2,), -7, **I64)
    path_off = torch.full((ref["T"] + 1,), -7, **I64)
    path_term = torch.full((ref["T"],), 0xAB, dtype=torch.uint8, device=DEV)
    K.mjrl_rollout_segments_carry(_dev(done), _dev(term), _dev(np.asarray(steps, np.int64)), 5, 3, ref["T"], None,
                                  env_row, path_off, path_term, None, None, None, counts, torch.zeros(9, **I64),
                                  _lib.stream_ptr())
    torch.cuda.synchronize()
    assert env_row.cpu().numpy().tobytes() == old["env_row"].tobytes()
    assert path_off.cpu().numpy().tobytes() == old["path_off"].tobytes()
    assert path_term.cpu().numpy().tobytes() == old["path_term"].tobytes()
    with pytest.raises(_lib.MjrlError, match="mjrl_rollout_segments_carry"):
        K.mjrl_rollout_segments_carry(None, None, None, 5, 3, 8, None, env_row, path_off, path_term, None, None, None,
                                      counts, torch.zeros(9, **I64), _lib.stream_ptr())


# ---- 2. predict with a time origin ----

def _carry_of(values):
    c = RI.RolloutCarry(len(values), DEV)
    c.episode_steps.copy_(torch.as_tensor(np.asarray(values, np.int64)))
    return c


def _fitted(n, m, seed):
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    base = LinearBaseline(_spec(n, m))
    c = np.random.RandomState(seed).randn(n + 4)
    base._coeffs = np.where(np.abs(c) < 0.05, 0.05, c)   # every coefficient non-zero, the time ones too
    return base


def _bound(base, paths):
    return np.concatenate([np.abs(base._features(p)).dot(np.abs(base._coeffs)) for p in paths])


@pytest.mark.parametrize("n", [1, 8, 17])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_predict_with_a_time_origin(dtype, n):
    from mjrl_amd.engine import DeviceBatch
    m, E = 2, 6
    host, dev = _rollout(40, E, n, m, seed=20 + n, dtype=dtype)
    c0 = np.random.RandomState(n).randint(1, 901, size=E)
    base = _fitted(n, m, n)
    carry = _carry_of(c0)
    batch = DeviceBatch.from_rollout(baseline=base, carry=carry, reuse=False, **dev)
    ref = RI.segment_rollout_reference(host["done"], host["terminated"], host["steps"], c0)
    assert np.array_equal(batch.path_t0.cpu().numpy(), ref["path_t0"]) and batch.path_t0.any()
    assert np.array_equal(batch.env_path.cpu().numpy(), ref["env_path"])
    assert np.array_equal(carry.episode_steps.cpu().numpy(), ref["episode_steps_next"])
    paths = RI.rollout_to_paths(episode_steps=c0, **host)
    want = np.concatenate([base.predict(p) for p in paths])
    pred = batch.baseline.cpu().numpy()
    bound = _bound(base, paths)
    print("predict t0 %s n=%d: max |d| / bound = %.3e" % (np.dtype(dtype).name, n, np.max(np.abs(pred - want) / bound)))
    assert np.all(np.abs(pred - want) <= 1e-12 * bound)
    # the origin is what makes the difference
    plain = DeviceBatch.from_rollout(baseline=base, reuse=False, **dev)
    assert plain.path_t0 is None and not torch.equal(plain.baseline, batch.baseline)


# ---- 3. two halves with a carry against the uncut rollout ----

def test_two_halves_with_a_carry_equal_the_uncut_rollout():
    from mjrl_amd.engine import DeviceBatch
    n, m, H, E, K = 8, 2, 40, 6, 20
    host, dev = _rollout(H, E, n, m, seed=31)
    steps = np.asarray(host["steps"], np.int64)
    c0 = np.array([0, 17, 900, 3, 250, 0])
    base = _fitted(n, m, 3)
    whole_c = _carry_of(c0)
    whole = DeviceBatch.from_rollout(baseline=base, carry=whole_c, reuse=False, **dev)
    carry = _carry_of(c0)
    halves = []
    for lo, hi, s in ((0, K, np.minimum(steps, K)), (K, H, np.maximum(steps - K, 0))):
        part = {k: (v[lo:hi].contiguous() if k != "steps" else [int(x) for x in s]) for k, v in dev.items()}
        halves.append((DeviceBatch.from_rollout(baseline=base, carry=carry, reuse=False, **part), s))
    assert torch.equal(carry.episode_steps, whole_c.episode_steps)
    pw = whole.baseline.cpu().numpy()
    bound = _bound(base, RI.rollout_to_paths(episode_steps=c0, **host))
    R = np.concatenate([[0], np.cumsum(steps)])
    checked = 0
    for (b, s), t_lo in zip(halves, (0, K)):
        ph, Rh = b.baseline.cpu().numpy(), np.concatenate([[0], np.cumsum(s)])
        for e in range(E):
            for t in range(int(s[e])):
                r = R[e] + t_lo + t
                assert abs(pw[r] - ph[Rh[e] + t]) <= 1e-12 * bound[r], (e, t_lo + t)
                checked += 1
    assert checked == whole.T > 0


# ---- 4. the fit with a time origin ----

def test_fit_with_a_time_origin():
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.utils import process_samples
    n, m, gamma, E = 8, 2, 0.995, 6
    host, dev = _rollout(400, E, n, m, seed=9, p=0.006)
    c0 = np.array([0, 120, 900, 45, 333, 610])
    agent = _agent("npg", n, m, (64, 64))
    agent.train_from_rollout(gamma=gamma, gae_lambda=0.97, fit_baseline=True, carry=_carry_of(c0), **dev)
    paths = RI.rollout_to_paths(episode_steps=c0, **host)
    process_samples.compute_returns(paths, gamma)
    ref = LinearBaseline(_spec(n, m))
    ref.fit(paths)
    err = np.linalg.norm(agent.baseline._coeffs - ref._coeffs)
    print("fit t0: |c - c_ref| = %.3e, bound %.3e" % (err, 1e-10 * np.linalg.norm(ref._coeffs)))
    assert err <= 1e-10 * np.linalg.norm(ref._coeffs)
    plain = LinearBaseline(_spec(n, m))
    plain.fit([{k: v for k, v in p.items() if k != "t0"} for p in paths])
    assert np.linalg.norm(plain._coeffs - ref._coeffs) > 1e-6 * np.linalg.norm(ref._coeffs)   # the origin matters


# ---- 5. seeded returns ----

def test_returns_seeded_bit_for_bit():
    from mjrl_amd import _lib
    from mjrl_amd.utils import process_samples
    K = _lib.calls()
    rs = np.random.RandomState(12)
    gamma = 0.995
    #           open fragments of every window edge, terminated ones, empty ones
    lengths = [1, 2, 63, 0, 64, 65, 1023, 7, 1024, 0, 1025, 2500, 1, 64, 1024, 2500, 0]
    flags = [0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 1, 0]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    T = int(off[-1])
    rew, base = rs.randn(T), rs.randn(T) * 40
    before = rs.randn(T)   # what the GAE scan would have left: any values
    ret = _dev(before.copy())
    K.mjrl_returns_seeded(_dev(rew), _dev(base), _dev(off), _dev(np.array(flags, np.uint8)), len(lengths), gamma, ret,
                          _lib.stream_ptr())
    torch.cuda.synchronize()
    got = ret.cpu().numpy()
    for p, (L, f) in enumerate(zip(lengths, flags)):
        a, b = off[p], off[p + 1]
        want = before[a:b] if f or L == 0 else reference_discount_sum(rew[a:b], gamma, base[b - 1])
        assert got[a:b].tobytes() == want.tobytes(), (p, L, f)
    # the project's own discount_sum(terminal=) (the exact GAE scan) agrees
    a, b = off[6], off[7]
    assert got[a:b].tobytes() == process_samples.discount_sum(rew[a:b], gamma, terminal=base[b - 1]).tobytes()
    # P = 0: nothing to do, nothing read
    assert K.mjrl_returns_seeded(None, None, None, None, 0, gamma, None, _lib.stream_ptr()) == _lib.MJRL_OK
    with pytest.raises(_lib.MjrlError, match="mjrl_returns_seeded"):
        K.mjrl_returns_seeded(None, None, None, None, 3, gamma, None, _lib.stream_ptr())


# ---- 6. end to end ----

N, M, HID, H6, E6 = 8, 2, (64, 64), 40, 6
GAMMA, LAM = 0.995, 0.97
MID = [0, 120, 900, 45, 333, 610]


def test_a_zero_carry_changes_nothing():
    host, dev = _rollout(H6, E6, N, M, seed=41)
    a, b = _agent("npg", N, M, HID), _agent("npg", N, M, HID)
    carry = RI.RolloutCarry(E6, DEV)
    want = a.train_from_rollout(gamma=GAMMA, gae_lambda=LAM, **dev)
    got = b.train_from_rollout(gamma=GAMMA, gae_lambda=LAM, carry=carry, **dev)
    assert got == want and len(got) == 4
    assert a.policy.get_param_values().tobytes() == b.policy.get_param_values().tobytes()
    assert a.baseline._coeffs.tobytes() == b.baseline._coeffs.tobytes()
    ref = RI.segment_rollout_reference(host["done"], host["terminated"], host["steps"])
    assert np.array_equal(carry.episode_steps.cpu().numpy(), ref["episode_steps_next"])
    assert carry.episode_steps.any()


def _timeline(hosts):
    """Per env, the valid cells of consecutive rollouts in order: (call, reward, done)."""
    E = hosts[0]["done"].shape[1]
    lines = [[] for _ in range(E)]
    for k, h in enumerate(hosts):
        for e in range(E):
            for t in range(int(h["steps"][e])):
                lines[e].append((k, float(h["rewards"][t, e]), bool(h["done"][t, e])))
    return lines


def _episodes_ending_in(lines, call):
    """(rewards of the whole episode) for every episode whose done cell lies in `call`,
    env-ascending then time-ascending: the order of the closed paths."""
    out = []
    for line in lines:
        cur = []
        for k, r, d in line:
            cur.append(r)
            if d:
                if k == call:
                    out.append(cur)
                cur = []
    return out


def test_second_call_origin_bootstrap_and_episode_returns():
    """The environments start mid-episode (MID: up to 900 steps in, what a batched
    simulator's envs are at when a run of 40-step rollouts is picked up), so the time
    features of the 40-step paths span [0, 0.95] and the fit is as well posed as
    the sampler's own: cond(F^T F + reg I) = 1.4e5 on the second rollout, and the host
    fit itself moves by 4e-12 |c| when its Gram is summed in another row order.  With
    every env at step 0 the second call's carries are at most 14, a <= 0.054, cond =
    6.8e7, the host fit moves by 5e-11 |c| under the same reordering, and the
    device fit measured 1.09e-8 against the bound 8.6e-9: the bound sits at the
    reference's own rounding there, so that start checks nothing about the carry."""
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.engine import DeviceBatch
    from mjrl_amd.utils import process_samples
    host1, dev1 = _rollout(H6, E6, N, M, seed=42, p=0.05)
    host2, dev2 = _rollout(H6, E6, N, M, seed=43, p=0.05)
    b, c = _agent("npg", N, M, HID), _agent("npg", N, M, HID)
    cb, cc = _carry_of(MID), _carry_of(MID)
    b.save_logs = True
    from mjrl_amd.utils.logger import DataLog
    b.logger = DataLog()
    b.train_from_rollout(gamma=GAMMA, gae_lambda=LAM, carry=cb, **dev1)
    c.train_from_rollout(gamma=GAMMA, gae_lambda=LAM, carry=cc, **dev1)
    assert b.policy.get_param_values().tobytes() == c.policy.get_param_values().tobytes()
    assert torch.equal(cb.episode_steps, cc.episode_steps) and cb.episode_steps.any()
    lines = _timeline([host1, host2])
    got, eps = b.episode_returns(), _episodes_ending_in(lines, 0)
    assert len(got) == len(eps) > 0
    for g, r in zip(got, eps):
        assert abs(g - math.fsum(r)) <= len(r) * 2.0 ** -52 * math.fsum(abs(x) for x in r)
    assert b.logger.log["episodes_done"][-1] == len(eps)
    c_before = cb.episode_steps.cpu().numpy().copy()
    # the predictions the second call will read: the fitted coefficients, the carried origin
    probe = RI.RolloutCarry(E6, DEV)
    probe.episode_steps.copy_(cb.episode_steps)
    base2 = DeviceBatch.from_rollout(baseline=b.baseline, carry=probe, reuse=False, **dev2).baseline.cpu().numpy()
    # c forgets its carry: the same call, the clocks of the open episodes restarted
    cc.reset()
    b.train_from_rollout(gamma=GAMMA, gae_lambda=LAM, carry=cb, bootstrap_returns=True, **dev2)
    c.train_from_rollout(gamma=GAMMA, gae_lambda=LAM, carry=cc, bootstrap_returns=True, **dev2)
    assert not np.array_equal(b.policy.get_param_values(), c.policy.get_param_values())   # the origin reaches the update
    assert torch.equal(cb.episode_steps, probe.episode_steps)
    # bootstrapped fit targets: the host fit on the "t0" paths with the same predictions
    paths = RI.rollout_to_paths(episode_steps=c_before, **host2)
    off = np.concatenate([[0], np.cumsum([len(p["rewards"]) for p in paths])])
    for i, p in enumerate(paths):
        p["baseline"] = base2[off[i]:off[i + 1]]
    assert any(not p["terminated"] and p["baseline"][-1] != 0.0 for p in paths)
    process_samples.compute_returns(paths, GAMMA, bootstrap=True)
    ref = LinearBaseline(_spec(N, M))
    ref.fit(paths)
    err = np.linalg.norm(b.baseline._coeffs - ref._coeffs)
    print("bootstrapped fit: |c - c_ref| = %.3e, bound %.3e" % (err, 1e-10 * np.linalg.norm(ref._coeffs)))
    assert err <= 1e-10 * np.linalg.norm(ref._coeffs)
    # whole-episode returns: episodes that ended in the second call, over both rollouts
    got, eps = b.episode_returns(), _episodes_ending_in(lines, 1)
    assert len(got) == len(eps) > 0
    for g, r in zip(got, eps):
        assert abs(g - math.fsum(r)) <= len(r) * 2.0 ** -52 * math.fsum(abs(x) for x in r)
    # at least one of them began in the first call, or the carry of returns was not exercised
    first = _episodes_ending_in(_timeline([host2]), 0)
    assert any(len(r) != len(q) for r, q in zip(eps, first))
    assert b.logger.log["episodes_done"][-1] == len(eps)
    assert abs(b.logger.log["episode_return_mean"][-1] - np.mean(got)) <= 1e-12 * np.max(np.abs(got))
    with pytest.raises(ValueError, match="bootstrap_returns needs GAE"):
        b.train_from_rollout(gamma=GAMMA, gae_lambda=None, carry=cb, bootstrap_returns=True, **dev2)


def test_no_allocation_in_steady_state_with_a_carry():
    _, dev = _rollout(H6, E6, N, M, seed=3)
    agent = _agent("npg", N, M, HID)
    carry = RI.RolloutCarry(E6, DEV)
    kw = dict(carry=carry, bootstrap_returns=True)
    agent.train_from_rollout(**kw, **dev)
    agent.train_from_rollout(**kw, **dev)
    torch.cuda.synchronize()
    second = torch.cuda.memory_allocated()
    agent.train_from_rollout(**kw, **dev)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == second
