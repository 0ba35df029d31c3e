"""Host side of carried device rollouts (mjrl_amd/samplers/rollout_ingest.py): the
carry of an episode across two calls, defined once — a board cut anywhere and fed its
first part's next carry gives every row the episode time it has on the uncut board —
the "t0" of the equivalent host paths, the time origin of LinearBaseline's features,
bootstrapped returns, and every argument error of the carried route, raised before
the GPU library is loaded."""
import numpy as np
import pytest
import torch

from mjrl_amd.samplers import rollout_ingest as RI
from test_rollout_ingest import DONE, E, H, STEPS, TERM, _agent, _rollout, _spec, no_gpu_library  # noqa: F401


def random_board(rs, H, E, p=0.1):
    """done / terminated / steps with, among the envs (E >= 4): steps 0, steps H, a
    done in the last valid cell, and no done at all."""
    done = (rs.rand(H, E) < p).astype(np.uint8)
    term = (rs.rand(H, E) < 0.5).astype(np.uint8)
    steps = rs.randint(0, H + 1, size=E)
    steps[0], steps[1] = 0, H
    steps[2] = max(int(steps[2]), 1)
    done[steps[2] - 1, 2] = 1          # a done in the last valid cell
    steps[3] = H
    done[:, 3] = 0                     # no done at all
    return done, term, steps.astype(np.int64)


def episode_times(seg, t_shift=0):
    """{(env, step of the board): steps the row's episode had taken before it}"""
    out = {}
    for (e, t0, L, _), c in zip(seg["paths"], seg["path_t0"]):
        for i in range(L):
            out[(e, t0 + i + t_shift)] = int(c) + i
    return out


def test_halves_equal_the_whole():
    rs = np.random.RandomState(0)
    for trial in range(60):
        H_, E_ = int(rs.randint(2, 40)), int(rs.randint(4, 9))
        done, term, steps = random_board(rs, H_, E_)
        c0 = rs.randint(0, 900, size=E_).astype(np.int64)
        c0[rs.rand(E_) < 0.3] = 0
        whole = RI.segment_rollout_reference(done, term, steps, c0)
        for K in sorted({1, H_ // 2, H_ - 1} - {0}):
            a = RI.segment_rollout_reference(done[:K], term[:K], np.minimum(steps, K), c0)
            b = RI.segment_rollout_reference(done[K:], term[K:], np.maximum(steps - K, 0), a["episode_steps_next"])
            times = episode_times(a)
            times.update(episode_times(b, K))
            assert times == episode_times(whole), (trial, K)
            assert np.array_equal(b["episode_steps_next"], whole["episode_steps_next"]), (trial, K)
        # the definitions, restated
        for e in range(E_):
            p0, p1 = whole["env_path"][e], whole["env_path"][e + 1]
            assert [q[0] for q in whole["paths"][p0:p1]] == [e] * (p1 - p0)
            assert (p1 == p0) == (steps[e] == 0)
            if steps[e] == 0:
                assert whole["episode_steps_next"][e] == c0[e]
            elif done[steps[e] - 1, e]:
                assert whole["episode_steps_next"][e] == 0
        assert whole["env_path"][0] == 0 and whole["env_path"][-1] == whole["P"]
        assert whole["episode_steps_next"][3] == c0[3] + H_ and whole["path_t0"].dtype == np.int64


def test_hand_case_with_a_carry():
    seg = RI.segment_rollout_reference(DONE, TERM, STEPS, [7, 11, 13])
    # paths (0, 0, 1) (0, 1, 1) (0, 2, 3) (2, 0, 3): only an env's path that starts at t = 0 has the carry
    assert seg["path_t0"].tolist() == [7, 0, 0, 13]
    assert seg["env_path"].tolist() == [0, 3, 3, 4]
    assert seg["episode_steps_next"].tolist() == [0, 11, 16]   # done at the end; no steps; an open path from t = 0
    no = RI.segment_rollout_reference(DONE, TERM, STEPS)
    assert no["path_t0"].tolist() == [0, 0, 0, 0] and no["episode_steps_next"].tolist() == [0, 0, 3]
    for k in ("paths", "path_off", "path_term", "R"):   # the cut itself does not depend on the carry
        assert np.array_equal(np.asarray(seg[k], dtype=object), np.asarray(no[k], dtype=object))
    for bad in ([1, 2], [1, -1, 0], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="episode_steps"):
            RI.segment_rollout_reference(DONE, TERM, STEPS, bad)


def test_rollout_to_paths_t0():
    rs = np.random.RandomState(3)
    obs, act, rew = rs.randn(H, E, 4), rs.randn(H, E, 2), rs.randn(H, E)
    paths = RI.rollout_to_paths(obs, act, rew, DONE, TERM, STEPS, episode_steps=[7, 11, 13])
    assert [p["t0"] for p in paths] == [7, 0, 0, 13] and all(type(p["t0"]) is int for p in paths)
    zero = RI.rollout_to_paths(obs, act, rew, DONE, TERM, STEPS, episode_steps=torch.zeros(E, dtype=torch.int64))
    assert [p["t0"] for p in zero] == [0, 0, 0, 0]
    plain = RI.rollout_to_paths(obs, act, rew, DONE, TERM, STEPS)
    assert all("t0" not in p for p in plain)   # without a carry: the sampler's dicts, key for key
    for a, b in zip(paths, plain):
        assert all(np.array_equal(a[k], b[k]) for k in ("observations", "actions", "rewards"))


@pytest.mark.parametrize("t0", [0, 1, 37, 999, 1000, 12345])
def test_time_features_with_an_origin_are_the_suffix_rows(t0):
    from mjrl_amd.baselines.linear_baseline import time_features
    rs = np.random.RandomState(t0)
    L = 29
    obs = rs.randn(t0 + L, 5) * 8     # some values beyond the clip
    long = time_features(obs)
    got = time_features(obs[t0:], t0)
    assert got.tobytes() == long[t0:].tobytes()
    assert got.tobytes() == time_features(obs[t0:], t0=np.int64(t0)).tobytes()


def _old_features(obs):
    """LinearBaseline's features as they were before the time origin."""
    o = np.clip(obs, -10.0, 10.0)
    t = (np.arange(o.shape[0]) / 1000.0)[:, None]
    return np.concatenate([o, t, t ** 2, t ** 3, np.ones_like(t)], axis=1)


def test_paths_without_t0_give_unchanged_bits():
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    rs = np.random.RandomState(5)
    paths = [dict(observations=rs.randn(L, 4) * 6, rewards=rs.randn(L), returns=rs.randn(L)) for L in (1, 17, 230)]
    base = LinearBaseline(_spec())
    e0 = base.fit(paths, return_errors=True)
    F = np.concatenate([_old_features(p["observations"]) for p in paths])
    y = np.concatenate([p["returns"] for p in paths])
    c = np.linalg.lstsq(F.T.dot(F) + 1e-5 * np.identity(F.shape[1]), F.T.dot(y), rcond=None)[0]
    assert base._coeffs.tobytes() == c.tobytes()
    for p in paths:
        assert base.predict(p).tobytes() == _old_features(p["observations"]).dot(c).tobytes()
    zero = LinearBaseline(_spec())
    assert zero.fit([dict(p, t0=0) for p in paths], return_errors=True) == e0
    assert zero._coeffs.tobytes() == c.tobytes()
    # and an origin moves them
    moved = dict(paths[1], t0=400)
    assert not np.array_equal(base.predict(moved), base.predict(paths[1]))
    assert base.predict(moved).tobytes() == base._features(moved).dot(c).tobytes()


def reference_discount_sum(x, gamma, terminal=0.0):
    """mjrl/utils/process_samples.py:37-44, the definition."""
    y, run = [], terminal
    for t in range(len(x) - 1, -1, -1):
        run = x[t] + gamma * run
        y.append(run)
    return np.array(y[::-1])


def test_compute_returns_bootstrap(monkeypatch):
    """compute_returns(bootstrap=True) is discount_sum(rewards, gamma, terminal = 0 if
    terminated else baseline[-1]) per path.  The device scan behind it is replaced by
    its NumPy definition here (tests/test_gpu_rollout_carry.py runs the real one)."""
    from mjrl_amd.utils import process_samples as ps

    def host_scan(rewards, baseline, lengths, terminated, gamma, gae_lambda, **kw):
        assert baseline is None and gae_lambda is None and not any(terminated)
        off = np.concatenate([[0], np.cumsum(lengths)])
        parts = [reference_discount_sum(rewards[a:b], gamma) for a, b in zip(off[:-1], off[1:])]
        return (np.concatenate(parts) if parts else np.zeros(0)), None
    monkeypatch.setattr(ps, "device_returns_advantages", host_scan)
    rs = np.random.RandomState(8)
    gamma = 0.995
    paths = [dict(rewards=rs.randn(L), baseline=rs.randn(L) * 30, terminated=t)
             for L, t in ((1, False), (1, True), (40, False), (40, True), (333, False))]
    paths.append(dict(rewards=rs.randn(9), baseline=rs.randn(9)))   # no flag: not terminated
    keep = [p["rewards"].copy() for p in paths]
    ps.compute_returns(paths, gamma, bootstrap=True)
    for p, r in zip(paths, keep):
        terminal = 0.0 if p.get("terminated", False) else p["baseline"][-1]
        assert p["returns"].tobytes() == reference_discount_sum(r, gamma, terminal).tobytes()
        assert np.array_equal(p["rewards"], r)
    ps.compute_returns(paths, gamma)
    for p, r in zip(paths, keep):
        assert p["returns"].tobytes() == reference_discount_sum(r, gamma).tobytes()


# ---- argument errors, without the GPU library ----

def _carry(E_=E, device="cpu"):
    return RI.RolloutCarry(E_, device)


def _bad_carries():
    wrong_dtype = _carry()
    wrong_dtype.episode_steps = torch.zeros(E, dtype=torch.int32)
    wrong_ret = _carry()
    wrong_ret.episode_return = torch.zeros(E, dtype=torch.float32)
    elsewhere = _carry()
    elsewhere.episode_steps = torch.zeros(E, dtype=torch.int64, device="meta")
    return [(torch.zeros(E, dtype=torch.int64), "carry must be a RolloutCarry"),
            ([0, 0, 0], "carry must be a RolloutCarry"),
            (_carry(E + 1), r"carry.episode_steps holds \(4,\) envs, the rollout has E = 3"),
            (elsewhere, "carry.episode_steps is on meta"),
            (wrong_dtype, "carry.episode_steps must be torch.int64"),
            (wrong_ret, "carry.episode_return must be torch.float64")]


@pytest.mark.parametrize("i", range(6))
def test_carry_argument_errors(no_gpu_library, i):  # noqa: F811
    from mjrl_amd.algos.npg_cg import NPG
    from mjrl_amd.engine import DeviceBatch
    carry, match = _bad_carries()[i]
    with pytest.raises(ValueError, match=match):
        DeviceBatch.from_rollout(carry=carry, **_rollout())
    with pytest.raises(ValueError, match=match):
        DeviceBatch.check_rollout(carry=carry, **_rollout())
    with pytest.raises(ValueError, match=match):
        RI.check_rollout(carry=carry, **_rollout())
    with pytest.raises(ValueError, match=match):
        _agent(NPG).train_from_rollout(carry=carry, **_rollout())


def test_a_good_carry_passes_up_to_the_device_check(no_gpu_library):  # noqa: F811
    from mjrl_amd.algos.npg_cg import NPG
    from mjrl_amd.engine import DeviceBatch
    carry = _carry()
    assert carry.episode_steps.dtype == torch.int64 and carry.episode_return.dtype == torch.float64
    assert not carry.episode_steps.any() and not carry.episode_return.any()
    with pytest.raises(ValueError, match="is a CPU tensor"):
        DeviceBatch.from_rollout(carry=carry, **_rollout())
    with pytest.raises(ValueError, match="is a CPU tensor"):
        _agent(NPG).train_from_rollout(carry=carry, bootstrap_returns=True, **_rollout())
    carry.episode_steps += 5
    carry.episode_return += 1.5
    carry.reset(mask=[True, False, True])
    assert carry.episode_steps.tolist() == [0, 5, 0] and carry.episode_return.tolist() == [0.0, 1.5, 0.0]
    carry.reset(torch.tensor([False, True, False]))
    assert not carry.episode_steps.any() and not carry.episode_return.any()
    carry.episode_steps += 2
    carry.reset()
    assert not carry.episode_steps.any()
    with pytest.raises(ValueError, match="mask"):
        carry.reset(mask=[True, False])


@pytest.mark.parametrize("lam", [None, -1.0, 1.5])
def test_bootstrap_returns_needs_gae(no_gpu_library, lam):  # noqa: F811
    from mjrl_amd.algos.npg_cg import NPG
    with pytest.raises(ValueError, match="bootstrap_returns needs GAE"):
        _agent(NPG).train_from_rollout(gae_lambda=lam, bootstrap_returns=True, **_rollout())


def test_from_paths_refuses_a_time_origin(no_gpu_library):  # noqa: F811
    from mjrl_amd.engine import DeviceBatch
    paths = RI.rollout_to_paths(np.zeros((H, E, 4)), np.zeros((H, E, 2)), np.zeros((H, E)), DONE, TERM, STEPS,
                                episode_steps=[7, 0, 0])
    with pytest.raises(ValueError, match='non-zero "t0"'):
        DeviceBatch.from_paths(paths, torch.device("cuda:0"))
    with pytest.raises(ValueError, match="no train_from_rollout"):
        from mjrl_amd.algos.npg_cg import NPG
        _agent(NPG).episode_returns()
