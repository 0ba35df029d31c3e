"""The inputs of test_gpu_policy_passes_fp64.py, checked with the reference alone
(pass_ref.py, oracle.npg_cpu): a comparison with fp64 at 1e-4 only means something
where the step is large enough that the reference's own fp32 evaluation does not
cancel, small enough that no likelihood ratio explodes, and where a poisoned tail
row would be seen.  A condition on the inputs belongs here, not next to the
kernel."""
import numpy as np
import pytest
import torch

import pass_ref as R
from oracle import npg_cpu as O

PAIRS = [pytest.param(c, T, id="%s-T%d" % (c.id, T)) for c in R.CASES if c.pipe in (None, 0) for T in c.rows()]


def test_table_covers_every_instance():
    """A set comparison on (kernel hidden, mp, family, KG, pipe): every instance the
    passes had no fp64 anchor on, and the cases with their own reason."""
    L, H32, H64, H128, H256 = R.LIN, R.H32, R.H64, R.H128, R.H256
    want = {(L, 16, "rows", None, None), (L, 32, "rows", None, None), (L, 64, "rows", None, None),
            (H32, 16, "fused", None, None), (H32, 32, "fused", None, None), (H32, 64, "rows", None, None),
            (H64, 16, "fused", None, None), (H64, 32, "fused", None, None), (H64, 64, "rows", None, None),
            (H128, 16, "rows", None, None), (H128, 32, "rows", None, None), (H128, 64, "rows", None, None),
            (H256, 16, "rows", None, None), (H256, 32, "rows", None, None), (H256, 64, "rows", None, None)}
    want |= {(H64, mp, "ks", kg, None) for mp in (16, 32) for kg in (2, 4, 6, 8, 12)}
    want |= {(H64, mp, "kx", kg, pipe) for mp in (16, 32) for kg in (4, 8, 12) for pipe in (0, 1)}
    assert {c.instance for c in R.CASES} == want
    by = lambda **kw: [c for c in R.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    # np = 80: the linear policy's third 32-column block and (128, 128)'s k_wgrad fallback
    assert by(hidden=L, n=70, m=40)[0].expect["np"] == 80 and by(hidden=H128, n=70, m=40)[0].expect["np"] == 80
    assert by(hidden=H64, n=20, m=6)[0].expect == dict(mp=16, np=32, path=1, split=False)   # KG = 1: not k_ks
    assert by(hidden=(48, 32))[0].kernel_hidden == H64                                      # the padded real shape
    # one case per family without transformations, one with the extra row counts
    fam = lambda c: (c.family, c.kernel_hidden if c.family == "rows" and c.kernel_hidden[0] in (0, 128, 256) else None)
    fams = {fam(c) for c in R.CASES}
    assert {fam(c) for c in R.CASES if c.identity} == fams
    assert {fam(c) for c in R.CASES if c.extra} == fams - {("rows", None)}   # k_rows 32 / 64 is the k_fused shapes' EVAL
    for c in R.CASES:
        assert (33 in c.rows() and 97 in c.rows()) and (len(c.rows()) == 5) == c.extra
        s = R.V.make_shape(c.n, c.m, *c.kernel_hidden)
        assert (c.expect["mp"], c.expect["np"]) == (s.mp, s.np)
        assert c.expect["split"] == (c.family == "kx") == (c.pipe is not None)
    assert len({c.id for c in R.CASES}) == len(R.CASES)


@pytest.mark.parametrize("c,T", PAIRS)
def test_inputs_meet_the_conditions(c, T):
    d = R.make_case(c, T)
    bar = R.BAR_EVAL
    lr, adv = d.lr[:T], d.adv[:T]
    # the truth's parts agree with the oracle's own functions
    assert abs(np.mean(lr * adv) - d.surr64) <= 1e-12 * d.absmean64
    assert abs(np.mean(d.kl_rows[:T]) - d.kl64) <= 1e-12 * d.kl64
    print("%s T=%d: step %.3g KL %.4f max ratio %.3g | fp32 oracle: VPG %.2g Fv %.2g surr %.2g KL %.2g | ll0 poison %.1f"
          % (c.id, T, d.step_scale, d.kl64, lr.max(), d.err32["vpg"], d.err32["fvp"], d.err32["surr"],
             d.err32["kl"], d.ll0_poison))
    assert 0.02 <= d.kl64 <= 0.1, d.kl64
    assert lr.max() <= 50, lr.max()
    # the reference's own fp32 evaluation: within a quarter of the GPU bar of fp64
    assert d.err32["surr"] <= bar / 4, d.err32
    assert d.err32["kl"] <= bar / 4, d.err32
    # log-stds stay above the clamp (the packed parameters are the given ones)
    assert d.theta1[-c.m:].min() > -3.0 and d.theta0[-c.m:].min() > -3.0
    # the poison works: a counted tail row moves every sum by more than 100 bars
    assert d.ll0_poison <= R.LL0_POISON
    surr_moves = np.exp(d.ll_new[T:] - d.ll0_poison) * R.ADV_POISON / (T * d.absmean64)
    assert surr_moves.min() > 100 * bar, surr_moves.min()
    assert np.exp(d.ll_new[T:] - d.ll0_poison).max() * R.ADV_POISON < 1e36      # and stays a finite f32
    for i in (T, T + R.TAIL // 2, d.T_load - 1):
        s, k, g = R.poisoned_row_moves(c, d, i)
        assert s > 100 * bar and k > 100 * bar and g > 100 * R.BAR_VEC, (i, s, k, g)


def test_eval_rows_is_the_oracles_formula():
    """eval_rows against Policy.surrogate / Policy.kl in fp32 too (another dtype, the
    linear policy, no transformations)."""
    c = [c for c in R.CASES if c.hidden == R.LIN and c.identity][0]
    d = R.make_case(c, 33)
    p = R._policy(c, d, d.theta0, d.theta1, torch.float32)
    lr, kl, _, _ = R.eval_rows(p, d.obs, d.act)
    assert np.mean(lr * d.adv) == pytest.approx(float(p.surrogate(d.obs, d.act, d.adv).detach()), rel=1e-5, abs=1e-6)
    assert np.mean(kl) == pytest.approx(float(p.kl(d.obs, d.act).detach()), rel=1e-5)
    assert O.param_shapes(c.n, c.m, None) == [(c.m, c.n), (c.m,), (c.m,)]
