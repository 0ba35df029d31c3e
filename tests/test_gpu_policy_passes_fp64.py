"""mjrl_policy_vpg / _fvp / _eval / _eval_if against an fp64 evaluation
(oracle.npg_cpu.Policy in float64, pass_ref.py) on every kernel that implements
them: k_rows at every hidden width and action width (the linear policy included),
k_fused, k_ks at every (MP, KG), k_kx and k_kx_eval_pipe; with all four
transformations set (one case per family without any), at theta_new != theta_old
for the EVAL pass, and with the rows after the T the passes run over poisoned, so
that a row past T that reaches a sum shows.  The conditions on the inputs are
test_policy_pass_inputs.py's.

Two forms per (case, T).  Tail form: rows.T = T, a partial last tile; what the
passes could read of the 40 rows loaded after T is poison.  Shard form (DAPG's
layout): rows.T = T + 40, the forward pass over all of them, F v and the EVAL pass
over the first T, with adv[T:] = 1e6.

Bars (the project's existing ones): VPG and F v 1e-5 norm-relative, 1e-4 on each
parameter block; surrogate |S - S64| / mean|lr adv| and KL |K - K64| / K64 below
1e-4.

Measured on an MI355X: the worst error of each kind over the cases, row counts and
both forms of a kernel family (what _report prints per line), and beside it the
worst error of the oracle's own fp32 evaluation of the same inputs:

                                  VPG      F v      surr     KL     | fp32 oracle: VPG  F v      surr     KL
  k_rows, linear policy           5.4e-07  1.9e-07  8.7e-07  7.8e-06 |         2.8e-06  2.1e-06  6.1e-07  1.3e-05
  k_fused (EVAL on k_rows 32/64)  3.4e-07  2.4e-07  4.3e-07  5.1e-06 |         9.4e-07  2.2e-07  2.3e-07  1.1e-05
  k_rows 32 / 64 at MP 64         2.5e-07  2.7e-07  8.9e-07  6.9e-06 |         3.0e-07  2.4e-07  4.6e-07  5.6e-06
  k_ks                            7.2e-07  5.6e-07  8.9e-07  4.9e-06 |         6.8e-07  5.0e-07  9.4e-07  6.1e-06
  k_kx, serial EVAL               4.8e-07  3.8e-07  1.2e-06  4.2e-06 |         5.8e-07  4.9e-07  1.2e-06  6.1e-06
  k_kx, k_kx_eval_pipe            4.8e-07  3.8e-07  1.2e-06  4.2e-06 |         5.8e-07  4.9e-07  1.2e-06  6.1e-06
  k_rows 128                      8.0e-07  6.4e-07  1.5e-06  9.6e-06 |         5.6e-07  4.1e-07  8.3e-07  7.6e-06
  k_rows 256                      9.1e-07  8.1e-07  2.2e-06  1.0e-05 |         1.6e-06  1.4e-06  1.1e-06  1.2e-05

So every kernel sits where the fp32 reference itself sits against fp64, a factor of
ten or more inside the bars."""
import numpy as np
import pytest
import torch

import pass_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 777.25


@pytest.fixture(autouse=True)
def _restore_setting():
    from mjrl_amd import _lib
    K = _lib.calls()
    was = K.mjrl_eval_pipe(-1)
    yield
    K.mjrl_eval_pipe(was)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


class _Run:
    """One engine with one (case, T) loaded; the passes through the ABI (eng.K) with
    rows.T, T_fvp / T_eval and adv_vpg chosen per call."""

    def __init__(self, eng, c, d):
        from mjrl_amd import _lib
        self.eng, self.c, self.d, self.st = eng, c, d, _lib.stream_ptr()
        self.theta0, self.theta1, self.v = _dev(d.theta0), _dev(d.theta1), _dev(d.v)
        eng.load_rows(d.obs, d.act, d.adv)
        eng.ws["adv_vpg"][:d.T_load].copy_(_dev(d.adv_vpg))
        # nothing the passes write is left as the allocator gave it
        for k in ("a0", "a1", "mu0", "gu0", "gu1", "gp"):
            eng.ws[k].fill_(1e3)
        eng.ws["ll0"].fill_(d.ll0_poison)

    def rows(self, T_rows):
        return self.eng._rows(T_rows, self.eng.ws["adv_vpg"])

    def vpg(self, T_rows):
        """mjrl_pack_params + mjrl_policy_vpg over rows.T = T_rows; the VPG mean."""
        eng = self.eng
        K, s = eng.K, eng.shape
        _, _, osh, osc = eng.transforms
        K.mjrl_pack_params(s, eng._pad(self.theta0, "theta"), eng.packed_theta, 1, eng.min_log_std, self.st)
        K.mjrl_policy_vpg(s, self.rows(T_rows), eng.packed_theta, osh, osc, eng._scratch(T_rows), eng.pvec["gsum"],
                          self.st)
        return eng._unpad(eng.pvec["gsum"]).double().cpu().numpy() / T_rows

    def fvp(self, T_rows, T):
        """F v + damping v over the first T of rows.T = T_rows rows: the three calls of
        UpdateEngine.fvp."""
        eng = self.eng
        K, s, vv = eng.K, eng.shape, eng.pvec
        K.mjrl_cg_init(s, eng._pad(self.v, "v"), vv["x"], vv["r"], vv["p"], eng.packed_p, eng.cg, eng.done, self.st)
        K.mjrl_policy_fvp(s, self.rows(T_rows), T, eng.packed_theta, eng.packed_p, eng.transforms[3],
                          eng._scratch(T), eng.done, vv["gsum"], self.st)
        K.mjrl_cg_step(s, vv["gsum"], 1.0 / T, R.DAMPING, eng.packed_theta, vv["x"], vv["r"], vv["p"], vv["z"],
                       eng.packed_p, eng.cg, eng.done, 0.0, self.st)
        return eng._unpad(vv["z"]).double().cpu().numpy()

    def eval(self, T_rows, T, skip=None, fill=None):
        """mjrl_policy_eval(_if) at theta1 over the first T rows; (the two sums, the
        per-workgroup records) as f64, read from the statistics buffer and rpart.
        fill: both are set to it before the call."""
        from mjrl_amd.engine import S_EVAL
        eng = self.eng
        K, s = eng.K, eng.shape
        _, _, osh, osc = eng.transforms
        G = K.mjrl_eval_grid(s, T)
        if fill is not None:
            eng.stats[S_EVAL:S_EVAL + 2].fill_(fill)
            eng.ws["rpart"][:2 * G].fill_(fill)
        K.mjrl_pack_params(s, eng._pad(self.theta1, "theta_new"), eng.packed_new, 1, eng.min_log_std, self.st)
        args = (s, self.rows(T_rows), T, eng.packed_new, eng.packed_theta, osh, osc, eng._scratch(T),
                eng.stats[S_EVAL:])
        if skip is None:
            K.mjrl_policy_eval(*args, self.st)
        else:
            K.mjrl_policy_eval_if(*args, skip, self.st)
        torch.cuda.synchronize()
        return eng.stats[S_EVAL:S_EVAL + 2].cpu().numpy(), eng.ws["rpart"][:2 * G].cpu().numpy()


def _check_vec(what, got, want, offs):
    e = R.nrel(got, want)
    assert e < R.BAR_VEC, (what, e)
    for a, b in zip(offs[:-1], offs[1:]):   # every parameter block, not just the norm
        eb = R.nrel(got[a:b], want[a:b])
        assert eb < R.BAR_BLOCK, (what, "block %d:%d" % (a, b), eb)
    return e


def _check_eval(what, sums, d):
    T = d.T
    es = abs(sums[0] / T - d.surr64) / d.absmean64
    ek = abs(sums[1] / T - d.kl64) / d.kl64
    assert es < R.BAR_EVAL, (what, "surrogate", es, sums[0] / T, d.surr64)
    assert ek < R.BAR_EVAL, (what, "KL", ek, sums[1] / T, d.kl64)
    return es, ek


def _report(c, T, form, errs, d):
    """One line per (case, T, form): the kernels' errors against fp64 and, beside them,
    the fp32 oracle's on the same input."""
    print("%s T=%d %s: VPG %.2g (fp32 oracle %.2g) Fv %.2g (%.2g) surr %.2g (%.2g) KL %.2g (%.2g)"
          % (c.id, T, form, errs[0], d.err32["vpg"], errs[1], d.err32["fvp"], errs[2], d.err32["surr"], errs[3],
             d.err32["kl"]))


@pytest.mark.parametrize("c", [pytest.param(c, id=c.id) for c in R.CASES])
def test_passes_vs_fp64(c):
    from mjrl_amd.engine import UpdateEngine
    eng = UpdateEngine(c.n, c.m, None if c.hidden == R.LIN else c.hidden, device="cuda:0", precision=c.precision)
    K, s = eng.K, eng.shape
    assert dict(mp=s.mp, np=s.np, path=eng.accumulate_path(), split=eng.split) == c.expect
    assert (s.h0, s.h1) == c.kernel_hidden
    if c.pipe is not None:
        assert K.mjrl_eval_pipe(c.pipe) in (0, 1) and K.mjrl_eval_pipe(-1) == c.pipe
    offs = R.block_offsets(c)
    tiles = lambda T: -(-T // (64 if c.family not in ("ks", "kx") and s.h0 < 128 else 32))
    multi = [T for T in c.rows() if T > 97]
    for T in multi:   # the smallest T at which a workgroup of the eval pass runs two tiles
        assert K.mjrl_eval_grid(s, T) < tiles(T) and K.mjrl_eval_grid(s, T - 1) == tiles(T - 1), T
    for T in c.rows():
        if T <= 97:
            assert K.mjrl_eval_grid(s, T) == tiles(T)
        d = R.make_case(c, T)
        if c.identity:
            assert d.transforms is None and eng.transforms == (None, None, None, None)
        else:
            eng.set_transformations(*d.transforms)
            assert all(t is not None for t in eng.transforms)
        R_ = d.T_load

        # a. tail form: rows.T = T, the rows after T poisoned
        run = _Run(eng, c, d)
        R.poison(d, eng.ws)
        g = run.vpg(T)
        fv = run.fvp(T, T)
        sums, rpart = run.eval(T, T)
        errs = (_check_vec("tail VPG", g, d.vpg64, offs), _check_vec("tail Fv", fv, d.fv64, offs),
                *_check_eval("tail", sums, d))
        _report(c, T, "tail", errs, d)
        # and the forward pass wrote no cache row past rows.T
        assert bool(eng.ws["mu0"][T:R_].eq(R.MU0_POISON).all()), "tail: mu0 written past rows.T"
        assert bool(eng.ws["ll0"][T:R_].eq(d.ll0_poison).all()), "tail: ll0 written past rows.T"

        # c. mjrl_policy_eval_if: set, nothing is written; clear, mjrl_policy_eval's bytes
        if c.extra:
            flag = torch.ones(1, dtype=torch.int32, device="cuda:0")
            kept = run.eval(T, T, skip=flag, fill=SENTINEL)
            assert np.all(kept[0] == SENTINEL) and np.all(kept[1] == SENTINEL)
            flag.zero_()
            again = run.eval(T, T, skip=flag, fill=SENTINEL)
            assert again[0].tobytes() == sums.tobytes() and again[1].tobytes() == rpart.tobytes()

        # b. shard form: rows.T = T_load; the forward pass over all of them (ordinary
        # adv_vpg), F v and the EVAL pass over the first T with adv[T:] = 1e6
        run = _Run(eng, c, d)
        eng.ws["adv32"][T:R_].fill_(R.ADV_POISON)
        g = run.vpg(R_)
        fv = run.fvp(R_, T)
        sums, _ = run.eval(R_, T)
        errs = (_check_vec("shard VPG", g, d.vpg64_load, offs), _check_vec("shard Fv", fv, d.fv64, offs),
                *_check_eval("shard", sums, d))
        _report(c, T, "shard", errs, d)
