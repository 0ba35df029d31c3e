"""The sliced minibatch Adam steps for policies up to 256 units wide (csrc/policy_fit_wide.hip;
mjrl_policy_fit_wide_epoch, mjrl_policy_mse_wide_epoch; fit_backend = "hip_wide"): the four
kernel tests of test_gpu_policy_fit.py and test_gpu_bc_mse.py through the wide entry points
(one step's gradient and loss against float64 autograd, Adam against the float64 formula, the
split of a run into calls bit for bit, masked rows), the narrow and the wide entry points bit for
bit against each other at widths both accept, and the three classes on the reference's
own runs at these widths (tests/golden/bc_wide.npz, bc2_wide.npz, ppo_wide.npz) against the
fixture and against the torch backend."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_bc_mse as M
from test_gpu_policy_fit import (B1, B2, CLIP, EPS, EXTRA, LR, NAMES, STEP0, T, Net, _steps, assert_gradient,
                                 f64_eval, loss_of, make_state, same_bits, shapes, split)
from test_policy_fit_wide import ppo_wide_agent, ppo_wide_paths, run_bc_wide

pytestmark = pytest.mark.gpu
# (n, m, h0, h1, bs, head, weight_decay, seed): HalfCheetah's and door's widths; one unit past 64
# and a width that is no multiple of 64; several X chunks (the kernels hold 256 columns of X at a
# time) and one unit past a 16-block; the action cap with a single row; m = 1, n one past an X
# chunk, one unit short of the width cap; narrow widths.  The seeds by test_gpu_policy_fit.py's
# rule, asserted from the float64 / float32 CPU evaluations alone (f64_eval): of the seeds 1..12
# meeting it for the step tested and for the masked minibatch, the one whose float32 figure is
# smallest.
CASES = [
    (17, 6, 128, 128, 64, "ppo", 0.0, 11),
    (39, 28, 256, 256, 64, "ppo-aliased", 1e-3, 8),
    (5, 3, 65, 80, 20, "bc", 1e-3, 7),
    (376, 17, 256, 129, 33, "ppo", 0.0, 6),
    (8, 64, 96, 256, 1, "bc", 0.0, 11),
    (257, 1, 16, 255, 64, "ppo-aliased", 0.0, 6),
    (20, 5, 33, 17, 64, "ppo", 0.0, 7),
]
IDS = ["n%d-m%d-h%dx%d-bs%d-%s" % c[:6] for c in CASES]
# the same shapes under the MSE head, (n, m, h0, h1, bs, weight_decay, seed), the seeds by the same
# rule on test_gpu_bc_mse.py's condition
MSE_CASES = [
    (17, 6, 128, 128, 64, 0.0, 2),
    (39, 28, 256, 256, 64, 1e-3, 5),
    (5, 3, 65, 80, 20, 1e-3, 1),
    (376, 17, 256, 129, 33, 0.0, 11),
    (8, 64, 96, 256, 1, 0.0, 6),
    (257, 1, 16, 255, 64, 0.0, 10),
    (20, 5, 33, 17, 64, 0.0, 8),
]
MSE_IDS = ["mse-n%d-m%d-h%dx%d-bs%d" % c[:5] for c in MSE_CASES]
LOSS_OFF = 4 * 64 * 256   # the last step's loss in the scratch


def state(case):
    if len(case) == 8:
        return make_state(*case)
    n, m, h0, h1, bs, wd, seed = case
    return dict(make_state(n, m, h0, h1, bs, "bc", wd, seed), head="mse")


class WideNet:
    """The state on the device and mjrl_policy_fit_wide_epoch / mjrl_policy_mse_wide_epoch calls
    over it.  The scratch starts as NaN: nothing of it may be read before it is written.  Under the
    MSE head adv, ll_old and old_log_std are NaN buffers and kind is 77 (the entry reads none)."""

    def __init__(self, st):
        from mjrl_amd import _lib
        self.lib, self.st, dev = _lib, st, torch.device("cuda:0")
        self.mse = st["head"] == "mse"
        self.nt = 6 if self.mse else 7
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self.p, self.m, self.v = ([up(a) for a in st[k][:self.nt]] for k in ("p", "m_", "v"))
        self.rows = {k: up(st[k]) for k in ("obs", "act", "adv", "ll_old", "old_ls", "in_shift", "in_scale",
                                            "out_shift", "out_scale")}
        if self.mse:
            self.rows["adv"] = self.rows["ll_old"] = torch.full((T + EXTRA,), float("nan"), device=dev)
            self.rows["old_ls"] = torch.full((st["m"],), float("nan"), device=dev)
        nf = C.c_int64()
        _lib.calls().mjrl_policy_fit_wide_scratch(st["n"], st["m"], st["h0"], st["h1"], st["bs"], nf)
        assert nf.value > LOSS_OFF
        self.scratch = torch.full((nf.value,), float("nan"), dtype=torch.float32, device=dev)
        self.d = sum(int(np.prod(s)) for s in shapes(st["n"], st["m"], st["h0"], st["h1"])[:self.nt])

    def epoch(self, idx, nmb, step0=STEP0, grads=False):
        _lib, st, r = self.lib, self.st, self.rows
        net = _lib.MeanNet() if self.mse else _lib.PolicyNet()
        for i in range(self.nt):
            net.p[i], net.exp_avg[i], net.exp_avg_sq[i] = (t[i].data_ptr() for t in (self.p, self.m, self.v))
        head = st["head"]
        ptr = lambda k, on=True: r[k].data_ptr() if on else None   # noqa: E731
        kind = 77 if self.mse else (_lib.POLICY_FIT_BC if head == "bc" else _lib.POLICY_FIT_PPO)
        data = _lib.PolicyFitData(ptr("obs"), ptr("act"), ptr("adv", head != "bc"),
                                  ptr("ll_old", head in ("ppo", "mse")), ptr("old_ls", head in ("ppo-aliased", "mse")),
                                  ptr("in_shift"), ptr("in_scale"), ptr("out_shift"), ptr("out_scale"), T, st["n"],
                                  st["m"], st["h0"], st["h1"], kind, float("nan") if self.mse else CLIP)
        hp = _lib.Adam(LR, B1, B2, EPS, st["wd"], step0)
        dev = self.scratch.device
        idx = torch.as_tensor(np.ascontiguousarray(idx), dtype=torch.int64).to(dev)
        assert idx.numel() >= nmb * st["bs"]
        g = torch.full((nmb, self.d), float("nan"), device=dev) if grads else None
        loss = torch.full((nmb,), float("nan"), device=dev) if grads else None
        fn = _lib.calls().mjrl_policy_mse_wide_epoch if self.mse else _lib.calls().mjrl_policy_fit_wide_epoch
        with torch.cuda.device(dev):
            fn(data, idx, nmb, st["bs"], net, hp, self.scratch, g, loss, _lib.stream_ptr())
            torch.cuda.synchronize()
        return (g.cpu().numpy(), loss.cpu().numpy()) if grads else None

    def host(self):
        return [[t.cpu().numpy() for t in ts] for ts in (self.p, self.m, self.v)]


def reference(st, idx):
    return M.f64_eval(st, idx) if st["head"] == "mse" else f64_eval(st, idx)


def parts(flat, st):
    return M.split(flat, st) if st["head"] == "mse" else split(flat, st)


def check_gradient(st, got, ref):
    (M.assert_gradient if st["head"] == "mse" else assert_gradient)(got, ref)


_ONE = {}


def one_step(case):
    """One step from the case's start state (computed once, shared, never changed): the kernels'
    gradient and loss, the state after it, and the float64 evaluation."""
    if case not in _ONE:
        st = state(case)
        net = WideNet(st)
        g, loss = net.epoch(st["perm"], 1, grads=True)
        _ONE[case] = dict(st=st, grad=parts(g[0], st), loss=float(loss[0]), after=net.host(),
                          last=float(net.scratch[LOSS_OFF].item()), ref=reference(st, st["perm"][:st["bs"]]))
    return _ONE[case]


ALL = CASES + MSE_CASES
ALL_IDS = IDS + MSE_IDS


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_gradient_and_loss_match_float64_autograd(case):
    r = one_step(case)
    ref_g, ref_loss = r["ref"]
    assert all(np.all(np.isfinite(g)) for g in r["grad"]) and np.isfinite(r["loss"])
    check_gradient(r["st"], r["grad"], ref_g)
    print("loss %.9g float64 %.9g" % (r["loss"], ref_loss))
    np.testing.assert_allclose(r["loss"], ref_loss, rtol=1e-5)
    assert r["last"] == r["loss"]


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_adam_arithmetic_matches_the_float64_formula(case):
    """torch's single-tensor Adam in float64 on the kernels' own gradient, every tensor."""
    r = one_step(case)
    st, t = r["st"], STEP0 + 1
    for i, name in enumerate(NAMES[:len(r["grad"])]):
        p, m, v = (st[k][i].astype(np.float64) for k in ("p", "m_", "v"))
        g = r["grad"][i].astype(np.float64) + st["wd"] * p
        m1 = m + (g - m) * (1 - B1)
        v1 = B2 * v + (1 - B2) * g * g
        delta = (LR / (1 - B1 ** t)) * m1 / (np.sqrt(v1) / np.sqrt(1 - B2 ** t) + EPS)
        p1, gm, gv = (r["after"][k][i].astype(np.float64) for k in range(3))
        print("%s: exp_avg %.3g exp_avg_sq %.3g relative, parameters %.3g of the bound" % (
            name, np.max(np.abs(gm - m1) / (np.abs(m1) + 1e-300)), np.max(np.abs(gv - v1) / (np.abs(v1) + 1e-300)),
            np.max(np.abs(p1 - (p - delta)) / (2.0 ** -23 * np.abs(p) + 2e-6 * np.abs(delta)))))
        np.testing.assert_allclose(gm, m1, rtol=1e-6, atol=1e-37, err_msg=name)
        np.testing.assert_allclose(gv, v1, rtol=1e-6, atol=1e-37, err_msg=name)
        assert np.all(np.abs(p1 - (p - delta)) <= 2.0 ** -23 * np.abs(p) + 2e-6 * np.abs(delta)), name


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_partition_into_calls_changes_no_bit(case):
    st = state(case)
    bs = st["bs"]
    runs = []
    for mode in ("five", "ones", "2+3", "five"):
        net = WideNet(st)
        if mode == "ones":
            for k in range(5):
                net.epoch(st["perm"][k * bs:(k + 1) * bs], 1, step0=STEP0 + k)
        elif mode == "2+3":
            net.epoch(st["perm"], 2)
            net.epoch(st["perm"][2 * bs:], 3, step0=STEP0 + 2)
        else:
            net.epoch(st["perm"], 5)
        runs.append(net.host())
    for other in runs[1:]:
        same_bits(runs[0], other)
    # and the steps did move every tensor, away from the one-step state too
    for k, key in enumerate(("p", "m_", "v")):
        for i in range(len(runs[0][k])):
            assert np.all(np.isfinite(runs[0][k][i]))
            assert not np.array_equal(runs[0][k][i], st[key][i])
            assert not np.array_equal(runs[0][k][i], one_step(case)["after"][k][i])


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_rows_out_of_range_are_masked(case):
    """A minibatch holding the indices T and -1: the gradient and loss of the other rows, still
    divided by bs.  Rows T .. T + 7 of every row array hold 1e30: a broken guard fails here.
    (bs = 1: its one row is masked, and gradient and loss are exactly zero.)"""
    st = state(case)
    bs = st["bs"]
    assert all(np.all(st[k][T:] == 1e30) for k in ("obs", "act", "adv", "ll_old"))
    idx = st["perm"][bs:2 * bs].copy()
    idx[1 % bs], idx[(bs - 2) % bs] = T, -1
    g, loss = WideNet(st).epoch(idx, 1, grads=True)
    assert np.all(np.isfinite(g)) and np.isfinite(loss[0])
    if not any(0 <= i < T for i in idx):
        assert not np.any(g) and loss[0] == 0.0
        return
    ref_g, ref_loss = reference(st, idx)
    check_gradient(st, parts(g[0], st), ref_g)
    np.testing.assert_allclose(float(loss[0]), ref_loss, rtol=1e-5)


# (n, m, h0, h1, bs, head) at widths both backends accept, weight decay 1e-3, seed 1
BOTH = [(13, 1, 7, 64, 1, "bc"), (20, 5, 33, 17, 64, "ppo"), (257, 3, 16, 48, 33, "ppo-aliased"),
        (20, 5, 33, 17, 64, "mse")]


@pytest.mark.parametrize("case", BOTH, ids=["n%d-m%d-h%dx%d-bs%d-%s" % c for c in BOTH])
def test_narrow_and_wide_entry_points_leave_the_same_bits(case):
    """Both backends keep one arithmetic contract (csrc/policy_step.h holds the shared pieces), and
    at these widths they order every sum alike: three steps through mjrl_policy_fit_epoch /
    mjrl_policy_mse_epoch and through the wide entry points leave the same parameters, moments,
    gradients and losses, bit for bit."""
    n, m, h0, h1, bs, head = case
    mse = head == "mse"
    st = make_state(n, m, h0, h1, bs, "bc" if mse else head, 1e-3, 1)
    narrow, wide = (M.Net if mse else Net)(st), WideNet(dict(st, head=head))
    (gn, ln), (gw, lw) = (net.epoch(st["perm"], 3, grads=True) for net in (narrow, wide))
    same_bits(narrow.host(), wide.host())
    same_bits([[gn, ln]], [[gw, lw]])
    assert np.all(np.isfinite(gn)) and np.all(np.isfinite(ln)) and len(narrow.host()[0]) == (6 if mse else 7)
    assert float(narrow.scratch[0].item()) == float(wide.scratch[LOSS_OFF].item()) == float(ln[2])


# ---- the classes ------------------------------------------------------------------------------
def _nrel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


_BC = {}


def bc_run(which, backend):
    if (which, backend) not in _BC:
        bc, policy, z = run_bc_wide(which, "cuda:0", backend)
        assert bc.fit_backend == backend
        params = list(policy.trainable_params if which == 1 else policy.model.parameters())
        _BC[which, backend] = (bc, z, policy.get_param_values(), np.array(bc.logger.log["loss"], dtype=np.float64),
                               [float(bc.optimizer.state[p]["step"]) for p in params])
    return _BC[which, backend]


@pytest.mark.parametrize("which", (1, 2))
def test_bc_wide_golden_run_with_the_torch_backend(which):
    """Half the bound of the fused run below, so that the fused route has room of its own."""
    bc, z, params, loss, steps = bc_run(which, "torch")
    print("BC %d wide, torch backend on the GPU: parameters %.3g from the reference's (in norm)" % (
        which, _nrel(params, z["final"])))
    np.testing.assert_allclose(loss, z["loss"], rtol=1e-4)
    assert _nrel(params, z["final"]) <= 5e-4
    assert bc.trainer().graphable and bc.trainer().device.type == "cuda"


@pytest.mark.parametrize("which", (1, 2))
def test_bc_wide_golden_run_with_the_hip_wide_backend(which):
    bc, z, params, loss, steps = bc_run(which, "hip_wide")
    _, _, tparams, _, tsteps = bc_run(which, "torch")
    ref = z["final"]
    print("BC %d hip_wide: parameters %.3g from the reference's, %.3g from the torch backend's (in norm)" % (
        which, _nrel(params, ref), _nrel(params, tparams)))
    np.testing.assert_allclose(loss, z["loss"], rtol=1e-4)
    assert _nrel(params, ref) <= 1e-3
    assert _nrel(params, tparams) <= 1e-3
    assert steps == tsteps == [2 * int(300 / 32)] * (7 if which == 1 else 6)
    if which == 2:   # log_std: bit for bit, not trained
        assert np.array_equal(params[-3:].view(np.uint32), z["after_init"][-3:].view(np.uint32))
    assert bc.logger.log["epoch"] == [0, 1, 2]
    assert hasattr(bc.trainer(), "_hip_wide_scratch") and not hasattr(bc.trainer(), "_hip_scratch")


_PPO = {}


def ppo_run(backend):
    if backend not in _PPO:
        ppo, policy, z = ppo_wide_agent(None, backend)
        out = []
        for it in range(2):
            assert ppo._aliasing() == ([False] * 7 if it == 0 else [True] * 6 + [False])
            np.random.seed(int(z["np_seed%d" % it]))
            stats = ppo.train_from_paths(ppo_wide_paths(z, it))
            out.append(dict(stats=stats, params=policy.get_param_values(), kl=ppo.logger.log["kl_dist"][-1],
                            surr=ppo.logger.log["surr_improvement"][-1], score=ppo.logger.log["running_score"][-1],
                            steps=_steps(ppo.optimizer, policy)))
        _PPO[backend] = (z, out)
    return _PPO[backend]


def test_ppo_wide_golden_run_with_the_torch_backend():
    z, tor = ppo_run("torch")
    for it in range(2):
        rel = _nrel(tor[it]["params"], z["params%d" % it])
        print("PPO wide iteration %d, torch backend on the GPU: parameters %.3g from the reference's" % (it, rel))
        assert rel <= 5e-4, it


def test_ppo_wide_golden_run_with_the_hip_wide_backend():
    """test_gpu_policy_fit.py::test_ppo_golden_run_with_the_hip_backend at hidden (128, 128): the
    second iteration is the aliased form."""
    z, hip = ppo_run("hip_wide")
    _, tor = ppo_run("torch")
    for it in range(2):
        h, t = hip[it], tor[it]
        np.testing.assert_allclose(h["stats"], z["base_stats%d" % it], rtol=1e-12)
        ref = z["params%d" % it]
        print("PPO wide iteration %d hip_wide: parameters %.3g from the reference's, %.3g from the torch backend's; "
              "kl %.6g (%.6g) surr %.6g (%.6g)" % (it, _nrel(h["params"], ref), _nrel(h["params"], t["params"]),
                                                   h["kl"], z["kl_dist%d" % it], h["surr"],
                                                   z["surr_improvement%d" % it]))
        assert _nrel(h["params"], ref) <= 1e-3, it
        assert abs(h["kl"] - z["kl_dist%d" % it]) <= 0.05 * abs(z["kl_dist%d" % it]) + 1e-6
        assert abs(h["surr"] - z["surr_improvement%d" % it]) <= 0.05 * abs(z["surr_improvement%d" % it]) + 1e-5, it
        np.testing.assert_allclose(h["score"], z["running_score%d" % it], rtol=1e-12)
        assert _nrel(h["params"], t["params"]) <= 1e-3, it
        assert h["steps"] == t["steps"] == [(it + 1) * 2 * int(600 / 64)] * 7
