"""The fused MSE head of the policy fit (csrc/policy_fit.hip, mjrl_policy_mse_epoch;
behavior_cloning_2.BC.fit_backend = "hip"): one step's gradient and loss against a
float64 autograd evaluation of the torch expression, Adam's arithmetic against the
float64 formula on the kernel's own gradient, the split of a run into calls and
launches bit for bit, masked rows, and the class on the reference's own run
(tests/golden/bc2.npz) under both backends."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_policy_fit import B1, B2, EPS, EXTRA, LR, STEP0, T, make_state, same_bits, shapes

pytestmark = pytest.mark.gpu
# (n, m, h0, h1, bs, weight_decay), seed 1 each: widths that are no multiples of 16, scalar and
# 16-byte row loads, two X chunks, m = 64 and m = 1, bs = 1, bs < 64 with padded rows, bs = 64.
# For all six, torch's own float32 CPU autograd of the same expression is within 2.5e-6 of
# float64 (asserted below from CPU evaluations alone; 1.2e-7 to 4.5e-7 for the seeds 1..6, but
# 5.8e-5 for seed 7 of the bs = 1 shape, which has a row whose action nearly equals the mean)
CASES = [
    (5, 3, 16, 8, 20, 1e-3),
    (39, 28, 64, 48, 33, 1e-3),
    (20, 5, 33, 17, 64, 0.0),
    (376, 17, 64, 64, 64, 0.0),
    (8, 64, 32, 32, 64, 0.0),
    (13, 1, 7, 64, 1, 0.0),
]
IDS = ["n%d-m%d-h%dx%d-bs%d" % c[:5] for c in CASES]
NAMES = ("W0", "b0", "W1", "b1", "W2", "b2")


def state(case):
    n, m, h0, h1, bs, wd = case
    return make_state(n, m, h0, h1, bs, "bc", wd, 1)


def mse_of(st, p, idx):
    """torch's MSELoss (mean reduction) over the [bs][m] tile of rows idx at the six
    tensors p (any dtype); an index outside [0, T) adds nothing, the divisor stays bs m."""
    rows = [int(i) for i in idx if 0 <= i < T]
    c = lambda a: torch.from_numpy(np.asarray(a)).to(p[0].dtype)   # noqa: E731
    x, act = c(st["obs"][rows]), c(st["act"][rows])
    h = (x - c(st["in_shift"])) / (c(st["in_scale"]) + 1e-8)
    h = torch.tanh(h @ p[0].T + p[1])
    h = torch.tanh(h @ p[2].T + p[3])
    mu = (h @ p[4].T + p[5]) * c(st["out_scale"]) + c(st["out_shift"])
    return torch.sum((mu - act) ** 2) / (st["bs"] * st["m"])


def f64_eval(st, idx):
    """Float64 autograd of the minibatch loss at the f32 parameters: the six gradients
    and the loss, with the condition on the inputs (see CASES) asserted on the way."""
    p = [torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in st["p"][:6]]
    loss = mse_of(st, p, idx)
    loss.backward()
    g64 = [q.grad.numpy() for q in p]
    p32 = [torch.from_numpy(a.copy()).requires_grad_() for a in st["p"][:6]]
    mse_of(st, p32, idx).backward()
    for name, q, b in zip(NAMES, p32, g64):
        rel = np.linalg.norm(q.grad.numpy().astype(np.float64) - b) / np.linalg.norm(b)
        print("input condition %s: torch float32 %.3g from float64" % (name, rel))
        assert rel <= 2.5e-6, "pick another seed: torch float32 %s %.3g from float64" % (name, rel)
    return g64, float(loss.detach())


class Net:
    """The six tensors' state on the device and mjrl_policy_mse_epoch calls over it.  adv,
    ll_old and old_log_std are valid device buffers full of NaN and kind is 77: finite,
    matching results show that the entry reads none of them."""

    def __init__(self, st):
        from mjrl_amd import _lib
        self.lib, self.st, dev = _lib, st, torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self.p, self.m, self.v = ([up(a) for a in st[k][:6]] for k in ("p", "m_", "v"))
        self.rows = {k: up(st[k]) for k in ("obs", "act", "in_shift", "in_scale", "out_shift", "out_scale")}
        self.nan_rows = torch.full((T + EXTRA,), float("nan"), device=dev)
        self.nan_cols = torch.full((st["m"],), float("nan"), device=dev)
        nf = C.c_int64()
        _lib.calls().mjrl_policy_fit_scratch(st["n"], st["m"], st["h0"], st["h1"], st["bs"], nf)
        self.scratch = torch.zeros(nf.value, dtype=torch.float32, device=dev)
        self.d = sum(int(np.prod(s)) for s in shapes(st["n"], st["m"], st["h0"], st["h1"])[:6])

    def epoch(self, idx, nmb, step0=STEP0, grads=False, spl=0):
        _lib, st, r = self.lib, self.st, self.rows
        net = _lib.MeanNet()
        for i in range(6):
            net.p[i], net.exp_avg[i], net.exp_avg_sq[i] = (t[i].data_ptr() for t in (self.p, self.m, self.v))
        ptr = lambda k: r[k].data_ptr()   # noqa: E731
        data = _lib.PolicyFitData(ptr("obs"), ptr("act"), self.nan_rows.data_ptr(), self.nan_rows.data_ptr(),
                                  self.nan_cols.data_ptr(), ptr("in_shift"), ptr("in_scale"), ptr("out_shift"),
                                  ptr("out_scale"), T, st["n"], st["m"], st["h0"], st["h1"], 77, float("nan"))
        hp = _lib.Adam(LR, B1, B2, EPS, st["wd"], step0)
        dev = self.scratch.device
        idx = torch.as_tensor(np.ascontiguousarray(idx), dtype=torch.int64).to(dev)
        assert idx.numel() >= nmb * st["bs"]
        g = torch.full((nmb, self.d), float("nan"), device=dev) if grads else None
        loss = torch.full((nmb,), float("nan"), device=dev) if grads else None
        with torch.cuda.device(dev):
            _lib.calls().mjrl_policy_mse_epoch(data, idx, nmb, st["bs"], net, hp, self.scratch, spl, g, loss,
                                               _lib.stream_ptr())
            torch.cuda.synchronize()
        return (g.cpu().numpy(), loss.cpu().numpy()) if grads else None

    def host(self):
        return [[t.cpu().numpy() for t in ts] for ts in (self.p, self.m, self.v)]


def split(flat, st):
    out, o = [], 0
    for s in shapes(st["n"], st["m"], st["h0"], st["h1"])[:6]:
        k = int(np.prod(s))
        out.append(flat[o:o + k].reshape(s))
        o += k
    assert o == flat.size
    return out


_ONE = {}


def one_step(case):
    """One step from the case's start state (computed once, shared, never changed):
    the kernel's gradient and loss, the state after it, and the float64 evaluation."""
    if case not in _ONE:
        st = state(case)
        net = Net(st)
        g, loss = net.epoch(st["perm"], 1, grads=True)
        _ONE[case] = dict(st=st, grad=split(g[0], st), loss=float(loss[0]), after=net.host(),
                          last=float(net.scratch[0].item()), ref=f64_eval(st, st["perm"][:st["bs"]]))
    return _ONE[case]


def assert_gradient(got, ref):
    for name, a, b in zip(NAMES, got, ref):
        rel = np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b)
        print("grad %s norm-relative %.3g" % (name, rel))
        assert rel <= 1e-5, (name, rel)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_and_loss_match_float64_autograd(case):
    r = one_step(case)
    ref_g, ref_loss = r["ref"]
    assert all(np.all(np.isfinite(g)) for g in r["grad"]) and np.isfinite(r["loss"])
    assert_gradient(r["grad"], ref_g)
    print("loss %.9g float64 %.9g" % (r["loss"], ref_loss))
    np.testing.assert_allclose(r["loss"], ref_loss, rtol=1e-5)
    assert r["last"] == r["loss"]   # scratch[0]: the last step's loss


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_adam_arithmetic_matches_the_float64_formula(case):
    """torch's single-tensor Adam in float64 on the kernel's own gradient, the six tensors."""
    r = one_step(case)
    st, t = r["st"], STEP0 + 1
    for i, name in enumerate(NAMES):
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


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_partition_into_calls_and_launches_changes_no_bit(case):
    st = state(case)
    bs = st["bs"]
    runs = []
    for mode in ("five", "ones", "spl2", "five"):
        net = Net(st)
        if mode == "ones":
            for k in range(5):
                net.epoch(st["perm"][k * bs:(k + 1) * bs], 1, step0=STEP0 + k)
        else:
            net.epoch(st["perm"], 5, spl=2 if mode == "spl2" else 0)
        runs.append(net.host())
    for other in runs[1:]:
        same_bits(runs[0], other)
    # and the steps did move every tensor, away from the one-step state too
    for k, key in enumerate(("p", "m_", "v")):
        for i in range(6):
            assert np.all(np.isfinite(runs[0][k][i]))
            assert not np.array_equal(runs[0][k][i], st[key][i])
            assert not np.array_equal(runs[0][k][i], one_step(case)["after"][k][i])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_out_of_range_are_masked(case):
    """A minibatch holding the indices T and -1: the gradient and loss of the other rows,
    still divided by bs m.  Rows T .. T + 7 of obs / act hold 1e30: a broken guard fails here.
    (bs = 1: its one row is masked, and gradient and loss are exactly zero.)"""
    st = state(case)
    bs = st["bs"]
    assert np.all(st["obs"][T:] == 1e30) and np.all(st["act"][T:] == 1e30)
    idx = st["perm"][bs:2 * bs].copy()
    idx[1 % bs], idx[(bs - 2) % bs] = T, -1
    g, loss = Net(st).epoch(idx, 1, grads=True)
    assert np.all(np.isfinite(g)) and np.isfinite(loss[0])
    if not any(0 <= i < T for i in idx):
        assert not np.any(g) and loss[0] == 0.0
        return
    ref_g, ref_loss = f64_eval(st, idx)
    assert_gradient(split(g[0], st), ref_g)
    np.testing.assert_allclose(float(loss[0]), ref_loss, rtol=1e-5)


# ---- the class ------------------------------------------------------------------------------
def _steps(opt, policy):
    return [float(opt.state[p]["step"]) for p in policy.model.parameters()]


def _run(backend, device, twice=False):
    from test_bc_mse import run_bc2
    bc, policy, z = run_bc2(device, backend)
    assert bc.fit_backend == backend
    m = policy.m
    ls = lambda: policy.get_param_values()[-m:].view(np.uint32)   # noqa: E731
    assert np.array_equal(ls(), z["after_init"][-m:].view(np.uint32))   # log_std: bit for bit, not trained
    first = (policy.get_param_values(), np.array(bc.logger.log["loss"], dtype=np.float64), _steps(bc.optimizer, policy))
    if twice:
        rs = np.random.RandomState(99)
        bc.expert_paths = [dict(observations=p["observations"] * 0.5 + rs.randn(*p["observations"].shape) * 0.1,
                                actions=p["actions"][::-1].copy()) for p in bc.expert_paths]
        np.random.seed(123)
        bc.train()
        assert np.array_equal(ls(), z["after_init"][-m:].view(np.uint32))
    assert len(bc.optimizer.state) == 6
    return bc, z, first, (policy.get_param_values(), np.array(bc.logger.log["loss"], dtype=np.float64),
                          _steps(bc.optimizer, policy))


_TORCH_GPU = []


def torch_gpu_run():
    if not _TORCH_GPU:
        _TORCH_GPU.append(_run("torch", "cuda:0"))
    return _TORCH_GPU[0]


def test_bc2_golden_run_with_the_hip_backend():
    """The reference's run with fit_backend = "hip", both backends against each other,
    and a second train() on new rows against the CPU-device run of the same sequence."""
    _, z, hip1, hip2 = _run("hip", "cuda:0", twice=True)
    _, _, tor1, _ = torch_gpu_run()
    _, _, _, cpu2 = _run("torch", "cpu", twice=True)
    ref = z["final"]
    print("BC MSE hip: parameters %.3g from the reference's, %.3g from the torch backend's (in norm)" % (
        np.linalg.norm(hip1[0] - ref) / np.linalg.norm(ref), np.linalg.norm(hip1[0] - tor1[0]) / np.linalg.norm(tor1[0])))
    np.testing.assert_allclose(hip1[1], z["loss"], rtol=1e-4)
    assert np.linalg.norm(hip1[0] - ref) <= 1e-3 * np.linalg.norm(ref)
    assert np.linalg.norm(hip1[0] - tor1[0]) <= 1e-3 * np.linalg.norm(tor1[0])
    assert hip1[2] == tor1[2] == [2 * int(300 / 32)] * 6
    np.testing.assert_allclose(hip2[1], cpu2[1], rtol=1e-4)
    assert np.linalg.norm(hip2[0] - cpu2[0]) <= 1e-3 * np.linalg.norm(cpu2[0])
    assert hip2[2] == cpu2[2] == [4 * int(300 / 32)] * 6


def test_bc2_golden_run_with_the_torch_backend():
    bc, z, tor1, _ = torch_gpu_run()
    ref = z["final"]
    print("BC MSE torch backend on the GPU: parameters %.3g from the reference's (in norm)" % (
        np.linalg.norm(tor1[0] - ref) / np.linalg.norm(ref)))
    np.testing.assert_allclose(tor1[1], z["loss"], rtol=1e-4)
    assert np.linalg.norm(tor1[0] - ref) <= 1e-3 * np.linalg.norm(ref)
    assert bc.trainer().graphable and bc.trainer().device.type == "cuda"
    assert bc.logger.log["epoch"] == [0, 1, 2]
