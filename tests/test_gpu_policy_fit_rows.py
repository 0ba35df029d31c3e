"""The row-tiled minibatch Adam steps of PPO and BC (csrc/policy_fit_rows.hip,
mjrl_policy_fit_rows_epoch; fit_backend = "hip_rows"): with one row tile the bits of
mjrl_policy_fit_epoch; with several, one step's gradient and loss against a float64 autograd
evaluation of the torch expression, masked rows across tiles, the split of a run into calls
bit for bit, Adam's arithmetic against the float64 formula on the kernel's own gradient, and
the classes against the torch backend and, at the reference's mb_size, against "hip".

The construction is tests/test_gpu_policy_fit.py's (its bounds too), restated where that file
fixes T = 200: minibatches above 200 rows draw from T = 2000 rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_policy_fit import (B1, B2, CLIP, EPS, LR, NAMES, RATIOS, STEP0, _run_ppo, _steps, assert_gradient,
                                 f64_policy, same_bits, shapes, split)

pytestmark = pytest.mark.gpu
EXTRA = 8


def rows_of(bs):
    return 200 if bs <= 200 else 2000


def make_state(n, m, h0, h1, bs, head, wd, seed):
    """test_gpu_policy_fit.make_state over T = rows_of(bs) rows (T + 8 in memory, the last eight
    holding 1e30), with permutations on end for six steps, and for bs > T one minibatch drawn
    with replacement."""
    T = rows_of(bs)
    rs = np.random.RandomState(100000 * seed + 1000 * n + 10 * m + bs)
    p, mo, v = [], [], []
    for s, fan_in in zip(shapes(n, m, h0, h1), (n, n, h0, h0, h1, h1, None)):
        if fan_in is None:
            p.append(rs.uniform(-1.0, 0.3, s).astype(np.float32))
        else:
            bound = 1.0 / np.sqrt(fan_in)
            p.append(rs.uniform(-bound, bound, s).astype(np.float32))
        mo.append((0.02 * rs.randn(*s)).astype(np.float32))
        v.append(rs.uniform(1e-5, 1e-3, s).astype(np.float32))
    st = dict(T=T, n=n, m=m, h0=h0, h1=h1, bs=bs, head=head, wd=wd, p=p, m_=mo, v=v)
    st["in_shift"] = (0.3 * rs.randn(n)).astype(np.float32)
    st["in_scale"] = rs.uniform(0.5, 2.0, n).astype(np.float32)
    st["out_shift"] = (0.2 * rs.randn(m)).astype(np.float32)
    st["out_scale"] = rs.uniform(0.5, 1.5, m).astype(np.float32)
    st["obs"] = (rs.randn(T + EXTRA, n) * st["in_scale"] + st["in_shift"]).astype(np.float32)
    st["act"] = np.zeros((T + EXTRA, m), np.float32)
    st["adv"] = rs.randn(T + EXTRA).astype(np.float32)
    p64 = [torch.from_numpy(a.astype(np.float64)) for a in p]
    c = lambda a: torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    h = (c(st["obs"][:T]) - c(st["in_shift"])) / (c(st["in_scale"]) + 1e-8)
    h = torch.tanh(h @ p64[0].T + p64[1])
    h = torch.tanh(h @ p64[2].T + p64[3])
    mu = ((h @ p64[4].T + p64[5]) * c(st["out_scale"]) + c(st["out_shift"])).numpy()
    st["act"][:T] = (mu + np.exp(p[6].astype(np.float64)) * rs.randn(T, m)).astype(np.float32)
    LL, _ = f64_policy(st, p64, np.arange(T))
    st["ll_old"] = np.zeros(T + EXTRA, np.float32)
    st["ll_old"][:T] = (LL.numpy() - np.log(rs.choice(RATIOS, T))).astype(np.float32)
    st["old_ls"] = (p[6].astype(np.float64) + rs.uniform(-0.25, 0.25, m) / np.sqrt(m)).astype(np.float32)
    for k in ("obs", "act", "adv", "ll_old"):
        st[k][T:] = 1e30
    if bs > T:
        st["perm"] = rs.randint(0, T, size=bs).astype(np.int64)   # with replacement: one step
    else:
        st["perm"] = np.concatenate([rs.permutation(T) for _ in range(max(2, -(-6 * bs // T)))]).astype(np.int64)
    return st


def loss_of(st, p, idx):
    """test_gpu_policy_fit.loss_of with the state's own T."""
    rows = [int(i) for i in idx if 0 <= i < st["T"]]
    dt = p[0].dtype
    aliased = st["head"] == "ppo-aliased"
    LL, LLa = f64_policy(st, p, rows, st["old_ls"] if aliased else None)
    if st["head"] == "bc":
        return -LL.sum() / st["bs"], None
    LLold = LLa if aliased else torch.from_numpy(st["ll_old"][rows]).to(dt)
    adv = torch.from_numpy(st["adv"][rows]).to(dt)
    ratio = torch.exp(LL - LLold)
    surr = torch.min(ratio * adv, torch.clamp(ratio, min=1 - CLIP, max=1 + CLIP) * adv)
    return -surr.sum() / st["bs"], (ratio.detach(), adv)


def f64_eval(st, idx):
    """test_gpu_policy_fit.f64_eval: float64 autograd of the minibatch loss at the f32
    parameters, with that file's conditions on the inputs asserted on the way."""
    p = [torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in st["p"]]
    loss, lr = loss_of(st, p, idx)
    loss.backward()
    g64 = [q.grad.numpy() if q.grad is not None else np.zeros(q.shape) for q in p]
    if lr is not None:
        ratio, adv = (t.numpy() for t in lr)
        clipped = ratio * adv > np.clip(ratio, 1 - CLIP, 1 + CLIP) * adv
        assert clipped.sum() >= 4 and (~clipped).sum() >= 4, "pick another seed: %d clipped of %d" % (
            clipped.sum(), clipped.size)
        edge = min(np.abs(ratio - (1 - CLIP)).min(), np.abs(ratio - (1 + CLIP)).min())
        assert edge > 1e-3, "pick another seed: a likelihood ratio %g from the clip range's edge" % edge
    # torch's own float32 CPU autograd of the same expression: a quarter of the bound below
    p32 = [torch.from_numpy(a.copy()).requires_grad_() for a in st["p"]]
    l32, _ = loss_of(st, p32, idx)
    l32.backward()
    for name, q, b in zip(NAMES, p32, g64):
        rel = np.linalg.norm(q.grad.numpy().astype(np.float64) - b) / np.linalg.norm(b)
        assert rel <= 2.5e-6, "pick another seed: torch float32 %s %.3g from float64" % (name, rel)
    return g64, float(loss.detach())


class Net:
    """The state on the device and calls of either entry point over it."""

    def __init__(self, st):
        from mjrl_amd import _lib
        self.lib, self.st, dev = _lib, st, torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self.p, self.m, self.v = ([up(a) for a in st[k]] for k in ("p", "m_", "v"))
        self.rows = {k: up(st[k]) for k in ("obs", "act", "adv", "ll_old", "old_ls", "in_shift", "in_scale",
                                            "out_shift", "out_scale")}
        self.dev, self.scratch = dev, {}
        self.d = sum(int(np.prod(s)) for s in shapes(st["n"], st["m"], st["h0"], st["h1"]))

    def epoch(self, idx, nmb, step0=STEP0, grads=False, narrow=False):
        """nmb steps of mjrl_policy_fit_rows_epoch (narrow: of mjrl_policy_fit_epoch); the scratch
        is poisoned with NaN before its first use: the slab needs no zero-fill."""
        _lib, st, r, dev = self.lib, self.st, self.rows, self.dev
        K = _lib.calls()
        if narrow not in self.scratch:
            nf = C.c_int64()
            (K.mjrl_policy_fit_scratch if narrow else K.mjrl_policy_fit_rows_scratch)(
                st["n"], st["m"], st["h0"], st["h1"], st["bs"], nf)
            self.scratch[narrow] = torch.full((nf.value,), float("nan"), dtype=torch.float32, device=dev)
        net = _lib.PolicyNet()
        for i in range(7):
            net.p[i], net.exp_avg[i], net.exp_avg_sq[i] = (t[i].data_ptr() for t in (self.p, self.m, self.v))
        head = st["head"]
        ptr = lambda k, on=True: r[k].data_ptr() if on else None   # noqa: E731
        data = _lib.PolicyFitData(ptr("obs"), ptr("act"), ptr("adv", head != "bc"), ptr("ll_old", head == "ppo"),
                                  ptr("old_ls", head == "ppo-aliased"), ptr("in_shift"), ptr("in_scale"),
                                  ptr("out_shift"), ptr("out_scale"), st["T"], st["n"], st["m"], st["h0"], st["h1"],
                                  _lib.POLICY_FIT_BC if head == "bc" else _lib.POLICY_FIT_PPO, CLIP)
        hp = _lib.Adam(LR, B1, B2, EPS, st["wd"], step0)
        idx = torch.as_tensor(np.ascontiguousarray(idx), dtype=torch.int64).to(dev)
        assert idx.numel() >= nmb * st["bs"]
        g = torch.full((nmb, self.d), float("nan"), device=dev) if grads else None
        loss = torch.full((nmb,), float("nan"), device=dev) if grads else None
        with torch.cuda.device(dev):
            if narrow:
                K.mjrl_policy_fit_epoch(data, idx, nmb, st["bs"], net, hp, self.scratch[narrow], 0, g, loss,
                                        _lib.stream_ptr())
            else:
                K.mjrl_policy_fit_rows_epoch(data, idx, nmb, st["bs"], net, hp, self.scratch[narrow], g, loss,
                                             _lib.stream_ptr())
            torch.cuda.synchronize()
        return (g.cpu().numpy(), loss.cpu().numpy()) if grads else None

    def host(self):
        return [[t.cpu().numpy() for t in ts] for ts in (self.p, self.m, self.v)]


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


# ---- 1: one tile carries k_pfit's bits ----------------------------------------------------------
# (n, m, h0, h1, bs, head, weight_decay, seed)
ONE_TILE = [
    (6, 2, 32, 32, 64, "ppo", 0.0, 1),
    (39, 28, 64, 48, 33, "ppo-aliased", 1e-3, 1),
    (5, 3, 16, 8, 20, "bc", 0.0, 1),
    (13, 1, 7, 64, 1, "bc", 0.0, 1),
]


def ids(cases):
    return ["n%d-m%d-h%dx%d-bs%d-%s" % c[:6] for c in cases]


@pytest.mark.parametrize("case", ONE_TILE, ids=ids(ONE_TILE))
def test_one_tile_carries_the_narrow_kernels_bits(case):
    st = make_state(*case)
    out = []
    for narrow in (False, True):
        net = Net(st)
        g, loss = net.epoch(st["perm"], 3, grads=True, narrow=narrow)
        out.append((net.host(), g, loss))
    (ha, ga, la), (hb, gb, lb) = out
    same_bits(ha, hb)
    assert np.all(np.isfinite(ga)) and np.all(np.isfinite(la))
    assert np.array_equal(bits(ga), bits(gb)) and np.array_equal(bits(la), bits(lb))
    for k, key in enumerate(("p", "m_", "v")):   # and the steps did move every tensor
        for i in range(7):
            assert not np.array_equal(ha[k][i], st[key][i])


# ---- 2: several tiles against float64 autograd --------------------------------------------------
# The seeds: for every PPO minibatch at least 4 clipped and 4 unclipped rows, no likelihood ratio
# within 1e-3 of 1 +- c, torch's own float32 CPU autograd within 2.5e-6 of float64 (asserted in
# f64_eval from the float64 evaluation alone); of the seeds 1..30 meeting them, the one whose
# float32 figure is smallest (the last case: see there)
TILED = [
    (6, 2, 32, 32, 65, "ppo", 0.0, 27),             # the second tile holds one row
    (6, 2, 32, 32, 65, "ppo-aliased", 0.0, 8),
    (20, 5, 33, 17, 130, "ppo", 0.0, 29),           # three tiles, odd widths
    (20, 5, 33, 17, 130, "ppo-aliased", 1e-3, 13),
    (20, 5, 33, 17, 130, "bc", 1e-3, 11),
    (376, 17, 64, 64, 256, "ppo", 0.0, 7),          # two X chunks
    (376, 17, 64, 64, 256, "ppo-aliased", 0.0, 30),
    (6, 2, 32, 32, 1024, "ppo", 0.0, 7),
    (6, 2, 32, 32, 1024, "ppo-aliased", 0.0, 25),
    # the cap, indices drawn with replacement.  Over 16384 rows torch's own float32 summation sits
    # close to the 2.5e-6 precondition whatever the seed (the sum's length, not the conditioning
    # of the problem), so this seed is the one of 1..30 that keeps the most margin
    (6, 2, 32, 32, 16384, "ppo", 0.0, 20),
]
_ONE = {}


def one_step(case):
    """One step from the case's start state (computed once, shared, never changed): the
    kernels' gradient and loss, the state after it, and the float64 evaluation."""
    if case not in _ONE:
        st = make_state(*case)
        net = Net(st)
        g, loss = net.epoch(st["perm"], 1, grads=True)
        _ONE[case] = dict(st=st, grad=split(g[0], st), loss=float(loss[0]), after=net.host(),
                          ref=f64_eval(st, st["perm"][:st["bs"]]))
    return _ONE[case]


@pytest.mark.parametrize("case", TILED, ids=ids(TILED))
def test_gradient_and_loss_match_float64_autograd(case):
    r = one_step(case)
    ref_g, ref_loss = r["ref"]
    assert_gradient(r["grad"], ref_g)
    print("loss %.9g float64 %.9g" % (r["loss"], ref_loss))
    np.testing.assert_allclose(r["loss"], ref_loss, rtol=1e-5)


# ---- 3: masking across tiles --------------------------------------------------------------------
MASKED = [c for c in TILED if c[4] == 130]


def masked_indices(st):
    """bs = 130: indices outside [0, T) scattered through tiles 0 and 1, tile 2 (rows 128, 129)
    wholly masked."""
    T = st["T"]
    idx = st["perm"][130:260].copy()
    for row, bad in ((0, T), (7, -1), (63, T + 3), (64, -(1 << 40)), (90, T + EXTRA), (127, 1 << 40), (128, T),
                     (129, -1)):
        idx[row] = bad
    return idx


@pytest.mark.parametrize("case", MASKED, ids=ids(MASKED))
def test_rows_out_of_range_are_masked_across_tiles(case):
    """The gradient of the other rows, still divided by 130.  Rows T .. T + 7 of every row array
    hold 1e30: a broken guard fails here."""
    st = make_state(*case)
    idx = masked_indices(st)
    net = Net(st)
    g, loss = net.epoch(idx, 1, grads=True)
    ref_g, ref_loss = f64_eval(st, idx)
    assert np.all(np.isfinite(g)) and np.isfinite(loss[0])
    assert all(np.all(np.isfinite(t)) for ts in net.host() for t in ts)
    assert_gradient(split(g[0], st), ref_g)
    np.testing.assert_allclose(float(loss[0]), ref_loss, rtol=1e-5)


# ---- 4: splits and repeats ----------------------------------------------------------------------
@pytest.mark.parametrize("case", MASKED, ids=ids(MASKED))
def test_partition_into_calls_and_repeats_change_no_bit(case):
    st = make_state(*case)
    bs = st["bs"]
    runs = []
    for mode in ("six", "two-four", "six"):
        net = Net(st)
        if mode == "six":
            g, loss = net.epoch(st["perm"], 6, grads=True)
        else:
            g1, l1 = net.epoch(st["perm"][:2 * bs], 2, grads=True)
            g2, l2 = net.epoch(st["perm"][2 * bs:6 * bs], 4, step0=STEP0 + 2, grads=True)
            g, loss = np.concatenate([g1, g2]), np.concatenate([l1, l2])
        runs.append((net.host(), g, loss))
    for h, g, loss in runs[1:]:
        same_bits(runs[0][0], h)
        assert np.array_equal(bits(runs[0][1]), bits(g)) and np.array_equal(bits(runs[0][2]), bits(loss))
    assert np.all(np.isfinite(runs[0][1])) and np.all(np.isfinite(runs[0][2]))
    # and the steps did move every tensor, away from the one-step state too
    for k, key in enumerate(("p", "m_", "v")):
        for i in range(7):
            assert not np.array_equal(runs[0][0][k][i], st[key][i])
            assert not np.array_equal(runs[0][0][k][i], one_step(case)["after"][k][i])


# ---- 5: Adam on the kernels' own gradient -------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in MASKED if c[6] > 0], ids=ids([c for c in MASKED if c[6] > 0]))
def test_adam_arithmetic_matches_the_float64_formula(case):
    """torch's single-tensor Adam in float64 on the folded gradient, all seven tensors, with
    weight decay (test_gpu_policy_fit.py's bounds)."""
    r = one_step(case)
    st, t = r["st"], STEP0 + 1
    assert st["wd"] > 0
    for i, name in enumerate(NAMES):
        p, m, v = (st[k][i].astype(np.float64) for k in ("p", "m_", "v"))
        g = r["grad"][i].astype(np.float64) + st["wd"] * p
        m1 = m + (g - m) * (1 - B1)
        v1 = B2 * v + (1 - B2) * g * g
        delta = (LR / (1 - B1 ** t)) * m1 / (np.sqrt(v1) / np.sqrt(1 - B2 ** t) + EPS)
        p1, gm, gv = (r["after"][k][i].astype(np.float64) for k in range(3))
        np.testing.assert_allclose(gm, m1, rtol=1e-6, atol=1e-37, err_msg=name)
        np.testing.assert_allclose(gv, v1, rtol=1e-6, atol=1e-37, err_msg=name)
        assert np.all(np.abs(p1 - (p - delta)) <= 2.0 ** -23 * np.abs(p) + 2e-6 * np.abs(delta)), name


# ---- 6: the classes -----------------------------------------------------------------------------
def _policy():
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    return MLP(EnvSpec(6, 2, 500, 1), hidden_sizes=(32, 32), seed=3, init_log_std=-0.5)


def _paths(seed, rewards=True):
    rs = np.random.RandomState(seed)
    paths = [dict(observations=rs.randn(500, 6), actions=0.6 * rs.randn(500, 2)) for _ in range(8)]
    if rewards:
        for p in paths:
            p.update(rewards=rs.randn(500), advantages=rs.randn(500))
    return paths


def _ppo_run(backend):
    from mjrl_amd.algos.ppo_clip import PPO
    policy = _policy()
    ppo = PPO(None, policy, None, clip_coef=0.2, epochs=2, mb_size=256, learn_rate=3e-3)
    ppo.fit_backend = backend
    out = []
    for it in range(2):
        assert ppo._aliasing() == ([False] * 7 if it == 0 else [True] * 6 + [False])   # the second: aliased
        np.random.seed(40 + it)
        ppo.train_from_paths(_paths(10 + it))
        out.append((policy.get_param_values(), _steps(ppo.optimizer, policy)))
    return out


def test_ppo_with_the_rows_backend_matches_the_torch_backend():
    rows, tor = _ppo_run("hip_rows"), _ppo_run("torch")
    init = _policy().get_param_values()
    for it in range(2):
        (a, sa), (b, sb) = rows[it], tor[it]
        rel = np.linalg.norm(a - b) / np.linalg.norm(b)
        print("PPO call %d hip_rows: parameters %.3g from the torch backend's (in norm)" % (it, rel))
        assert np.all(np.isfinite(a)) and rel <= 1e-3, it
        assert sa == sb and sa[0] == 2 * (4000 // 256) * (it + 1)
        assert np.linalg.norm(b - init) > 1e-2 * np.linalg.norm(init)   # the steps moved the policy


def _bc_run(backend):
    from mjrl_amd.algos.behavior_cloning import BC
    policy = _policy()
    bc = BC(_paths(20, rewards=False), policy, epochs=2, batch_size=256, lr=1e-3, device="cuda:0")
    bc.fit_backend = backend
    np.random.seed(50)
    bc.train()
    return policy.get_param_values(), np.array(bc.logger.log["loss"], dtype=np.float64), _steps(bc.optimizer, policy)


def test_bc_with_the_rows_backend_matches_the_torch_backend():
    (a, la, sa), (b, lb, sb) = _bc_run("hip_rows"), _bc_run("torch")
    rel = np.linalg.norm(a - b) / np.linalg.norm(b)
    print("BC hip_rows: parameters %.3g from the torch backend's (in norm)" % rel)
    assert np.all(np.isfinite(a)) and rel <= 1e-3
    np.testing.assert_allclose(la, lb, rtol=1e-4)
    assert sa == sb and sa[0] == 2 * (4000 // 256)


def test_ppo_golden_run_at_the_reference_mb_size_leaves_the_hip_backends_bits():
    """tests/golden/ppo.npz at mb_size = 64 (the second iteration is the aliased form): one row
    tile, so "hip_rows" leaves "hip"'s parameters bit for bit."""
    _, rows = _run_ppo("hip_rows")
    _, hip = _run_ppo("hip")
    for it in range(2):
        assert rows[it]["params"].dtype == hip[it]["params"].dtype
        assert np.array_equal(rows[it]["params"], hip[it]["params"]), it
        assert rows[it]["steps"] == hip[it]["steps"] and rows[it]["steps"][0] > 0
        assert rows[it]["kl"] == hip[it]["kl"] and rows[it]["surr"] == hip[it]["surr"]
