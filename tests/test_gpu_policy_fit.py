"""The fused minibatch Adam steps of PPO and BC on the Gaussian MLP policy
(csrc/policy_fit.hip, mjrl_policy_fit_epoch; fit_backend = "hip"): one step's
gradient and loss against a float64 autograd evaluation of the torch expression,
Adam's arithmetic against the float64 formula on the kernel's own gradient, the
split of a run into calls and launches bit for bit, masked rows, and the classes
on the reference's own runs (tests/golden/bc.npz, ppo.npz) against the torch
backend."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T, EXTRA = 200, 8
LR, B1, B2, EPS, STEP0, CLIP = 1e-3, 0.9, 0.999, 1e-8, 5, 0.2
RATIOS = (0.55, 0.7, 0.9, 0.97, 1.03, 1.1, 1.3, 1.6)
# (n, m, h0, h1, bs, head, weight_decay, seed).  The seeds are ones for which every PPO
# minibatch tested holds at least 4 clipped and 4 unclipped rows, no likelihood ratio lies
# within 1e-3 of 1 +- c, and torch's own float32 CPU autograd of the same expression is within
# 2.5e-6 of float64 (all asserted below from the float64 evaluation alone; of the seeds 1..30
# meeting them, the one whose float32 figure is smallest: it moves a little from CPU to CPU)
CASES = [
    (6, 2, 32, 32, 64, "ppo", 0.0, 28),
    (6, 2, 32, 32, 64, "ppo-aliased", 0.0, 15),
    (5, 3, 16, 8, 20, "bc", 1e-3, 20),
    (39, 28, 64, 48, 33, "ppo-aliased", 1e-3, 11),
    (20, 5, 33, 17, 64, "ppo", 0.0, 25),
    (376, 17, 64, 64, 64, "ppo", 0.0, 10),
    (376, 17, 64, 64, 64, "ppo-aliased", 0.0, 18),
    (8, 64, 32, 32, 64, "bc", 0.0, 2),
    (13, 1, 7, 64, 1, "bc", 0.0, 3),
]
IDS = ["n%d-m%d-h%dx%d-bs%d-%s" % c[:6] for c in CASES]
NAMES = ("W0", "b0", "W1", "b1", "W2", "b2", "log_std")


def shapes(n, m, h0, h1):
    return [(h0, n), (h0,), (h1, h0), (h1,), (m, h1), (m,), (m,)]


def f64_policy(st, p, rows, old_ls=None):
    """The torch expression of DeviceTrainer.mean / log_likelihood in the dtype of p."""
    dt = p[0].dtype
    c = lambda a: torch.from_numpy(np.asarray(a)).to(dt)   # noqa: E731
    x, act = c(st["obs"][rows]), c(st["act"][rows])
    h = (x - c(st["in_shift"])) / (c(st["in_scale"]) + 1e-8)
    h = torch.tanh(h @ p[0].T + p[1])
    h = torch.tanh(h @ p[2].T + p[3])
    mu = (h @ p[4].T + p[5]) * c(st["out_scale"]) + c(st["out_shift"])
    m = p[6].shape[0]
    ll = lambda mean, ls: (-0.5 * torch.sum(((act - mean) / torch.exp(ls)) ** 2, dim=1)   # noqa: E731
                           + -torch.sum(ls) + -0.5 * m * float(np.log(2 * np.pi)))
    LL = ll(mu, p[6])
    return LL, (ll(mu.detach(), c(old_ls)) if old_ls is not None else None)


def make_state(n, m, h0, h1, bs, head, wd, seed):
    """A start state that is not fresh, on the host: f32 parameters (torch's Linear
    init ranges, log_std in [-1, 0.3]), random non-zero exp_avg, positive exp_avg_sq,
    non-identity transformations, T + 8 rows of every row array whose last eight hold
    1e30 (the kernel is told T), actions around the float64 mean, ll_old the float64
    LL minus the log of a ratio drawn from RATIOS, and two permutations on end."""
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
    st = dict(n=n, m=m, h0=h0, h1=h1, bs=bs, head=head, wd=wd, p=p, m_=mo, v=v)
    st["in_shift"] = (0.3 * rs.randn(n)).astype(np.float32)
    st["in_scale"] = rs.uniform(0.5, 2.0, n).astype(np.float32)
    st["out_shift"] = (0.2 * rs.randn(m)).astype(np.float32)
    st["out_scale"] = rs.uniform(0.5, 1.5, m).astype(np.float32)
    st["obs"] = (rs.randn(T + EXTRA, n) * st["in_scale"] + st["in_shift"]).astype(np.float32)
    st["act"] = np.zeros((T + EXTRA, m), np.float32)
    st["adv"] = rs.randn(T + EXTRA).astype(np.float32)
    p64 = [torch.from_numpy(a.astype(np.float64)) for a in p]
    allrows = np.arange(T)
    c = lambda a: torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    h = (c(st["obs"][:T]) - c(st["in_shift"])) / (c(st["in_scale"]) + 1e-8)
    h = torch.tanh(h @ p64[0].T + p64[1])
    h = torch.tanh(h @ p64[2].T + p64[3])
    mu = ((h @ p64[4].T + p64[5]) * c(st["out_scale"]) + c(st["out_shift"])).numpy()
    st["act"][:T] = (mu + np.exp(p[6].astype(np.float64)) * rs.randn(T, m)).astype(np.float32)
    LL, _ = f64_policy(st, p64, allrows)
    st["ll_old"] = np.zeros(T + EXTRA, np.float32)
    st["ll_old"][:T] = (LL.numpy() - np.log(rs.choice(RATIOS, T))).astype(np.float32)
    st["old_ls"] = (p[6].astype(np.float64) + rs.uniform(-0.25, 0.25, m) / np.sqrt(m)).astype(np.float32)
    for k in ("obs", "act", "adv", "ll_old"):
        st[k][T:] = 1e30
    st["perm"] = np.concatenate([rs.permutation(T), rs.permutation(T)]).astype(np.int64)
    return st


def loss_of(st, p, idx):
    """The minibatch loss of rows idx at parameters p (any dtype); an index outside
    [0, T) adds nothing, the mean still divides by bs.  Returns (loss, LR or None)."""
    rows = [int(i) for i in idx if 0 <= i < T]
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
    """Float64 autograd of the minibatch loss at the f32 parameters: gradients and
    loss, with the conditions on the inputs (see CASES) asserted on the way."""
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
    if l32.requires_grad and any(0 <= i < T for i in idx):
        l32.backward()
        for name, q, b in zip(NAMES, p32, g64):
            rel = np.linalg.norm(q.grad.numpy().astype(np.float64) - b) / np.linalg.norm(b)
            assert rel <= 2.5e-6, "pick another seed: torch float32 %s %.3g from float64" % (name, rel)
    return g64, float(loss.detach())


class Net:
    """The state on the device and mjrl_policy_fit_epoch calls over it."""

    def __init__(self, st):
        from mjrl_amd import _lib
        self.lib, self.st, dev = _lib, st, torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self.p, self.m, self.v = ([up(a) for a in st[k]] for k in ("p", "m_", "v"))
        self.rows = {k: up(st[k]) for k in ("obs", "act", "adv", "ll_old", "old_ls", "in_shift", "in_scale",
                                            "out_shift", "out_scale")}
        nf = C.c_int64()
        _lib.calls().mjrl_policy_fit_scratch(st["n"], st["m"], st["h0"], st["h1"], st["bs"], nf)
        self.scratch = torch.zeros(nf.value, dtype=torch.float32, device=dev)
        self.d = sum(int(np.prod(s)) for s in shapes(st["n"], st["m"], st["h0"], st["h1"]))

    def epoch(self, idx, nmb, step0=STEP0, grads=False, spl=0):
        _lib, st, r = self.lib, self.st, self.rows
        net = _lib.PolicyNet()
        for i in range(7):
            net.p[i], net.exp_avg[i], net.exp_avg_sq[i] = (t[i].data_ptr() for t in (self.p, self.m, self.v))
        head = st["head"]
        ptr = lambda k, on=True: r[k].data_ptr() if on else None   # noqa: E731
        data = _lib.PolicyFitData(ptr("obs"), ptr("act"), ptr("adv", head != "bc"), ptr("ll_old", head == "ppo"),
                                  ptr("old_ls", head == "ppo-aliased"), ptr("in_shift"), ptr("in_scale"),
                                  ptr("out_shift"), ptr("out_scale"), T, st["n"], st["m"], st["h0"], st["h1"],
                                  _lib.POLICY_FIT_BC if head == "bc" else _lib.POLICY_FIT_PPO, CLIP)
        hp = _lib.Adam(LR, B1, B2, EPS, st["wd"], step0)
        dev = self.scratch.device
        idx = torch.as_tensor(np.ascontiguousarray(idx), dtype=torch.int64).to(dev)
        assert idx.numel() >= nmb * st["bs"]
        g = torch.full((nmb, self.d), float("nan"), device=dev) if grads else None
        loss = torch.full((nmb,), float("nan"), device=dev) if grads else None
        with torch.cuda.device(dev):
            _lib.calls().mjrl_policy_fit_epoch(data, idx, nmb, st["bs"], net, hp, self.scratch, spl, g, loss,
                                               _lib.stream_ptr())
            torch.cuda.synchronize()
        return (g.cpu().numpy(), loss.cpu().numpy()) if grads else None

    def host(self):
        return [[t.cpu().numpy() for t in ts] for ts in (self.p, self.m, self.v)]


def split(flat, st):
    out, o = [], 0
    for s in shapes(st["n"], st["m"], st["h0"], st["h1"]):
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
        st = make_state(*case)
        net = Net(st)
        g, loss = net.epoch(st["perm"], 1, grads=True)
        _ONE[case] = dict(st=st, grad=split(g[0], st), loss=float(loss[0]), after=net.host(),
                          ref=f64_eval(st, st["perm"][:st["bs"]]))
    return _ONE[case]


def assert_gradient(got, ref):
    for name, a, b in zip(NAMES, got, ref):
        if np.linalg.norm(b) == 0.0:   # every row masked
            assert not np.any(a), name
            continue
        rel = np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b)
        print("grad %s norm-relative %.3g" % (name, rel))
        assert rel <= 1e-5, (name, rel)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_and_loss_match_float64_autograd(case):
    r = one_step(case)
    ref_g, ref_loss = r["ref"]
    assert_gradient(r["grad"], ref_g)
    print("loss %.9g float64 %.9g" % (r["loss"], ref_loss))
    np.testing.assert_allclose(r["loss"], ref_loss, rtol=1e-5)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_adam_arithmetic_matches_the_float64_formula(case):
    """torch's single-tensor Adam in float64 on the kernel's own gradient, all seven tensors."""
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


def same_bits(a, b):
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            assert s.dtype == t.dtype == np.float32 and np.array_equal(s.view(np.uint32), t.view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_partition_into_calls_and_launches_changes_no_bit(case):
    st = make_state(*case)
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
        for i in range(7):
            assert not np.array_equal(runs[0][k][i], st[key][i])
            assert not np.array_equal(runs[0][k][i], one_step(case)["after"][k][i])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_out_of_range_are_masked(case):
    """A minibatch holding the indices T and -1: the gradient of the other rows, still
    divided by bs.  Rows T .. T + 7 of every row array hold 1e30: a broken guard fails here."""
    st = make_state(*case)
    bs = st["bs"]
    idx = st["perm"][bs:2 * bs].copy()
    idx[1 % bs], idx[(bs - 2) % bs] = T, -1
    g, loss = Net(st).epoch(idx, 1, grads=True)
    ref_g, ref_loss = f64_eval(st, idx)
    assert np.all(np.isfinite(g)) and np.isfinite(loss[0])
    assert_gradient(split(g[0], st), ref_g)
    np.testing.assert_allclose(float(loss[0]), ref_loss, rtol=1e-5, atol=0 if ref_loss else 1e-30)


# ---- the classes ----------------------------------------------------------------------------
def _steps(opt, policy):
    return [float(opt.state[p]["step"]) for p in policy.trainable_params]


def _run_bc(backend, device, monkeypatch, twice=False):
    from mjrl_amd.algos.behavior_cloning import BC
    from test_bc_ppo import run_bc
    monkeypatch.setattr(BC, "fit_backend", backend)
    bc, policy, z = run_bc(device)
    assert bc.fit_backend == backend
    first = (policy.get_param_values(), np.array(bc.logger.log["loss"], dtype=np.float64), _steps(bc.optimizer, policy))
    if twice:
        rs = np.random.RandomState(99)
        bc.expert_paths = [dict(observations=p["observations"] * 0.5 + rs.randn(*p["observations"].shape) * 0.1,
                                actions=p["actions"][::-1].copy()) for p in bc.expert_paths]
        np.random.seed(123)
        bc.train()
    return z, first, (policy.get_param_values(), np.array(bc.logger.log["loss"], dtype=np.float64),
                      _steps(bc.optimizer, policy))


def test_bc_golden_run_with_the_hip_backend(monkeypatch):
    """test_gpu_api.py::test_bc_on_gpu_matches_reference's assertions with
    fit_backend = "hip", both backends against each other, and a second train() on
    new rows against the CPU-device run (test_bc_train_twice_on_gpu_matches_cpu)."""
    z, hip1, hip2 = _run_bc("hip", "cuda:0", monkeypatch, twice=True)
    _, tor1, _ = _run_bc("torch", "cuda:0", monkeypatch)
    _, _, cpu2 = _run_bc("torch", "cpu", monkeypatch, twice=True)
    ref = z["final"]
    print("BC hip: parameters %.3g from the reference's, %.3g from the torch backend's (in norm)" % (
        np.linalg.norm(hip1[0] - ref) / np.linalg.norm(ref), np.linalg.norm(hip1[0] - tor1[0]) / np.linalg.norm(tor1[0])))
    np.testing.assert_allclose(hip1[1], z["loss"], rtol=1e-4)
    assert np.linalg.norm(hip1[0] - ref) <= 1e-3 * np.linalg.norm(ref)
    assert np.linalg.norm(hip1[0] - tor1[0]) <= 1e-3 * np.linalg.norm(tor1[0])
    assert hip1[2] == tor1[2] and hip1[2][0] > 0
    np.testing.assert_allclose(hip2[1], cpu2[1], rtol=1e-4)
    assert np.linalg.norm(hip2[0] - cpu2[0]) <= 1e-3 * np.linalg.norm(cpu2[0])
    assert hip2[2] == cpu2[2]


def _run_ppo(backend):
    from mjrl_amd.algos.ppo_clip import PPO
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    z = np.load(os.path.join(GOLD, "ppo.npz"))
    policy = MLP(EnvSpec(6, 2, 200, 1), hidden_sizes=(32, 32), seed=3, init_log_std=-0.5)
    np.testing.assert_array_equal(policy.get_param_values(), z["init"])
    ppo = PPO(None, policy, None, clip_coef=0.2, epochs=2, mb_size=64, learn_rate=3e-3, save_logs=True)
    ppo.fit_backend = backend
    offs = np.concatenate([[0], np.cumsum(z["lengths"])])
    out = []
    for it in range(2):
        sl = lambda k: [z["%s%d" % (k, it)][offs[i]:offs[i + 1]] for i in range(len(z["lengths"]))]   # noqa: E731
        paths = [dict(observations=o, actions=a, rewards=r, advantages=v)
                 for o, a, r, v in zip(sl("obs"), sl("act"), sl("rew"), sl("adv"))]
        assert ppo._aliasing() == ([False] * 7 if it == 0 else [True] * 6 + [False])
        np.random.seed(int(z["np_seed%d" % it]))
        stats = ppo.train_from_paths(paths)
        out.append(dict(stats=stats, params=policy.get_param_values(), kl=ppo.logger.log["kl_dist"][-1],
                        surr=ppo.logger.log["surr_improvement"][-1], score=ppo.logger.log["running_score"][-1],
                        steps=_steps(ppo.optimizer, policy)))
    return z, out


def test_ppo_golden_run_with_the_hip_backend():
    """test_gpu_api.py::test_ppo_on_gpu_matches_reference's assertions with
    fit_backend = "hip" (the second iteration is the aliased form), and both
    backends against each other."""
    z, hip = _run_ppo("hip")
    _, tor = _run_ppo("torch")
    for it in range(2):
        h, t = hip[it], tor[it]
        np.testing.assert_allclose(h["stats"], z["base_stats%d" % it], rtol=1e-12)
        ref = z["params%d" % it]
        print("PPO iteration %d hip: parameters %.3g from the reference's, %.3g from the torch backend's" % (
            it, np.linalg.norm(h["params"] - ref) / np.linalg.norm(ref),
            np.linalg.norm(h["params"] - t["params"]) / np.linalg.norm(t["params"])))
        assert np.linalg.norm(h["params"] - ref) <= 1e-3 * np.linalg.norm(ref), it
        assert abs(h["kl"] - z["kl_dist%d" % it]) <= 0.05 * abs(z["kl_dist%d" % it]) + 1e-6
        assert abs(h["surr"] - z["surr_improvement%d" % it]) <= 0.05 * abs(z["surr_improvement%d" % it]) + 1e-5, it
        np.testing.assert_allclose(h["score"], z["running_score%d" % it], rtol=1e-12)
        assert np.linalg.norm(h["params"] - t["params"]) <= 1e-3 * np.linalg.norm(t["params"]), it
        assert h["steps"] == t["steps"] and h["steps"][0] > 0


def test_refusals_on_the_gpu():
    """Every refusal of the classes raises its ValueError with a GPU present too."""
    from mjrl_amd.comm import LocalComm
    from test_policy_fit import _ppo_paths, bc_refusals, ppo_refusals
    for name, make, backend, match in bc_refusals():
        bc = make()
        bc.fit_backend = backend
        with pytest.raises(ValueError, match=match):
            bc.train()
    for name, make, backend, match in ppo_refusals():
        agent = make()
        agent.fit_backend = backend
        agent._comm = LocalComm()
        with pytest.raises(ValueError, match=match):
            agent.train_from_paths(_ppo_paths())
