"""The fused minibatch Adam steps of MLPBaseline's value fit (csrc/value_fit.hip,
mjrl_value_mlp_epoch; fit_backend = "hip"): one step's gradient and loss against
a float64 autograd evaluation, Adam's arithmetic against the float64 formula on
the kernel's own gradient, the step counter / fused update + forward plumbing
bit for bit, masked rows, the reference's own fit (tests/golden/mlp_baseline.npz)
and train_step on the streamed-staging route against the torch backend."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
T, EXTRA, H = 200, 8, 128
LR, B1, B2, EPS, STEP0 = 1e-3, 0.9, 0.999, 1e-8, 5
# (n, bs, weight_decay, seed): F = n + 4 = 7, 16, 9, 380; the seeds are ones for which no
# hidden pre-activation of the tested minibatches lies within 1e-5 of the ReLU kink
# (asserted below from the float64 evaluation alone)
CASES = [(3, 64, 1e-3, 1), (12, 64, 0.0, 8), (5, 20, 1e-3, 1), (376, 64, 0.0, 8), (376, 33, 1e-3, 2)]
IDS = ["n%d-bs%d" % (c[0], c[1]) for c in CASES]
NAMES = ("W0", "b0", "W1", "b1", "W2", "b2")


def shapes(n):
    F = n + 4
    return [(H, F), (H,), (H, H), (H,), (1, H), (1,)]


def make_state(n, bs, wd, seed):
    """A start state that is not fresh, on the host: f32 parameters (torch's Linear
    init ranges), random non-zero exp_avg, positive exp_avg_sq, T + 8 rows of X / Y
    whose last eight hold 1e30 (the kernels are told T), and two permutations on end
    (five minibatches of 64 rows)."""
    rs = np.random.RandomState(1000 * n + bs + 7919 * seed)
    p, m, v = [], [], []
    for s, fan_in in zip(shapes(n), (n + 4, n + 4, H, H, H, H)):
        bound = 1.0 / np.sqrt(fan_in)
        p.append(rs.uniform(-bound, bound, s).astype(np.float32))
        m.append((0.02 * rs.randn(*s)).astype(np.float32))
        v.append(rs.uniform(1e-5, 1e-3, s).astype(np.float32))
    X = rs.randn(T + EXTRA, n + 4).astype(np.float32)
    Y = rs.randn(T + EXTRA).astype(np.float32)
    X[T:], Y[T:] = 1e30, 1e30
    perm = np.concatenate([rs.permutation(T), rs.permutation(T)]).astype(np.int64)
    return dict(n=n, bs=bs, wd=wd, p=p, m=m, v=v, X=X, Y=Y, perm=perm)


def f64_eval(st, idx):
    """Float64 autograd of the minibatch MSE (rows idx; an index outside [0, T) adds
    nothing, the mean still divides by bs) at the f32 parameters: gradients, loss
    and the smallest |hidden pre-activation| of the rows that count."""
    p = [torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in st["p"]]
    rows = [int(i) for i in idx if 0 <= i < T]
    x = torch.from_numpy(st["X"][rows].astype(np.float64))
    y = torch.from_numpy(st["Y"][rows].astype(np.float64))
    pre0 = x @ p[0].T + p[1]
    pre1 = torch.relu(pre0) @ p[2].T + p[3]
    out = (torch.relu(pre1) @ p[4].T + p[5]).reshape(-1)
    loss = ((out - y) ** 2).sum() / st["bs"]
    loss.backward()
    kink = min(float(pre0.detach().abs().min()), float(pre1.detach().abs().min()))
    return [q.grad.numpy() for q in p], float(loss.detach()), kink


class Net:
    """The state on the device and one mjrl_value_mlp_epoch call over it."""

    def __init__(self, st):
        from mjrl_amd import _lib
        self.lib, self.st, dev = _lib, st, torch.device("cuda:0")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self.p, self.m, self.v = ([up(a) for a in st[k]] for k in "pmv")
        self.X, self.Y = up(st["X"]), up(st["Y"])
        nf = C.c_int64()
        _lib.calls().mjrl_value_mlp_scratch(st["n"], st["bs"], nf)
        self.scratch = torch.zeros(nf.value, dtype=torch.float32, device=dev)
        self.d = sum(int(np.prod(s)) for s in shapes(st["n"]))

    def epoch(self, perm, nmb, step0=STEP0, grads=False):
        _lib, st = self.lib, self.st
        net = _lib.ValueNet()
        for i in range(6):
            net.p[i], net.exp_avg[i], net.exp_avg_sq[i] = (t[i].data_ptr() for t in (self.p, self.m, self.v))
        hp = _lib.Adam(LR, B1, B2, EPS, st["wd"], step0)
        dev = self.X.device
        perm = torch.as_tensor(perm, dtype=torch.int64).to(dev)
        g = torch.full((nmb, self.d), float("nan"), device=dev) if grads else None
        loss = torch.full((nmb,), float("nan"), device=dev) if grads else None
        with torch.cuda.device(dev):
            _lib.calls().mjrl_value_mlp_epoch(self.X, self.Y, T, st["n"], perm, nmb, st["bs"], net, hp, self.scratch,
                                              g, loss, _lib.stream_ptr())
            torch.cuda.synchronize()
        return (g.cpu().numpy(), loss.cpu().numpy()) if grads else None

    def host(self):
        return [[t.cpu().numpy() for t in ts] for ts in (self.p, self.m, self.v)]


def split(flat, n):
    out, o = [], 0
    for s in shapes(n):
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
        n, bs, wd, seed = case
        st = make_state(n, bs, wd, seed)
        net = Net(st)
        g, loss = net.epoch(st["perm"], 1, grads=True)
        _ONE[case] = dict(st=st, grad=split(g[0], n), loss=float(loss[0]), after=net.host(),
                          ref=f64_eval(st, st["perm"][:bs]))
    return _ONE[case]


def assert_gradient(got, ref, kink):
    assert kink > 1e-5, "a hidden unit within rounding of its kink (%g): pick another seed" % kink
    for name, a, b in zip(NAMES, got, ref):
        rel = np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b)
        print("grad %s norm-relative %.3g" % (name, rel))
        assert rel <= 1e-5, (name, rel)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_and_loss_match_float64_autograd(case):
    r = one_step(case)
    ref_g, ref_loss, kink = r["ref"]
    assert_gradient(r["grad"], ref_g, kink)
    print("loss %.9g float64 %.9g" % (r["loss"], ref_loss))
    np.testing.assert_allclose(r["loss"], ref_loss, rtol=1e-5)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_adam_arithmetic_matches_the_float64_formula(case):
    """torch's single-tensor Adam in float64 on the kernel's own gradient."""
    r = one_step(case)
    st, t = r["st"], STEP0 + 1
    for i, name in enumerate(NAMES):
        p, m, v = (st[k][i].astype(np.float64) for k in "pmv")
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
def test_one_call_of_five_steps_equals_five_calls_and_repeats(case):
    n, bs, wd, seed = case
    st = make_state(n, bs, wd, seed)
    runs = []
    for mode in ("five", "ones", "five"):
        net = Net(st)
        if mode == "five":
            net.epoch(st["perm"], 5)
        else:
            for k in range(5):
                net.epoch(st["perm"][k * bs:(k + 1) * bs], 1, step0=STEP0 + k)
        runs.append(net.host())
    same_bits(runs[0], runs[1])
    same_bits(runs[0], runs[2])
    # and the steps did move every tensor, away from the one-step state too
    for i in range(6):
        assert not np.array_equal(runs[0][0][i], st["p"][i])
        assert not np.array_equal(runs[0][0][i], one_step(case)["after"][0][i])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_out_of_range_are_masked(case):
    """A minibatch holding the indices T and -1: the gradient of the other rows, still
    divided by bs.  Rows T .. T + 7 of X / Y hold 1e30: a broken guard fails here."""
    n, bs, wd, seed = case
    st = make_state(n, bs, wd, seed)
    idx = st["perm"][bs:2 * bs].copy()
    idx[1], idx[bs - 2] = T, -1
    g, loss = Net(st).epoch(idx, 1, grads=True)
    ref_g, ref_loss, kink = f64_eval(st, idx)
    assert np.all(np.isfinite(g))
    assert_gradient(split(g[0], n), ref_g, kink)
    np.testing.assert_allclose(float(loss[0]), ref_loss, rtol=1e-5)


# ---- the class ----------------------------------------------------------------------------
def _golden_fit(backend):
    from mjrl_amd.baselines.mlp_baseline import MLPBaseline
    from mjrl_amd.utils.gym_env import EnvSpec
    z = np.load(os.path.join(GOLD, "mlp_baseline.npz"))
    offs = np.concatenate([[0], np.cumsum(z["lengths"])])
    paths = [dict(observations=z["obs"][offs[i]:offs[i + 1]], rewards=z["rewards"][offs[i]:offs[i + 1]],
                  returns=z["returns"][offs[i]:offs[i + 1]]) for i in range(len(z["lengths"]))]
    torch.manual_seed(7)
    b = MLPBaseline(EnvSpec(5, 2, 300, 1), batch_size=64, epochs=2, learn_rate=3e-3)
    b.fit_backend = backend
    errs, preds = [], []
    for it in range(2):
        np.random.seed(int(z["np_seed%d" % it]))
        errs.append(b.fit(paths, return_errors=True))
        preds.append(np.concatenate([b.predict(p) for p in paths]))
    return z, paths, b, errs, preds


def test_golden_fit_with_the_hip_backend_matches_the_reference():
    """test_gpu_api.py::test_mlp_baseline_fit_matches_reference's assertions with
    fit_backend = "hip", and both backends against each other."""
    z, paths, b, errs, preds = _golden_fit("hip")
    _, _, bt, _, preds_t = _golden_fit("torch")
    for it in range(2):
        for name, pr in (("hip", preds[it]), ("torch", preds_t[it])):
            print("fit %d %s: predictions %.3g from the reference's (max relative)" % (
                it, name, np.max(np.abs(pr - z["pred%d" % it]) / np.abs(z["pred%d" % it]))))
        np.testing.assert_allclose(errs[it], z["err%d" % it], rtol=1e-4)
        np.testing.assert_allclose(preds[it], z["pred%d" % it], rtol=1e-3, atol=1e-4)
    for k, v in b.model.state_dict().items():
        ref = z["final_" + k.replace(".", "_")]
        print("%s: %.3g in norm from the reference's" % (k, np.linalg.norm(v.numpy() - ref) / np.linalg.norm(ref)))
        assert np.linalg.norm(v.numpy() - ref) <= 1e-3 * np.linalg.norm(ref), k
    clone = pickle.loads(pickle.dumps(b))
    assert clone.fit_backend == "hip"
    np.testing.assert_allclose(np.concatenate([clone.predict(p) for p in paths]), preds[1], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(preds[1], preds_t[1], rtol=1e-3)
    # the Adam state came back too: both optimizers took the same number of steps
    for p, q in zip(b.model.parameters(), bt.model.parameters()):
        assert float(b.optimizer.state[p]["step"]) == float(bt.optimizer.state[q]["step"]) > 0


def test_train_step_on_the_streamed_route_with_both_backends():
    """train_step on the stub environments, vector sampler and stream sink: the fit
    comes after the policy update, so the first update's parameters are the same
    whichever backend fits, and the fitted baselines predict alike."""
    from mjrl_amd.algos.npg_cg import NPG
    from mjrl_amd.baselines.mlp_baseline import MLPBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.samplers import env_workers
    from mjrl_amd.utils.gym_env import EnvSpec
    from stub_env import StubEnv

    class Env:
        env_id = "stub-v0"
    out = []
    try:
        for backend in ("hip", "torch"):
            spec = EnvSpec(6, 2, 40, 1)
            torch.manual_seed(9)
            mb = MLPBaseline(spec, epochs=2, batch_size=64)
            mb.fit_backend = backend
            agent = NPG(Env(), MLP(spec, hidden_sizes=(64, 64), seed=3, init_log_std=-1.0), mb,
                        normalized_step_size=0.05, seed=200, save_logs=True)
            agent.sampler, agent.env_factory, agent.num_envs, agent.stream_staging = "vector", StubEnv, 16, True
            agent.sampler_workers = 0
            seen = []
            fit = agent._fit_baseline

            def spy(paths, return_errors=False, fit=fit, agent=agent, seen=seen):
                seen.append(getattr(getattr(agent, "_last_batch", None), "value_feat", None) is not None)
                return fit(paths, return_errors=return_errors)
            agent._fit_baseline = spy
            np.random.seed(77)
            agent.train_step(N=60, gamma=0.99, gae_lambda=0.95)
            assert seen == [True]   # the fit read the sink's matrix
            rs = np.random.RandomState(5)
            probe = [dict(observations=rs.randn(40, 6), rewards=np.zeros(40)) for _ in range(3)]
            out.append((agent.policy.get_param_values(), np.concatenate([mb.predict(p) for p in probe]),
                        float(mb.optimizer.state[next(mb.model.parameters())]["step"])))
    finally:
        env_workers.close_env_pools()
    (th_h, pred_h, steps_h), (th_t, pred_t, steps_t) = out
    assert np.array_equal(th_h, th_t)
    assert steps_h == steps_t > 0
    print("predictions: hip from torch %.3g (max relative)" % np.max(np.abs(pred_h - pred_t) / np.abs(pred_t)))
    np.testing.assert_allclose(pred_h, pred_t, rtol=1e-3)


def test_errors():
    from mjrl_amd.baselines.mlp_baseline import MLPBaseline
    from mjrl_amd.utils.gym_env import EnvSpec
    rs = np.random.RandomState(0)
    paths = [dict(observations=rs.randn(300, 5), rewards=rs.randn(300), returns=rs.randn(300))]
    b = MLPBaseline(EnvSpec(5, 2, 300, 1), batch_size=128)
    b.fit_backend = "hip"
    with pytest.raises(ValueError, match="64"):
        b.fit(paths)
    b = MLPBaseline(EnvSpec(5, 2, 300, 1))
    b.fit_backend = "triton"
    with pytest.raises(ValueError, match="fit_backend"):
        b.fit(paths)
