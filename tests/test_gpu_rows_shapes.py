"""GPU tests of the row-kernel path (k_rows + the weight-gradient kernels) on the
shapes the fixtures do not cover: every (hidden, padded action width, padded
observation width) combination of k_wgrad_all's instances and of k_wgrad's
fallbacks, against an fp64 evaluation of the same closed forms (torch float64,
jvp / vjp of the Gaussian-MLP mean).  Row counts are not
multiples of the 32-row tiles, so every slice count / empty-slice / zero-tile
path of the slab layout runs.  Tolerance: 1e-5 norm-relative (the exact-f32
kernels' own error is 1e-7 .. 1e-6 against fp64)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def nrel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _mu64(theta, X, n, m, h):
    h0, h1 = h
    o = 0

    def take(k, shape):
        nonlocal o
        t = theta[o:o + k].reshape(shape)
        o += k
        return t
    W0 = take(h0 * n, (h0, n)); b0 = take(h0, (h0,))
    W1 = take(h1 * h0, (h1, h0)); b1 = take(h1, (h1,))
    W2 = take(m * h1, (m, h1)); b2 = take(m, (m,))
    return torch.tanh(torch.tanh(X @ W0.T + b0) @ W1.T + b1) @ W2.T + b2


def _truth(obs, act, adv, theta, v, damping, n, m, h):
    """fp64 VPG and F v + damping v at old == new (gaussian_mlp.py:100-140,
    npg_cg.py:55-74)."""
    from torch.func import jvp, vjp
    dev = torch.device("cuda:0")
    X = torch.from_numpy(np.float32(obs).astype(np.float64)).to(dev)
    A = torch.from_numpy(np.float32(act).astype(np.float64)).to(dev)
    adv = torch.from_numpy(np.float32(adv).astype(np.float64)).to(dev)
    th = torch.from_numpy(theta.astype(np.float64)).to(dev)
    vv = torch.from_numpy(v.astype(np.float64)).to(dev)
    T = X.shape[0]
    d_mu = th.numel() - m
    ls = th[d_mu:]
    sig2 = torch.exp(2 * ls)
    f = lambda t: _mu64(t, X, n, m, h)
    mu, back = vjp(f, th[:d_mu])
    z = (A - mu) / torch.exp(ls)
    g_mu = back((adv[:, None] * (A - mu) / sig2) / T)[0]
    g_ls = (adv[:, None] * (z * z - 1)).sum(0) / T
    _, Jv = jvp(f, (th[:d_mu],), (vv[:d_mu],))
    Fm = back((2.0 / (2.0 * sig2 + 1e-8)) * Jv / T)[0]
    c = 4 * sig2 * (2 * sig2 - 1e-8) / (2 * sig2 + 1e-8) ** 2
    return torch.cat([g_mu, g_ls]).cpu().numpy(), (torch.cat([Fm, c * vv[d_mu:]]) + damping * vv).cpu().numpy()


@pytest.mark.parametrize("n,m,h,T", [
    (17, 6, (128, 128), 5001),     # HalfCheetah: k_wgrad_all<128, 16, 2> (two prefetch stages)
    (45, 24, (128, 128), 3333),    # Adroit-like: k_wgrad_all<128, 32, 4>
    (100, 20, (128, 128), 1000),   # k_wgrad_all<128, 32, 8>
    (20, 40, (128, 128), 2049),    # k_wgrad_all<128, 64, 2>
    (70, 40, (128, 128), 777),     # 128-wide, 64 actions, np = 80: the k_wgrad fallback
    (15, 40, (32, 32), 4097),      # k_wgrad_all<32, 64, 2>
    (40, 33, (64, 64), 1500),      # k_wgrad_all<64, 64, 4>
    (39, 28, (256, 256), 2001),    # door: 256-wide layers on k_wgrad
    (17, 6, (128, 128), 31),       # a single partial tile, most slices empty
])
def test_rows_path_vs_fp64(n, m, h, T):
    from mjrl_amd.engine import UpdateEngine
    rs = np.random.RandomState(n * 1000 + T)
    obs, act, adv = rs.randn(T, n), rs.randn(T, m), rs.randn(T)
    d = h[0] * n + h[0] + h[1] * h[0] + h[1] + m * h[1] + m + m
    theta = (rs.randn(d) * 0.1).astype(np.float32)
    theta[-m:] = np.linspace(-1.0, 0.3, m)
    v = (rs.randn(d) * 1e-2).astype(np.float32)
    vpg64, fv64 = _truth(obs, act, adv, theta, v, 1e-4, n, m, h)
    eng = UpdateEngine(n, m, h, device="cuda:0", precision="f32")
    assert eng.accumulate_path() == 0
    eng.load_rows(obs, act, adv)
    g = eng.forward_pass(torch.from_numpy(theta).cuda(), T).cpu().numpy()
    fv = eng.fvp(torch.from_numpy(v).cuda(), damping=1e-4, T=T).cpu().numpy()
    assert nrel(g, vpg64) < 1e-5, nrel(g, vpg64)
    assert nrel(fv, fv64) < 1e-5, nrel(fv, fv64)
    # every block of the flat parameter vector, not just the norm (a missing
    # bias column or a dropped strip would hide in the total)
    offs = np.cumsum([0, h[0] * n, h[0], h[1] * h[0], h[1], m * h[1], m, m])
    for a, b in zip(offs[:-1], offs[1:]):
        assert nrel(g[a:b], vpg64[a:b]) < 1e-4, (a, b, nrel(g[a:b], vpg64[a:b]))
        assert nrel(fv[a:b], fv64[a:b]) < 1e-4, (a, b, nrel(fv[a:b], fv64[a:b]))


@pytest.mark.parametrize("n,m,h,T", [
    (8, 2, (64, 64), 12500),       # Swimmer: every weight image in LDS, one observation chunk
    (8, 2, (64, 64), 64),          # one tile
    (8, 2, (64, 64), 40000),       # more tiles than workgroups
    (17, 6, (32, 32), 9001),       # hidden 32, partial last tile
    (45, 20, (64, 64), 5000),      # MP 32: W1 / W2 images, W0 from L2
    (100, 6, (64, 64), 7777),      # two observation chunks (the gW0 re-stream)
    (150, 20, (32, 32), 4001),     # three chunks, MP 32
])
def test_fused_path_vs_fp64(n, m, h, T):
    """The fused persistent kernel (k_fused: weight images in LDS, W1^T / W2^T read
    transposed from them, the slab staged through LDS) against the same fp64
    closed forms, on each of its layout variants."""
    from mjrl_amd.engine import UpdateEngine
    rs = np.random.RandomState(n * 1000 + T)
    obs, act, adv = rs.randn(T, n), rs.randn(T, m), rs.randn(T)
    d = h[0] * n + h[0] + h[1] * h[0] + h[1] + m * h[1] + m + m
    theta = (rs.randn(d) * 0.1).astype(np.float32)
    theta[-m:] = np.linspace(-1.0, 0.3, m)
    v = (rs.randn(d) * 1e-2).astype(np.float32)
    vpg64, fv64 = _truth(obs, act, adv, theta, v, 1e-4, n, m, h)
    eng = UpdateEngine(n, m, h, device="cuda:0", precision="f32")
    assert eng.accumulate_path() == 1
    eng.load_rows(obs, act, adv)
    g = eng.forward_pass(torch.from_numpy(theta).cuda(), T).cpu().numpy()
    fv = eng.fvp(torch.from_numpy(v).cuda(), damping=1e-4, T=T).cpu().numpy()
    assert nrel(g, vpg64) < 1e-5, nrel(g, vpg64)
    assert nrel(fv, fv64) < 1e-5, nrel(fv, fv64)
    offs = np.cumsum([0, h[0] * n, h[0], h[1] * h[0], h[1], m * h[1], m, m])
    for a, b in zip(offs[:-1], offs[1:]):
        assert nrel(g[a:b], vpg64[a:b]) < 1e-4, (a, b, nrel(g[a:b], vpg64[a:b]))
        assert nrel(fv[a:b], fv64[a:b]) < 1e-4, (a, b, nrel(fv[a:b], fv64[a:b]))


def _cg_state(eng, k):
    """(x, r, p) of the update's CG after k iterations, cloned.  The buffer parity
    rule lives here: r alternates r / r2 every iteration on every schedule, p
    alternates p / p2 only on the mjrl_cg_step1 schedule (the others update p in
    place).  k = 0 is cg_solve's initial state, x = 0 and r = p = g."""
    v = eng.vec
    if k == 0:
        g = v["g"].clone()
        return torch.zeros_like(g), g, g.clone()
    r = v["r2"] if k % 2 else v["r"]
    p = v["p2"] if (k % 2 and _cg_step1(eng)) else v["p"]
    return v["x"].clone(), r.clone(), p.clone()


def _cg_step1(eng):
    """Whether update() runs this shape's CG on the mjrl_cg_step1 schedule: more
    64-parameter chunks than the CG state holds p.z partials for."""
    from mjrl_amd import _lib
    return (eng.shape.d + 63) // 64 > (_lib.CG_STATE - _lib.CG_PZ_PARTS) // 2


@pytest.mark.parametrize("n,m,h,step1", [
    (130, 3, (256, 256), True),    # wide: d = 100,102 = 1,565 chunks of 64 > 1,536: the mjrl_cg_step1 schedule
    (39, 28, (256, 256), False),   # door (control): the fused gather + mjrl_cg_step_xr_p schedule
])
def test_update_cg_iterations_teacher_forced(n, m, h, step1):
    """Single CG iterations of update() on the k_rows + k_wgrad shapes, each forced
    from the update's own state after K iterations: z = F p_K + damping p_K from the
    standalone eng.fvp (mjrl_cg_init + mjrl_policy_fvp + mjrl_cg_step: other
    launches than the update's), one step of cg_solve (mjrl/utils/cg_solve.py:9-20)
    in fp64 on the host, against the state update(cg_iters=K + 1) leaves.  The wide
    shape has more 64-parameter chunks than the CG state holds p.z partials for, so
    its iterations run all-reduce + mjrl_cg_step1; the door shape is the control
    (its schedule is pinned to the reference by the c5 fixtures).  T = 70 rows in
    two ragged paths: every 16- and 32-row tile is partial.  Bound: 1e-5
    norm-relative, the bar for a teacher-forced CG iteration."""
    from mjrl_amd.comm import LocalComm
    from mjrl_amd.engine import UpdateEngine, DeviceBatch
    rs = np.random.RandomState(n * 1000 + m)
    lengths = np.array([33, 37])
    T = int(lengths.sum())
    d = h[0] * n + h[0] + h[1] * h[0] + h[1] + m * h[1] + m + m
    theta = (rs.randn(d) * 0.1).astype(np.float32)
    theta[-m:] = np.linspace(-1.0, 0.3, m)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    batch = DeviceBatch(t(rs.randn(T, n).astype(np.float32)), t(rs.randn(T, m).astype(np.float32)), t(rs.randn(T)),
                        t(rs.randn(T)), t(off), t(np.zeros(2, dtype=np.uint8)))
    eng = UpdateEngine(n, m, h, device="cuda:0", comm=LocalComm())
    eng.graphs = False
    assert eng.accumulate_path() == 0 and eng.shape.d == d
    assert _cg_step1(eng) == step1
    th = t(theta)
    damping = 1e-4

    def run(K):
        res = eng.update(batch, th, algo="npg", cg_iters=K, damping=damping, graph=False)
        assert res["cg_iters"] == K, res["cg_iters"]   # no early exit: every iteration ran
        return [a.cpu().numpy().astype(np.float64) for a in _cg_state(eng, K)]

    for K in range(3):
        x0, r0, p0 = run(K)
        x1, r1, p1 = run(K + 1)
        z = eng.fvp(t(p0.astype(np.float32)), damping=damping).cpu().numpy().astype(np.float64)
        # one iteration of cg_solve.py:9-20 in fp64
        rdotr = r0.dot(r0)
        a = rdotr / p0.dot(z)
        xh = x0 + a * p0
        rh = r0 - a * z
        ph = rh + (rh.dot(rh) / rdotr) * p0
        nx = np.linalg.norm(x0) if K else np.linalg.norm(xh)
        errs = (np.linalg.norm(x1 - xh) / nx, np.linalg.norm(r1 - rh) / np.linalg.norm(r0),
                np.linalg.norm(p1 - ph) / np.linalg.norm(p0))
        print("cg iteration %d (step1=%s): x %.3g r %.3g p %.3g" % (K, step1, *errs))
        assert max(errs) < 1e-5, (K, errs)
