"""Plain-numpy restatement of the vector kernels between the policy passes of an
update (csrc/cg.hip and the statistics part of csrc/batch.hip), written from their
documented arithmetic (include/mjrl_amd.h), not from the
kernels:

  - a dot product is the f32 rounding of the EXACT sum of the (exact, 48-bit) fp64
    products; the kernels accumulate the same products in fp64 in some fixed order,
    which rounds to the same f32 whenever the exact sum is far enough from an f32
    rounding boundary (`exact_dot`'s margin, asserted >= 1 in test_vec_ref.py for
    every dot product the GPU tests take);
  - every element update is an f32 multiply and an f32 add, rounded separately
    (numpy f32 arrays: no fused multiply-add);
  - divisions and square roots are IEEE (correctly rounded).

Importable without a GPU and without the HIP library.  The fixed inputs of the GPU
tests (seeds, shapes) are built here too, so test_vec_ref.py can check them with the
reference alone."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

F32 = np.float32
F64 = np.float64

CG_STATE, CG_PZ_PARTS, STEP_OUT, LS_LOG, LS_STATE = 4096, 1024, 1024, 32, 128   # include/mjrl_amd.h
NAN_BITS = 0x7FC0BEEF   # the quiet NaN tests pre-fill outputs with: an unwritten word keeps these bits

Shape = namedtuple("Shape", "n m h0 h1 np mp d packed")


def round_up(x, k):
    return (x + k - 1) // k * k


def packed_offsets(h0, h1, np_, mp):
    """Float offsets of the packed parameter set (csrc/common.h `Packed`)."""
    o, off = 0, {}
    if h0 == 0:
        off["W0"] = o
        o += mp * np_
    else:
        for k, sz in (("W0", h0 * np_), ("W1", h1 * h0), ("b1", h1), ("W2", mp * h1), ("b2", mp),
                      ("W1T", h0 * h1), ("W2T", h1 * mp)):
            off[k] = o
            o += sz
    off["ls"] = o
    o += mp
    off["total"] = round_up(o, 4)
    return off


def make_shape(n, m, h0, h1):
    """mjrl_shape_init's formula (np, mp, d, packed)."""
    np_ = round_up(n + 1, 16)
    mp = 16 if m <= 16 else (32 if m <= 32 else (64 if m <= 64 else round_up(m, 16)))
    d = m * n + 2 * m if h0 == 0 else h0 * n + h0 + h1 * h0 + h1 + m * h1 + 2 * m
    return Shape(n, m, h0, h1, np_, mp, d, packed_offsets(h0, h1, np_, mp)["total"])


def param_shapes(s):
    """The flat vector's tensors, in order (the header's layout comment)."""
    if s.h0 == 0:
        return [(s.m, s.n), (s.m,), (s.m,)]
    return [(s.h0, s.n), (s.h0,), (s.h1, s.h0), (s.h1,), (s.m, s.h1), (s.m,), (s.m,)]


def split_params(s, theta):
    out, i = [], 0
    for shp in param_shapes(s):
        k = int(np.prod(shp))
        out.append(theta[i:i + k].reshape(shp))
        i += k
    assert i == s.d == len(theta)
    return out


def clamp_min(v, min_ls):
    """`v < min ? min : v` (a NaN stays)."""
    return np.where(v < F32(min_ls), F32(min_ls), v).astype(F32)


def pack(s, theta, clamp=False, min_ls=0.0, fill=0.0):
    """(packed[s.packed], mask): the packed set of flat theta and the positions it
    writes; every other position holds `fill`."""
    theta = np.asarray(theta, F32)
    off = packed_offsets(s.h0, s.h1, s.np, s.mp)
    packed = np.full(s.packed, fill, F32)
    mask = np.zeros(s.packed, bool)

    def put(o, block, pitch):
        block = np.atleast_2d(block)
        idx = o + np.arange(block.shape[0])[:, None] * pitch + np.arange(block.shape[1])[None, :]
        packed[idx] = block
        mask[idx] = True

    t = split_params(s, theta)
    ls = clamp_min(t[-1], min_ls) if clamp else t[-1]
    if s.h0 == 0:
        W, b = t[0], t[1]
        put(off["W0"], W, s.np)                  # [mp][np], rows < m
        put(off["W0"] + s.n, b[:, None], s.np)   # the bias in column n
    else:
        W0, b0, W1, b1, W2, b2 = t[:6]
        put(off["W0"], W0, s.np)                 # [h0][np]
        put(off["W0"] + s.n, b0[:, None], s.np)  # b0 in column n
        put(off["W1"], W1, s.h0)
        put(off["b1"], b1, s.h1)
        put(off["W2"], W2, s.h1)                 # [mp][h1], rows < m
        put(off["b2"], b2, s.m)
        put(off["W1T"], W1.T, s.h1)              # [h0][h1]
        put(off["W2T"], W2.T, s.mp)              # [h1][mp], columns < m
    put(off["ls"], ls, s.m)
    return packed, mask


# --------------------------------------------------------------------------
# dot products
# --------------------------------------------------------------------------
def round_margin(s, n, sabs):
    """Distance from s to the nearer boundary of its f32 rounding interval, in units
    of n 2^-53 sabs: the worst-case error of an fp64 accumulation of n terms with
    absolute sum sabs, in any order.  >= 1: every order rounds to the same f32."""
    f = F32(s)
    lo = (float(f) + float(np.nextafter(f, F32(-np.inf)))) / 2   # midpoints of adjacent f32s: exact in fp64
    hi = (float(f) + float(np.nextafter(f, F32(np.inf)))) / 2
    bound = n * 2.0 ** -53 * sabs
    return math.inf if bound == 0 else min(s - lo, hi - s) / bound


def exact_dot(a, b):
    """(f32 rounding of the exact a.b, margin) for f32 vectors a, b."""
    assert a.dtype == F32 and b.dtype == F32 and a.shape == b.shape
    t = a.astype(F64) * b.astype(F64)   # exact: 24 x 24 bits
    s = math.fsum(t.tolist())
    sabs = math.fsum(np.abs(t).tolist())
    return F32(s), round_margin(s, len(t), sabs)


class Dots:
    """Takes the dot products of one reference run and keeps (name, margin) of each."""

    def __init__(self):
        self.margins = []

    def __call__(self, name, a, b):
        v, mg = exact_dot(a, b)
        self.margins.append((name, mg))
        return v


def chunk_sums(a, b, chunk=64):
    """Exact sums and absolute sums of a.b over consecutive chunks (the fused
    gather's p.z partials: one per 64 parameters)."""
    t = a.astype(F64) * b.astype(F64)
    t = np.concatenate([t, np.zeros(-len(t) % chunk)]).reshape(-1, chunk)
    return (np.array([math.fsum(row.tolist()) for row in t]),
            np.array([math.fsum(np.abs(row).tolist()) for row in t]))


# --------------------------------------------------------------------------
# one CG iteration (mjrl_cg_step's documented formulas) and the init
# --------------------------------------------------------------------------
def sigma(log_std, ulps=0):
    """f32 exp(log_std), moved by `ulps` f32 steps (positive values: bit pattern + ulps)."""
    sg = np.exp(np.asarray(log_std, F32).astype(F64)).astype(F32)
    return (sg.view(np.int32) + np.int32(ulps)).view(F32)


def logstd_curv(sg):
    """c(sigma) of DESIGN.md §2 in fp64: 4 u (2 u - 1e-8) / (2 u + 1e-8)^2, u = sigma^2."""
    uu = np.asarray(sg, F64) * np.asarray(sg, F64)
    return 4.0 * uu * (2.0 * uu - 1e-8) / ((2.0 * uu + 1e-8) * (2.0 * uu + 1e-8))


def cg_hv(s, gsum, inv_T, log_std, p, sg_ulps=0):
    """F p without damping: f32(f64(gsum) inv_T) on the mean block, f32(c(sigma) p)
    on the log-std block (gsum's log-std block is not read)."""
    ls0 = s.d - s.m
    hv = np.empty(s.d, F32)
    hv[:ls0] = (gsum[:ls0].astype(F64) * inv_T).astype(F32)
    hv[ls0:] = (logstd_curv(sigma(log_std, sg_ulps)) * p[ls0:].astype(F64)).astype(F32)
    return hv


def cg_z(s, gsum, inv_T, damping, log_std, p, sg_ulps=0):
    return cg_hv(s, gsum, inv_T, log_std, p, sg_ulps) + F32(damping) * p   # fadd(hv, fmul(damping, p))


def cg_init(b, dot):
    b = np.asarray(b, F32)
    return dict(x=np.zeros_like(b), r=b.copy(), p=b.copy(), z=None,
                cg=np.array([dot("b.b", b, b), 0, 0, 0, 0], F32), done=0)


def cg_iter(st, z, tol, dot, k=0):
    """cg_solve.py:10-20 on state st with z = A p; returns the new state (a converged
    state is returned as it is)."""
    if st["done"]:
        return st
    x, r, p, rdotr = st["x"], st["r"], st["p"], st["cg"][0]
    pz = dot("p.z[%d]" % k, p, z)
    v = rdotr / pz                      # f32 division
    x = x + v * p
    r = r - v * z
    rr = dot("r.r[%d]" % k, r, r)
    mu = rr / rdotr
    p = r + mu * p
    return dict(x=x, r=r, p=p, z=z, cg=np.array([rr, st["cg"][1] + F32(1), v, mu, pz], F32),
                done=int(rr < F32(tol)))


# --------------------------------------------------------------------------
# the NPG step and the device TRPO line search
# --------------------------------------------------------------------------
def apply_step(s, theta, x, alpha, min_ls):
    v = (theta + F32(alpha) * x).astype(F32)
    v[s.d - s.m:] = clamp_min(v[s.d - s.m:], min_ls)
    return v


def npg_step(s, g, x, theta, mode, delta, alpha_in, const_lr, min_ls, dot):
    """(out[0..2] = (alpha, g.x, delta), theta_new)."""
    gx = dot("g.x", g, x)
    dl = F32(delta)
    if mode == 0:
        alpha = np.sqrt(np.abs(F32(delta) / (gx + F32(1e-20))))
    else:
        alpha = F32(alpha_in)
        if const_lr:
            dl = (alpha * alpha) * gx
    assert type(alpha) is F32 and type(dl) is F32
    return np.array([alpha, gx, dl], F32), apply_step(s, theta, x, alpha, min_ls)


class TrpoSearch:
    """mjrl_trpo_trial's state: ls[LS_STATE], skip, out[0] and theta_new."""

    def __init__(self, s, x, theta, min_ls, alpha0, theta_new, ls):
        self.s, self.x, self.theta, self.min_ls = s, x, theta, min_ls
        self.out0, self.theta_new, self.ls, self.skip = F32(alpha0), theta_new.copy(), ls.copy(), 0

    def trial(self, k, sums, inv_T, kl_dist, apply):
        if k > 1 and self.skip:
            return
        a_prev = self.out0 if k == 1 else self.ls[8 + k - 1]
        kl, surr = F32(F64(sums[1]) * inv_T), F32(F64(sums[0]) * inv_T)
        acc = float(kl) < kl_dist
        self.ls[LS_LOG + 3 * (k - 1):LS_LOG + 3 * k] = (a_prev, kl, surr)
        self.ls[1], self.ls[2], self.skip = F32(acc), F32(k), int(acc)
        if acc:
            self.out0 = a_prev
        elif apply:
            a = F32(0.9) * a_prev
            self.ls[8 + k] = a
            self.theta_new = apply_step(self.s, self.theta, self.x, a, self.min_ls)


# --------------------------------------------------------------------------
# statistics: elementwise IEEE fp64, sums by fsum
# --------------------------------------------------------------------------
def moments(x, center=None):
    """(out[6], (sum |x - c|, sum (x - c)^2)): out as mjrl_moments documents it, the
    sums exact over the fp64-rounded terms; the second pair scales the bound
    N 2^-53 sum|terms| of out[0] and out[1]."""
    x = np.asarray(x).astype(F64)
    c = F64(center[0]) / F64(center[2]) if center is not None else 0.0
    dv = x - c
    sq = dv * dv
    s1, s2 = math.fsum(dv.tolist()), math.fsum(sq.tolist())
    mn, mx = (x.min(), x.max()) if len(x) else (math.inf, -math.inf)
    return (np.array([s1, s2, len(x), mn, mx, -mn], F64),
            (math.fsum(np.abs(dv).tolist()), s2))


def whiten(adv, m1, m2, eps):
    """(w64, adv32) of mjrl_whiten."""
    mean = F64(m1[0]) / F64(m1[2])
    den = np.sqrt(F64(m2[1]) / F64(m1[2])) + eps
    w = (np.asarray(adv, F64) - mean) / den
    return w, w.astype(F32)


def dapg_adv(w64, mw1, mw2, T_demo, demo_coef):
    den = np.sqrt(F64(mw2[1]) / F64(mw1[2])) + 1e-8
    rl = (1e-2 * (np.asarray(w64, F64) / den)).astype(F32)
    return np.concatenate([rl, np.full(T_demo, F32(1e-2 * demo_coef), F32)])


# --------------------------------------------------------------------------
# the fixed inputs of tests/test_gpu_cg_kernels.py, and their reference runs
# --------------------------------------------------------------------------
# (n, m, h0, h1) -> d: the edges of the d-dependent code (see the GPU test's table)
CG_SHAPES = {
    (3, 2, 0, 0): 10,
    (5, 3, 32, 32): 1350,
    (12, 17, 32, 32): 2050,
    (59, 2, 64, 64): 8132,
    (60, 2, 64, 64): 8196,
    (376, 17, 64, 64): 29410,
    (39, 28, 256, 256): 83256,
    (130, 3, 256, 256): 100102,
    (1756, 1, 256, 256): 515842,
    (1757, 1, 256, 256): 516098,
}
# one seed per shape, chosen so every dot product of the case has margin >= 1
# (test_vec_ref.py asserts it; a seed that fails there is replaced, never the bound)
CG_SEEDS = {k: 100 + i for i, k in enumerate(CG_SHAPES)}
NPG_SHAPES = [(3, 2, 0, 0), (12, 17, 32, 32), (1756, 1, 256, 256), (1757, 1, 256, 256)]
NPG_SEEDS = {k: 200 + i for i, k in enumerate(NPG_SHAPES)}
TRPO_SHAPES = [(3, 2, 0, 0), (12, 17, 32, 32)]
WIDE_SHAPE = (27, 64, 32, 32)  # the log-std curvature over [-10, 2]: m = 64, the block 4064..4127 across 4096
CG_T = 1000                    # rows behind gsum: inv_T = 1 / 1000 is inexact in fp64
CG_DAMPING = 1e-4
CG_ITERS = 3
MIN_LS = -3.0


def _theta_with_log_std(s, rs, log_std):
    theta = (0.1 * rs.standard_normal(s.d)).astype(F32)
    theta[s.d - s.m:] = log_std
    return theta


@lru_cache(maxsize=None)
def cg_case(shape):
    """Inputs and the reference run of CG_ITERS teacher-forced iterations: iteration
    k's gsum is f32(a p_k T) from the REFERENCE's p_k with a fixed diagonal a in
    [0.5, 2] (an SPD operator, well-conditioned dots), NaN on the log-std block (which
    no kernel may read).  Also the convergence variant: the same run with a
    residual_tol between r.r of iterations 1 and 2."""
    s = make_shape(*shape)
    rs = np.random.RandomState(CG_SEEDS[shape])
    ls0, inv_T = s.d - s.m, 1.0 / CG_T
    gsum0 = (CG_T * rs.standard_normal(s.d)).astype(F32)      # the VPG's sums: b = f32(gsum0 / T)
    a = rs.uniform(0.5, 2.0, s.d)
    log_std = np.sort(rs.uniform(-1.0, 0.3, s.m)).astype(F32)      # spread over [-1, 0.3], both ends taken
    log_std[0], log_std[-1] = -1.0, 0.3
    theta = _theta_with_log_std(s, rs, log_std)
    dot = Dots()
    b = (gsum0.astype(F64) * inv_T).astype(F32)
    states, gsums = [cg_init(b, dot)], []
    for k in range(CG_ITERS):
        p = states[-1]["p"]
        gs = (a * p.astype(F64) * CG_T).astype(F32)
        gs[ls0:] = np.uint32(NAN_BITS).view(F32)
        gsums.append(gs)
        z = cg_z(s, gs, inv_T, CG_DAMPING, log_std, p)
        states.append(cg_iter(states[-1], z, 1e-10, dot, k))
    rr1, rr2 = states[1]["cg"][0], states[2]["cg"][0]
    tol = F32(math.sqrt(float(rr1) * float(rr2)))
    conv = [states[0], states[1], dict(states[2], done=1)]
    return dict(s=s, shape=shape, b=b, gsum0=gsum0, scale=inv_T, inv_T=inv_T, damping=CG_DAMPING, theta=theta,
                log_std=log_std, gsums=gsums, states=states, margins=dot.margins, tol_never=1e-10,
                tol_conv=tol, conv=conv, rr=(rr1, rr2))


@lru_cache(maxsize=None)
def npg_case(shape):
    """Inputs and reference results of mjrl_npg_step in mode 0, mode 1 and mode 1
    with const_lr.  x = g times a positive diagonal plus small noise (the CG solution
    of an SPD system is positively correlated with its right-hand side); some log-std
    entries start at or near min_log_std and move down, so the clamp acts."""
    s = make_shape(*shape)
    rs = np.random.RandomState(NPG_SEEDS[shape])
    g = rs.standard_normal(s.d).astype(F32)
    x = (g * rs.uniform(0.5, 2.0, s.d) + 0.01 * rs.standard_normal(s.d)).astype(F32)
    log_std = np.linspace(MIN_LS - 0.5, -1.0, s.m).astype(F32)
    log_std[0] = MIN_LS
    theta = _theta_with_log_std(s, rs, log_std)
    x[s.d - s.m] = F32(-1.0)      # the entry at min_log_std moves below it
    delta, alpha_in = 0.05, 0.0123
    runs = {}
    margins = []
    for name, (mode, const_lr) in (("mode0", (0, 0)), ("mode1", (1, 0)), ("const_lr", (1, 1))):
        dot = Dots()
        out, th = npg_step(s, g, x, theta, mode, delta, alpha_in, const_lr, MIN_LS, dot)
        runs[name] = dict(mode=mode, const_lr=const_lr, out=out, theta_new=th)
        margins += dot.margins
    return dict(s=s, shape=shape, g=g, x=x, theta=theta, delta=delta, alpha_in=alpha_in, runs=runs,
                margins=margins[:1])     # the three runs take the same g.x
