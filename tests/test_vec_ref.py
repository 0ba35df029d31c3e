"""The inputs of the direct kernel tests (test_gpu_cg_kernels.py), checked with the
reference alone (vec_ref.py): a bit-exact comparison of an fp64-accumulated dot
product is only meaningful where the exact sum is far enough from an f32 rounding
boundary that no summation order can round differently, and a condition on the
inputs belongs here, not next to the kernel.  Also the reference against the oracle's
CG and the packing against the parameter order."""
import numpy as np
import pytest

import vec_ref as V
from oracle import npg_cpu as O

F32, F64 = np.float32, np.float64


def test_shape_table_matches_the_formula():
    for shape, d in V.CG_SHAPES.items():
        assert V.make_shape(*shape).d == d
    wg = lambda d: (d + 1023) // 1024
    d = V.CG_SHAPES
    assert wg(d[(1756, 1, 256, 256)]) == 504 and wg(d[(1757, 1, 256, 256)]) == 505     # the partials end at cg[1024]
    assert d[(59, 2, 64, 64)] <= 8 * 1024 < d[(60, 2, 64, 64)]                           # k_cgm_xrp_f<8> / <32>
    assert (d[(39, 28, 256, 256)] + 63) // 64 == 1301 and d[(39, 28, 256, 256)] > 32 * 1024
    chunks_max = (V.CG_STATE - V.CG_PZ_PARTS) // 2
    assert (d[(39, 28, 256, 256)] + 63) // 64 <= chunks_max == 1536 < (d[(130, 3, 256, 256)] + 63) // 64 == 1565
    s = V.make_shape(12, 17, 32, 32)
    assert (s.mp, s.d - s.m, s.d - 1) == (32, 2033, 2049)     # log-std across the 2048 boundary


def test_exact_dot_margin():
    a = np.array([1, 2 ** -24, 2 ** -30], F32)
    one = np.ones(3, F32)
    v, mg = V.exact_dot(a, one)            # just above the midpoint of 1 and 1 + 2^-23
    assert v == F32(1 + 2 ** -23)
    assert mg == pytest.approx(2.0 ** -30 / (3 * 2.0 ** -53 * float(a.sum(dtype=F64))), rel=1e-12)
    v, mg = V.exact_dot(np.array([1, 2 ** -24], F32), np.ones(2, F32))   # on the boundary
    assert mg == 0
    v, mg = V.exact_dot(np.array([3, -1], F32), np.array([2, 2], F32))   # 4: the boundary below is 4 - 2^-23
    assert v == 4 and mg == (2.0 ** -23) / (2 * 2.0 ** -53 * 8)


@pytest.mark.parametrize("shape", list(V.CG_SHAPES))
def test_cg_dot_margins(shape):
    """b.b, p.z and r.r of every iteration: margin >= 1, so any fp64 summation order
    gives the reference's f32."""
    c = V.cg_case(shape)
    assert len(c["margins"]) == 1 + 2 * V.CG_ITERS
    assert all(mg >= 1 for _, mg in c["margins"]), c["margins"]
    rr1, rr2 = c["rr"]
    assert rr2 < c["tol_conv"] <= rr1 and c["tol_never"] < min(st["cg"][0] for st in c["states"])
    assert all(st["done"] == 0 for st in c["states"])


@pytest.mark.parametrize("shape", V.NPG_SHAPES)
def test_npg_dot_margin_and_clamp(shape):
    c = V.npg_case(shape)
    assert all(mg >= 1 for _, mg in c["margins"]), c["margins"]
    s, run = c["s"], c["runs"]["mode0"]
    ls = run["theta_new"][s.d - s.m:]
    raw = (c["theta"] + run["out"][0] * c["x"])[s.d - s.m:]
    assert (raw < F32(V.MIN_LS)).any() and (ls == F32(V.MIN_LS)).any()
    if s.m > 1:
        assert (ls > F32(V.MIN_LS)).any()


@pytest.mark.parametrize("shape", list(V.CG_SHAPES))
def test_log_std_block_is_insensitive_to_expf_rounding(shape):
    """hv on the log-std block at the cases' log-std values and directions: the same
    bits with sigma = exp(log_std) moved two f32 ulps either way, so the last bit of
    the device's expf cannot matter."""
    c = V.cg_case(shape)
    s = c["s"]
    for k in range(V.CG_ITERS):
        p = c["states"][k]["p"]
        hv = [V.cg_hv(s, c["gsums"][k], c["inv_T"], c["log_std"], p, u)[s.d - s.m:] for u in (-2, -1, 0, 1, 2)]
        assert all(np.array_equal(h.view(np.uint32), hv[2].view(np.uint32)) for h in hv)
        assert np.array_equal(V.cg_z(s, c["gsums"][k], c["inv_T"], c["damping"], c["log_std"], p).view(np.uint32),
                              c["states"][k + 1]["z"].view(np.uint32))
        assert not np.isnan(c["states"][k + 1]["z"]).any()


def test_reference_cg_matches_oracle():
    """Ten iterations with a dense SPD operator against oracle.cg_solve at the bar of
    test_cg_solve_generic_matches_reference_semantics."""
    rs = np.random.RandomState(2)
    A = rs.randn(300, 300).astype(F32)
    A = (A @ A.T / 300 + np.eye(300, dtype=F32)).astype(F32)
    b = rs.randn(300).astype(F32)
    f = lambda v: (A @ v).astype(F32)
    dot = V.Dots()
    st = V.cg_init(b, dot)
    for k in range(10):
        st = V.cg_iter(st, f(st["p"]), 1e-10, dot, k)
    xr = O.cg_solve(f, b.copy(), iters=10)
    assert st["x"].dtype == F32 and st["cg"][1] == 10
    assert np.linalg.norm(st["x"].astype(F64) - xr) / np.linalg.norm(xr) < 1e-5


def _unpack(s, packed):
    """The flat vector back from a packed set, tensor by tensor in oracle.param_shapes
    order, and the transposes."""
    off = V.packed_offsets(s.h0, s.h1, s.np, s.mp)
    if s.h0 == 0:
        Wp = packed[off["W0"]:off["W0"] + s.mp * s.np].reshape(s.mp, s.np)
        return [Wp[:s.m, :s.n], Wp[:s.m, s.n], packed[off["ls"]:off["ls"] + s.m]], []
    W0 = packed[off["W0"]:off["W0"] + s.h0 * s.np].reshape(s.h0, s.np)
    W1 = packed[off["W1"]:off["W1"] + s.h1 * s.h0].reshape(s.h1, s.h0)
    W2 = packed[off["W2"]:off["W2"] + s.mp * s.h1].reshape(s.mp, s.h1)
    W1T = packed[off["W1T"]:off["W1T"] + s.h0 * s.h1].reshape(s.h0, s.h1)
    W2T = packed[off["W2T"]:off["W2T"] + s.h1 * s.mp].reshape(s.h1, s.mp)
    return ([W0[:, :s.n], W0[:, s.n], W1, packed[off["b1"]:off["b1"] + s.h1], W2[:s.m],
             packed[off["b2"]:off["b2"] + s.m], packed[off["ls"]:off["ls"] + s.m]],
            [(W1T, W1.T), (W2T[:, :s.m], W2[:s.m].T)])


@pytest.mark.parametrize("shape", [(12, 17, 32, 32), (3, 2, 0, 0)])
def test_pack_round_trips(shape):
    s = V.make_shape(*shape)
    theta = np.arange(1, s.d + 1, dtype=F32)      # distinct, non-zero: every position names its source
    packed, mask = V.pack(s, theta)
    tensors, transposes = _unpack(s, packed)
    hidden = None if s.h0 == 0 else (s.h0, s.h1)
    assert [t.shape for t in tensors] == O.param_shapes(s.n, s.m, hidden)
    assert np.array_equal(np.concatenate([t.reshape(-1) for t in tensors]), theta)
    for a, b in transposes:
        assert np.array_equal(a, b)
    # every flat parameter once, plus its transpose copy for W1 and W2
    assert mask.sum() == s.d + (0 if s.h0 == 0 else s.h1 * s.h0 + s.m * s.h1)
    assert (packed[~mask] == 0).all() and (packed[mask] != 0).all()
    lo = theta.copy()
    lo[s.d - s.m:] = np.linspace(-4, -2, s.m)
    lo[s.d - 1] = -3.0
    pc, mc = V.pack(s, lo, clamp=True, min_ls=-3.0)
    assert np.array_equal(mc, mask)
    assert np.array_equal(_unpack(s, pc)[0][-1], np.maximum(lo[s.d - s.m:], F32(-3.0)))
