"""The statistics kernels of csrc/batch.hip (moments, whitening, DAPG advantages)
and the row gather, each called through the C ABI alone and compared with the numpy
restatement of vec_ref.py: elementwise results bit for bit (IEEE fp64 division and
square root are correctly rounded on both sides), minima / maxima / counts exactly,
and the two sums within N 2^-53 sum|terms| of their fsum values, the worst case of an
fp64 accumulation of N terms in any order.

Lengths: 0, 1, the wave (63, 64) and workgroup (257, 1023, 1025) edges, 16,385 (a
grid-stride tail), 69,632 = 17 x 4096 (the first one-launch grid above its floor of
16 workgroups) and 1,048,577 (both grids saturated at 256)."""
import math

import numpy as np
import pytest
import torch

import vec_ref as V

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
LENGTHS = [0, 1, 63, 64, 257, 1023, 1025, 16385, 69632, 1048577]
NAN32 = U32(V.NAN_BITS).view(F32)
NAN64 = U64(0x7FF80000DEADBEEF).view(F64)
MOM_SCRATCH = 2056
TAIL32, TAIL64 = np.full(1, NAN32, F32), np.full(1, NAN64, F64)   # the untouched element past an output


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: U32, 8: U64}[a.dtype.itemsize])


def _same(got, want, what):
    got = _host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want, got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: got %r, reference %r" % (
        what, len(bad), got.size, bad[:6].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())


@pytest.fixture(scope="module")
def K():
    from mjrl_amd import _lib
    return _lib.calls()


@pytest.fixture(scope="module")
def st():
    from mjrl_amd import _lib
    return _lib.stream_ptr()


_DATA = {}


def _data(N, seed=0):
    """N values of mean 40 and standard deviation 5 (a second pass that forgot its
    centre would give a sum of squares 65 times too large), computed once."""
    if (N, seed) not in _DATA:
        _DATA[N, seed] = 40.0 + 5.0 * np.random.RandomState(1000 + seed).standard_normal(N)
    return _DATA[N, seed]


_REF = {}


def _moments_ref(N, seed, f32, centred):
    key = (N, seed, f32, centred)
    if key not in _REF:
        x = _data(N, seed)
        _REF[key] = V.moments(x.astype(F32) if f32 else x, CENTER if centred else None)
    return _REF[key]


# the record a centred pass reads (the out[] of some uncentred pass): mean 39.96875
CENTER = np.array([1279.0, 7.0, 32.0, 0.0, 0.0, 0.0], F64)


def _check_moments(out, ref, N, what):
    want, (abs1, abs2) = ref
    out = _host(out) if isinstance(out, torch.Tensor) else out
    _same(out[2:6], want[2:6], what + " out[2..5] (N, min, max, -min)")
    for i, sabs in ((0, abs1), (1, abs2)):
        assert abs(out[i] - want[i]) <= N * 2.0 ** -53 * sabs, (what, i, out[i], want[i], N * 2.0 ** -53 * sabs)
    if N == 0:
        assert out[3] == math.inf and out[4] == -math.inf and out[5] == -math.inf and out[0] == 0 and out[1] == 0


def _out6():
    return _dev(np.full(6, NAN64, F64))


@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("centred", [False, True])
def test_moments_two_launch(K, st, N, centred):
    """mjrl_moments (f64 input) and mjrl_moments_f32."""
    rpart = torch.zeros(MOM_SCRATCH, dtype=torch.float64, device=DEV)
    center = _dev(CENTER) if centred else None
    for f32 in (False, True):
        x = _data(N)
        xd = _dev(x.astype(F32) if f32 else x)
        out = _out6()
        (K.mjrl_moments_f32 if f32 else K.mjrl_moments)(xd if N else None, N, center, rpart, out, st)
        _check_moments(out, _moments_ref(N, 0, f32, centred), N, "moments%s N=%d" % ("_f32" if f32 else "", N))


@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("centred", [False, True])
def test_moments2(K, st, N, centred):
    """mjrl_moments2: x1 alone (out2 null), then x1 [N] with x2 of another length, with
    N2 = 0, and with the two swapped, back to back on ONE rpart, so every launch runs
    on the ticket the one before it left, with a different grid."""
    rpart = torch.zeros(MOM_SCRATCH, dtype=torch.float64, device=DEV)
    center = _dev(CENTER) if centred else None
    N2 = 4097 if N != 4097 else 5000
    x1, x2, none = _dev(_data(N)) if N else None, _dev(_data(N2, 1)), None
    r1, r2, r0 = _moments_ref(N, 0, False, centred), _moments_ref(N2, 1, False, centred), \
        _moments_ref(0, 1, False, centred)
    o1, o2 = _out6(), _out6()
    K.mjrl_moments2(x1, N, center, None, 0, None, rpart, o1, None, st)
    _check_moments(o1, r1, N, "moments2 alone N=%d" % N)
    for (xa, Na, ra), (xb, Nb, rb) in (((x1, N, r1), (x2, N2, r2)), ((x2, N2, r2), (x1, N, r1)),
                                       ((x1, N, r1), (none, 0, r0))):
        o1, o2 = _out6(), _out6()
        K.mjrl_moments2(xa, Na, center, xb, Nb, center, rpart, o1, o2, st)
        _check_moments(o1, ra, Na, "moments2 out1 N=%d with N2=%d" % (Na, Nb))
        _check_moments(o2, rb, Nb, "moments2 out2 N=%d after N1=%d" % (Nb, Na))
    assert _host(rpart).view(U64)[2048] == 0, "ticket not reset"


def _whiten_inputs(N):
    """adv and the two moment records whitening reads: m1 the uncentred pass, m2 the
    pass centred on it (only m1[0], m1[2], m2[1] are read)."""
    adv = _data(N)
    m1, _ = V.moments(adv) if N else (np.array([40.0, 0, 1, 0, 0, 0], F64), None)
    m2, _ = V.moments(adv, m1) if N else (np.array([0, 25.0, 1, 0, 0, 0], F64), None)
    return adv, m1, m2


@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("eps", [1e-6, 1e-8])
def test_whiten(K, st, N, eps):
    """adv32 only, w64 only, both: bitwise the numpy fp64 expression and its f32 rounding;
    one element past the end stays untouched."""
    adv, m1, m2 = _whiten_inputs(N)
    w, a32 = V.whiten(adv, m1, m2, eps)
    advd, m1d, m2d = _dev(adv), _dev(m1), _dev(m2)
    for want32, want64 in ((True, False), (False, True), (True, True)):
        o32 = _dev(np.full(N + 1, NAN32, F32))
        o64 = _dev(np.full(N + 1, NAN64, F64))
        K.mjrl_whiten(advd, N, m1d, m2d, eps, o32 if want32 else None, o64 if want64 else None, st)
        _same(o32, np.concatenate([a32, TAIL32]) if want32 else np.full(N + 1, NAN32, F32), "adv32")
        _same(o64, np.concatenate([w, TAIL64]) if want64 else np.full(N + 1, NAN64, F64), "w64")


@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("eps", [1e-6, 1e-8])
def test_whiten_moments(K, st, N, eps):
    """mjrl_whiten_moments: mjrl_whiten's outputs bitwise (with and without w64), and
    out[6] the moments of the f32 outputs; twice on one rpart."""
    adv, m1, m2 = _whiten_inputs(N)
    w, a32 = V.whiten(adv, m1, m2, eps)
    ref = V.moments(a32)
    advd, m1d, m2d = _dev(adv if N else np.zeros(1)), _dev(m1), _dev(m2)
    rpart = torch.zeros(MOM_SCRATCH, dtype=torch.float64, device=DEV)
    for want64 in (True, False):
        o32 = _dev(np.full(N + 1, NAN32, F32))
        o64 = _dev(np.full(N + 1, NAN64, F64))
        out = _out6()
        K.mjrl_whiten_moments(advd, N, m1d, m2d, eps, o32, o64 if want64 else None, rpart, out, st)
        _same(o32, np.concatenate([a32, TAIL32]), "adv32")
        _same(o64, np.concatenate([w, TAIL64]) if want64 else np.full(N + 1, NAN64, F64), "w64")
        _check_moments(out, ref, N, "whiten_moments out N=%d" % N)
    assert _host(rpart).view(U64)[2048] == 0, "ticket not reset"


@pytest.mark.parametrize("T,T_demo", [(0, 0), (0, 300), (1, 0), (63, 1), (1025, 0), (1025, 4097), (69632, 0),
                                      (524289, 524289)])
def test_dapg_adv(K, st, T, T_demo):
    """float(1e-2 w / (std(w) + 1e-8)) for the T rows, float(1e-2 demo_coef) for the
    demo rows after them, bitwise; T = 0 with and without demo rows."""
    w = (_data(T) - 40.0) / 5.0
    mw1, _ = V.moments(w) if T else (np.array([0, 0, 1.0, 0, 0, 0], F64), None)
    mw2, _ = V.moments(w, mw1) if T else (np.array([0, 1.0, 1.0, 0, 0, 0], F64), None)
    demo_coef = 0.1 * 0.95 ** 7
    want = V.dapg_adv(w, mw1, mw2, T_demo, demo_coef)
    out = _dev(np.full(T + T_demo + 1, NAN32, F32))
    K.mjrl_dapg_adv(_dev(w) if T else None, T, _dev(mw1), _dev(mw2), T_demo, demo_coef, out, st)
    _same(out, np.concatenate([want, TAIL32]), "adv_vpg")


@pytest.mark.parametrize("row_bytes,n,src_rows,offset", [
    (4, 1000, 300, 0), (12, 1000, 300, 0), (16, 1000, 300, 0), (20, 1000, 300, 0), (48, 1000, 300, 0),
    (1504, 1000, 300, 0),              # a Humanoid xhat row: 376 floats, more than a wave of 16-byte words
    (16, 1000, 300, 4), (48, 257, 300, 4),   # 16-byte rows from a base 4 bytes off: the scalar path
    (48, 1, 300, 0), (1504, 1, 5, 0),
    (16, 40000, 777, 0),               # beyond 8,192 workgroups x 4 rows: the grid stride
])
def test_gather_rows(K, st, row_bytes, n, src_rows, offset):
    """dst row i = src row idx[i], indices repeating (n > src_rows); the destination is
    one row longer than n, so an overrun shows."""
    rs = np.random.RandomState(row_bytes + n)
    w = row_bytes // 4
    src = rs.standard_normal(src_rows * w + 4).astype(F32)
    idx = rs.randint(0, src_rows, n).astype(np.int64)
    idx[0] = src_rows - 1
    if n > 2:
        idx[1] = idx[2] = 0
    srcd = _dev(src)
    dst = _dev(np.full((n + 1) * w + 4, NAN32, F32))
    o = offset // 4
    K.mjrl_gather_rows(srcd[o:], row_bytes, _dev(idx), n, dst[o:], st)
    want = np.full((n + 1) * w + 4, NAN32, F32)
    want[o:o + n * w] = src[o:o + src_rows * w].reshape(src_rows, w)[idx].reshape(-1)
    _same(dst, want, "gathered rows")
