"""The C-ABI library loads and exports every entry point include/mjrl_amd.h
declares; the host-only entry points (shape / scratch sizing) work without a GPU."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mjrl_amd.h")


def declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(mjrl_\w+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from mjrl_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_every_declared_symbol_is_exported(lib):
    from mjrl_amd import _lib
    names = declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    # and every binding the Python side declares exists in the header
    assert set(_lib.SIGNATURES) <= set(names)
    assert set(names) <= set(_lib.SIGNATURES), set(names) - set(_lib.SIGNATURES)


def test_stage_lib_exports_every_host_entry_point(lib):
    """The host-only lib/libmjrl_stage.so carries every mjrl_host_* entry point the
    header declares (the pool controller loads only it)."""
    from mjrl_amd import _lib
    host = [n for n in declared() if n.startswith("mjrl_host_")]
    assert set(host) == set(_lib.STAGE_FUNCS)
    S = _lib.stage_lib()
    for n in host:
        assert hasattr(S, n), n


@pytest.mark.parametrize("n,m,h,np_,mp,d", [
    (6, 2, (0, 0), 16, 16, 16),            # point_mass, linear policy
    (8, 2, (64, 64), 16, 16, 4868),        # swimmer
    (17, 6, (128, 128), 32, 16, 19596),    # halfcheetah
    (376, 17, (64, 64), 384, 32, 29410),   # humanoid
    (39, 28, (256, 256), 48, 32, 83256),   # door
    (15, 40, (32, 32), 16, 64, 15 * 32 + 32 + 32 * 32 + 32 + 40 * 32 + 40 + 40),
])
def test_shape_padding(lib, n, m, h, np_, mp, d):
    from mjrl_amd import _lib
    s = _lib.make_shape(n, m, h[0], h[1])
    assert (s.np, s.mp, s.d) == (np_, mp, d)
    assert s.np >= n + 1 and s.np % 16 == 0        # bias column always present
    wf, rd, sl = C.c_int64(), C.c_int64(), C.c_int32()
    assert lib.mjrl_scratch_size(C.byref(s), 1000000, C.byref(wf), C.byref(rd), C.byref(sl)) == 0
    assert 1 <= sl.value <= 256 and wf.value > 0 and rd.value > 0


@pytest.mark.parametrize("n,m,h", [(6, 2, (0, 0)), (8, 2, (64, 64)), (17, 6, (128, 128)), (376, 17, (64, 64)),
                                   (39, 28, (256, 256)), (15, 40, (32, 32)), (45, 24, (128, 128))])
def test_scratch_size_is_monotonic(lib, n, m, h):
    """A scratch sized by mjrl_scratch_size for T rows must hold every pass over
    T' <= T rows (the engine sizes it once for the batch, then runs FVPs over the
    RL rows only, subsampled rows, ...): sizes and slice counts never shrink as T
    grows, over the tile-count boundaries of every kernel's grid."""
    from mjrl_amd import _lib
    s = _lib.make_shape(n, m, h[0], h[1])
    prev_w, prev_s = 0, 0
    Ts = sorted(set([1, 15, 16, 17, 31, 32, 33, 63, 64, 65] + [k * 16 + d for k in range(1, 1200, 7) for d in (-1, 0, 1)]
                    + [b * t + d for b in (16, 32, 64) for t in (128, 256) for d in (-1, 0, 1, b, b + 1)]
                    + [8192 * 32 + d for d in (-33, -1, 0, 1, 33)] + [1000000, 1000001]))
    for T in Ts:
        wf, rd, sl = C.c_int64(), C.c_int64(), C.c_int32()
        assert lib.mjrl_scratch_size(C.byref(s), T, C.byref(wf), C.byref(rd), C.byref(sl)) == 0
        assert wf.value >= prev_w and sl.value >= prev_s, T
        prev_w, prev_s = wf.value, sl.value


def test_unsupported_shape_is_rejected(lib):
    from mjrl_amd import _lib
    s = _lib.Shape()
    assert lib.mjrl_shape_init(C.byref(s), 10, 3, 48, 48) == _lib.MJRL_ESHAPE
    assert lib.mjrl_shape_init(C.byref(s), 0, 3, 64, 64) == _lib.MJRL_EINVAL
    with pytest.raises(_lib.MjrlError):
        _lib.make_shape(10, 100, 64, 64)


def test_null_arguments_fail_loudly(lib):
    from mjrl_amd import _lib
    s = _lib.make_shape(8, 2, 64, 64)
    # argument validation happens before any launch: no GPU needed
    assert lib.mjrl_pack_batch(None, None, 10, C.byref(s), None, None, None, None, None) == _lib.MJRL_EINVAL
    assert lib.mjrl_gae(None, None, None, None, 5, 0.99, 0.97, 1, None, None, None, None) == _lib.MJRL_EINVAL
    assert lib.mjrl_policy_fvp(C.byref(s), None, 10, None, None, None, None, None, None, None) == _lib.MJRL_EINVAL
    assert lib.mjrl_gather_rows(None, 16, None, 4, None, None) == _lib.MJRL_EINVAL
    assert lib.mjrl_gather_rows(C.c_void_p(16), 6, C.c_void_p(16), 4, C.c_void_p(16), None) == _lib.MJRL_EINVAL
    assert lib.mjrl_gather_rows(None, 16, None, 0, None, None) == _lib.MJRL_OK


@pytest.fixture(scope="module")
def calls(lib):
    """The checked handle, obtained as `lib` obtains the raw one: no GPU refusal."""
    from mjrl_amd import _lib
    return _lib.calls(_lib.load)


def test_checked_null_arguments_raise_with_the_entry_name(calls):
    """test_null_arguments_fail_loudly's four calls through the checked handle:
    MjrlError, named after the entry point from the table (not by the caller)."""
    from mjrl_amd import _lib
    s = _lib.make_shape(8, 2, 64, 64)
    for name, args in [
            ("mjrl_pack_batch", (None, None, 10, C.byref(s), None, None, None, None, None)),
            ("mjrl_gae", (None, None, None, None, 5, 0.99, 0.97, 1, None, None, None, None)),
            ("mjrl_policy_fvp", (C.byref(s), None, 10, None, None, None, None, None, None, None)),
            ("mjrl_gather_rows", (None, 16, None, 4, None, None))]:
        with pytest.raises(_lib.MjrlError, match=r"^%s failed: invalid argument$" % name):
            getattr(calls, name)(*args)
    assert calls.mjrl_gather_rows(None, 16, None, 0, None, None) == _lib.MJRL_OK


def test_checked_pointer_slots_convert(calls, lib):
    """A P slot takes a torch.Tensor (its data_ptr()), a c_void_p, an int or None;
    a POINTER(struct) slot the structure itself or a byref."""
    import torch
    from mjrl_amd import _lib
    t = torch.zeros(64)
    assert calls.mjrl_gather_rows(t, 16, None, 0, t, None) == _lib.MJRL_OK   # returns before any launch
    assert calls.mjrl_gather_rows(t[8:], 16, None, 0, C.c_void_p(t.data_ptr()), None) == _lib.MJRL_OK
    assert calls.mjrl_gather_rows(t.data_ptr(), 16, None, 0, t, None) == _lib.MJRL_OK
    with pytest.raises(_lib.MjrlError, match="mjrl_gather_rows"):   # row bytes no multiple of 4
        calls.mjrl_gather_rows(16, 6, C.c_void_p(16), 4, 16, None)
    bare, ref = _lib.Shape(), _lib.Shape()
    calls.mjrl_shape_init(bare, 376, 17, 64, 64)
    calls.mjrl_shape_init(C.byref(ref), 376, 17, 64, 64)
    assert bytes(bare) == bytes(ref) == bytes(_lib.make_shape(376, 17, 64, 64))
    wf, rd, sl = C.c_int64(), C.c_int64(), C.c_int32()
    calls.mjrl_scratch_size(bare, 1000, wf, rd, C.byref(sl))
    wf2, rd2, sl2 = C.c_int64(), C.c_int64(), C.c_int32()
    assert lib.mjrl_scratch_size(C.byref(ref), 1000, C.byref(wf2), C.byref(rd2), C.byref(sl2)) == 0
    assert (wf.value, rd.value, sl.value) == (wf2.value, rd2.value, sl2.value) and sl.value >= 1


def test_query_entry_points_are_not_status_checked(calls, lib):
    """_lib.QUERIES are exactly the header's entry points whose documented result
    is an answer, not a status; they return it through the checked handle as
    through the raw one, and every other entry point carries the errcheck."""
    from mjrl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    # in the header: the declarations with nowhere to put a result but the return
    # value (no stream to launch on, every pointer parameter const); their comments
    # document that value (the build flags, 1 / 0, the accumulate path)
    answers = set()
    for name, params in re.findall(r"\bint\s+(mjrl_\w+)\s*\(([^)]*)\)\s*;", src):
        ptrs = [p for p in params.split(",") if "*" in p]
        if all(p.strip().startswith("const ") for p in ptrs) and "stream" not in params:
            answers.add(name)
    assert answers == set(_lib.QUERIES), (sorted(answers), _lib.QUERIES)
    s = _lib.make_shape(376, 17, 64, 64)
    for name in ("mjrl_fused_path", "mjrl_split_supported"):
        assert getattr(calls, name)(s) == getattr(lib, name)(C.byref(s))
    assert calls.mjrl_fused_path(s) != 0   # an answer a blanket errcheck would have raised on
    assert calls.mjrl_build_flags() == lib.mjrl_build_flags()
    for name in _lib.SIGNATURES:
        assert (getattr(calls, name).errcheck is None) == (name in _lib.QUERIES), name


def test_checked_host_call_takes_numpy_arrays():
    """A checked host-library call with numpy arrays is bit-equal to the raw call
    with their .ctypes.data."""
    import numpy as np
    from mjrl_amd import _lib
    src = np.random.RandomState(0).randn(5, 8) * 3
    outs = []
    for checked in (False, True):
        dst = np.zeros((5, 8), np.float32)
        lo, hi = np.full(8, np.inf, np.float32), np.full(8, -np.inf, np.float32)
        if checked:
            assert _lib.stage_calls().mjrl_host_stage_f64(src, 5, 8, dst, lo, hi) == 0
        else:
            assert _lib.stage_lib().mjrl_host_stage_f64(src.ctypes.data, 5, 8, dst.ctypes.data, lo.ctypes.data,
                                                        hi.ctypes.data) == 0
        outs.append((dst, lo, hi))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(outs[0][0], src.astype(np.float32))
    # a ctypes array of pointers, and an int passed as the whole 64-bit address
    back = np.zeros_like(src)
    S = _lib.stage_calls()
    S.mjrl_host_gather((C.c_void_p * 1)(src.ctypes.data), (C.c_int64 * 1)(src.nbytes), 1, back.ctypes.data)
    assert back.tobytes() == src.tobytes()
    with pytest.raises(_lib.MjrlError, match="mjrl_host_gather"):
        _lib.stage_calls().mjrl_host_gather(None, None, -1, None)


def test_no_gpu_means_no_compute():
    """On a host without a GPU the product path refuses to run (no CPU fallback)."""
    import torch
    from mjrl_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.MjrlError):
        _lib.lib()
