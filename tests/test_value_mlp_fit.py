"""The fused value fit's C ABI and Python switch without a GPU: the entry points
are exported and bound, every refusal comes before any launch, the scratch size
is monotonic, fit_backend defaults to torch and survives pickling."""
import ctypes as C
import pickle

import pytest

from mjrl_amd import _lib

NAMES = ("mjrl_value_mlp_scratch", "mjrl_value_mlp_epoch")
FAKE = 4096   # a non-null address no refused call dereferences


@pytest.fixture(scope="module")
def lib():
    import os
    from mjrl_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_entry_points_are_bound(lib):
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert name not in _lib.QUERIES and name not in _lib.STAGE_FUNCS
        assert getattr(_lib.calls(_lib.load), name).errcheck is not None


def full_net(hole=None):
    net = _lib.ValueNet()
    for f, arr in enumerate((net.p, net.exp_avg, net.exp_avg_sq)):
        for i in range(6):
            arr[i] = None if hole == (f, i) else FAKE
    return net


def epoch_args(**kw):
    """A call that would launch; every case below changes one argument."""
    a = dict(X=FAKE, Y=FAKE, T=200, n=5, perm=FAKE, nmb=2, bs=64, net=C.byref(full_net()),
             hp=C.byref(_lib.Adam(1e-3, 0.9, 0.999, 1e-8, 0.0, 0)), scratch=FAKE, grad=None, loss=None, stream=None)
    a.update(kw)
    return tuple(a[k] for k in ("X", "Y", "T", "n", "perm", "nmb", "bs", "net", "hp", "scratch", "grad", "loss",
                                "stream"))


REFUSED = ([dict(bs=0), dict(bs=65), dict(bs=-1), dict(n=0), dict(n=-3), dict(T=-1), dict(nmb=-1),
            dict(hp=C.byref(_lib.Adam(1e-3, 0.9, 0.999, 1e-8, 0.0, -1)))]
           + [{k: None} for k in ("X", "Y", "perm", "net", "hp", "scratch")]
           + [dict(net=C.byref(full_net(hole=(f, i)))) for f in range(3) for i in (0, 3, 5)])


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_bad_arguments_are_refused_before_any_launch(lib, case):
    args = epoch_args(**REFUSED[case])
    assert lib.mjrl_value_mlp_epoch(*args) == _lib.MJRL_EINVAL
    with pytest.raises(_lib.MjrlError, match=r"^mjrl_value_mlp_epoch failed: invalid argument$"):
        _lib.calls(_lib.load).mjrl_value_mlp_epoch(*args)


def test_no_minibatch_is_ok_without_a_launch(lib):
    # nothing is dereferenced or launched: null data pointers are fine
    assert lib.mjrl_value_mlp_epoch(*epoch_args(nmb=0, X=None, Y=None, perm=None, net=None, hp=None,
                                                scratch=None)) == _lib.MJRL_OK
    assert lib.mjrl_value_mlp_epoch(*epoch_args(nmb=0, bs=65)) == _lib.MJRL_EINVAL


def test_scratch_size(lib):
    f = C.c_int64()
    for n, bs in ((0, 64), (5, 0), (5, 65), (-1, 1)):
        assert lib.mjrl_value_mlp_scratch(n, bs, C.byref(f)) == _lib.MJRL_EINVAL
    assert lib.mjrl_value_mlp_scratch(5, 64, None) == _lib.MJRL_EINVAL
    with pytest.raises(_lib.MjrlError, match=r"^mjrl_value_mlp_scratch failed"):
        _lib.calls(_lib.load).mjrl_value_mlp_scratch(5, 65, f)
    prev_n = 0
    for n in (1, 2, 3, 12, 13, 60, 376, 377, 1000, 5000):
        prev = 0
        for bs in (1, 2, 15, 16, 17, 33, 63, 64):
            assert lib.mjrl_value_mlp_scratch(n, bs, C.byref(f)) == _lib.MJRL_OK
            assert f.value >= 3 * 64 * 128 + 1 and f.value >= prev   # a0, g0, g1 and the loss
            prev = f.value
        assert prev >= prev_n
        prev_n = prev


def test_fit_backend_default_and_pickling():
    from mjrl_amd.baselines.mlp_baseline import MLPBaseline
    from mjrl_amd.utils.gym_env import EnvSpec
    assert MLPBaseline.fit_backend == "torch"
    b = MLPBaseline(EnvSpec(5, 2, 300, 1))
    assert b.fit_backend == "torch" and "fit_backend" not in b.__dict__
    assert pickle.loads(pickle.dumps(b)).fit_backend == "torch"
    b.fit_backend = "hip"
    c = pickle.loads(pickle.dumps(b))
    assert c.fit_backend == "hip" and c._dev is None
    assert MLPBaseline.fit_backend == "torch"
