"""The MLPBaseline value features of the streamed staging, without a GPU: the two
entry points (mjrl_value_features_slots, mjrl_value_features_finish) refuse bad
arguments before any launch, and the stub trajectories the GPU tests
(test_gpu_value_features.py) sample discriminate: features built from f32-rounded
observations differ from float32(clip(x) / 10) of the f64 values, so a sink that
formed them from its f32 rows would fail there."""
import ctypes as C
import os

import numpy as np
import pytest

# the sampling of the GPU tests: 37 stub trajectories on 8 slots
STUB = dict(N=37, num_envs=8, pegasus_seed=7, policy_seed=4)


def feat_f64(x):
    """The reference's observation features (mlp_baseline.py:37-56, 108)."""
    return (np.clip(np.asarray(x, np.float64), -10, 10) / 10.0).astype(np.float32)


def feat_via_f32(x):
    """The same from the f32 image of x: what f32-staged rows could give."""
    return feat_f64(np.asarray(x, np.float64).astype(np.float32).astype(np.float64))


def discriminating_elements(paths):
    """How many observation elements of paths give other feature bits through f32."""
    o = np.concatenate([p["observations"] for p in paths])
    return int(np.sum(feat_f64(o).view(np.uint32) != feat_via_f32(o).view(np.uint32)))


@pytest.fixture(scope="module")
def lib():
    from mjrl_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _cases(names, ok, bads):
    for bad in bads:
        yield bad, [bad.get(k, v) for k, v in zip(names, ok)]


P = C.c_void_p(64)
SLOTS_NAMES = ("obs", "live", "dest", "E", "S", "n", "cap", "feat", "stream")
SLOTS_OK = (P, P, P, 3, 8, 6, 100, P, None)
SLOTS_BAD = (dict(E=-1), dict(S=-1, E=0), dict(E=9), dict(n=0), dict(n=-3), dict(cap=-1), dict(obs=None),
             dict(live=None), dict(dest=None), dict(feat=None))
FINISH_NAMES = ("pad", "src", "T", "n", "cap", "H", "tab", "out", "stream")
FINISH_OK = (P, P, 5, 6, 100, 40, P, P, None)
FINISH_BAD = (dict(T=-1), dict(n=0), dict(n=-1), dict(cap=-1), dict(H=0), dict(H=-4), dict(pad=None), dict(tab=None),
              dict(out=None), dict(src=None, T=101))   # identity rows past the slab


def test_entry_points_validate_before_any_launch(lib):
    from mjrl_amd import _lib
    for name, names, ok, bads in (("mjrl_value_features_slots", SLOTS_NAMES, SLOTS_OK, SLOTS_BAD),
                                  ("mjrl_value_features_finish", FINISH_NAMES, FINISH_OK, FINISH_BAD)):
        raw, checked = getattr(lib, name), getattr(_lib.calls(_lib.load), name)
        for bad, args in _cases(names, ok, bads):
            assert raw(*args) == _lib.MJRL_EINVAL, (name, bad)
            with pytest.raises(_lib.MjrlError, match=r"^%s failed: invalid argument$" % name):
                checked(*args)
    # nothing to do: MJRL_OK without a launch, null pointers allowed
    for f in (lib.mjrl_value_features_slots, _lib.calls(_lib.load).mjrl_value_features_slots):
        assert f(P, P, P, 0, 8, 6, 100, P, None) == _lib.MJRL_OK
        assert f(None, None, None, 0, 0, 6, 0, None, None) == _lib.MJRL_OK
    for f in (lib.mjrl_value_features_finish, _lib.calls(_lib.load).mjrl_value_features_finish):
        assert f(P, P, 0, 6, 100, 40, P, P, None) == _lib.MJRL_OK
        assert f(None, None, 0, 6, 0, 40, None, None, None) == _lib.MJRL_OK


def test_both_take_a_stream_and_are_status_checked():
    from mjrl_amd import _lib
    for name in ("mjrl_value_features_slots", "mjrl_value_features_finish"):
        assert name in _lib.SIGNATURES and name not in _lib.QUERIES and name not in _lib.STAGE_FUNCS


def test_feature_arithmetic_discriminates_on_edge_values():
    """The rounding the device kernel must reproduce: of the f64 value, not of its
    f32 image; np.clip's treatment of -0.0, NaN and the clip edges."""
    x = np.random.RandomState(0).randn(4096) * 5
    assert np.any(feat_f64(x).view(np.uint32) != feat_via_f32(x).view(np.uint32))
    assert np.signbit(feat_f64(-0.0)) and np.isnan(feat_f64(np.nan))
    assert feat_f64(np.nextafter(10.0, np.inf)) == 1.0 and feat_f64(-1e300) == -1.0


@pytest.mark.parametrize("ragged", [True, False])
def test_stub_trajectories_discriminate(ragged):
    """The observations of the stub trajectories at the GPU tests' seeds (the
    reference's serial rollout here: the same environment streams, the first row of
    every trajectory bit for bit the vector sampler's) are not f32 values, and
    rounding them to f32 first changes feature bits."""
    import functools
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    from stub_env import StubEnv, serial_rollout
    env = StubEnv if ragged else functools.partial(StubEnv, radius=1e9)
    policy = MLP(EnvSpec(6, 2, 40, 1), hidden_sizes=(32, 32), seed=STUB["policy_seed"], init_log_std=-0.5)
    paths = serial_rollout(STUB["N"], policy, 1e6, env, STUB["pegasus_seed"])
    assert (len(set(len(p["rewards"]) for p in paths)) > 1) == ragged
    assert discriminating_elements(paths) >= 1
    first = [dict(observations=p["observations"][:1]) for p in paths]
    assert discriminating_elements(first) >= 1
