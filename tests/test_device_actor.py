"""The device actor without a GPU: Philox4x32-10 against Random123's known answers,
the properties of the NumPy statement of the action noise (noise_reference: what
the kernel is compared with in test_gpu_device_actor.py), its moments, and the
argument checks of DeviceActor / DeviceRollout / mjrl_policy_act, none of which
needs the GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mjrl_amd.samplers import device_actor as DA


# ---- Philox4x32-10: Random123's kat_vectors ----

@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = DA.philox4x32(counter, key)
    assert all(x.dtype == np.uint32 for x in got)
    assert " ".join("%08x" % int(x) for x in got) == want
    # vectorised: the same words at every position of an array of counters
    arr = DA.philox4x32([np.full((3, 2), c, dtype=np.uint32) for c in counter], key)
    assert all(a.shape == (3, 2) and np.all(a == g) for a, g in zip(arr, got))


# ---- noise_reference ----

MS = (1, 3, 4, 5, 17, 40)


@pytest.mark.parametrize("m", MS)
def test_noise_shape_range_and_sub_batches(m):
    full = DA.noise_reference(9, 3, 0, 12, m)
    assert full.shape == (12, m) and full.dtype == np.float32 and full.flags.c_contiguous
    assert np.all(np.abs(full) <= 5.78) and np.all(np.isfinite(full))
    part = DA.noise_reference(9, 3, 5, 7, m)
    assert part.tobytes() == full[5:12].tobytes()
    # a narrower action space is a prefix of the columns
    assert DA.noise_reference(9, 3, 0, 12, 40)[:, :m].tobytes() == full.tobytes()
    assert DA.noise_reference(9, 3, 0, 0, m).shape == (0, m)


def test_noise_depends_on_step_seed_and_their_high_words():
    base = DA.noise_reference(9, 3, 0, 12, 6)
    rows = {base.tobytes()}
    for seed, step in [(9, 4), (10, 3), (9 + (1 << 32), 3), (9, 3 + (1 << 32)), (9 + (5 << 40), 3 + (7 << 35))]:
        rows.add(DA.noise_reference(seed, step, 0, 12, 6).tobytes())
    assert len(rows) == 6
    # the high words are used, not dropped: clearing them gives the base rows back
    assert DA.noise_reference((9 + (1 << 32)) & 0xffffffff, (3 + (1 << 32)) & 0xffffffff, 0, 12, 6).tobytes() \
        == base.tobytes()
    # rows of one call differ from each other, and so do the blocks of a row
    assert len({r.tobytes() for r in base}) == 12
    wide = DA.noise_reference(9, 3, 0, 2, 40)
    assert len({wide[0, 4 * b:4 * b + 4].tobytes() for b in range(10)}) == 10
    with pytest.raises(ValueError, match="step"):
        DA.noise_reference(9, -1, 0, 4, 2)


def _lag1(x, axis):
    a = np.take(x, range(x.shape[axis] - 1), axis=axis).ravel()
    b = np.take(x, range(1, x.shape[axis]), axis=axis).ravel()
    return float(np.corrcoef(a, b)[0, 1]) * np.sqrt(a.size)


@pytest.mark.parametrize("seed,E,m,steps", [(123, 257, 17, 16), (7, 1024, 6, 8), (2026, 64, 40, 16)])
def test_noise_moments(seed, E, m, steps):
    """Six statistics of the noise over steps 0 .. steps - 1, each within 4 standard
    errors of a standard normal sample of independent entries."""
    x = np.stack([DA.noise_reference(seed, t, 0, E, m) for t in range(steps)]).astype(np.float64)   # [steps][E][m]
    N = x.size
    mean, var = x.mean(), x.var()
    kurt = np.mean((x - mean) ** 4) / var ** 2 - 3.0
    z = dict(mean=abs(mean) * np.sqrt(N), var=abs(var - 1.0) / np.sqrt(2.0 / N), kurt=abs(kurt) / np.sqrt(24.0 / N),
             lag_env=abs(_lag1(x, 1)), lag_step=abs(_lag1(x, 0)), lag_col=abs(_lag1(x, 2)))
    print("moments (seed %d, E %d, m %d, steps %d):" % (seed, E, m, steps),
          " ".join("%s=%.2f" % kv for kv in z.items()))
    for k, v in z.items():
        assert v < 4.0, (k, v)


# ---- argument checks: before the GPU library is loaded ----

class _Policy:
    """What the checks read of a policy."""
    n, m, min_log_std = 8, 2, -3


def test_act_argument_checks_need_no_gpu():
    actor = DA.DeviceActor(_Policy(), seed=5)
    f32 = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="obs is a CPU tensor"):
        actor.act(f32)
    with pytest.raises(ValueError, match=r"obs must be \[E\]\[n = 8\]"):
        actor.act(torch.zeros(4, 9))
    with pytest.raises(ValueError, match=r"obs must be \[E\]\[n = 8\]"):
        actor.act(torch.zeros(8))
    with pytest.raises(ValueError, match="obs must be float32 or float64"):
        actor.act(torch.zeros(4, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="obs must be a torch tensor"):
        actor.act(np.zeros((4, 8), np.float32))
    assert actor._bp is None and actor.step == 0   # nothing was built, no step was spent
    with pytest.raises(ValueError, match="seed"):
        DA.DeviceActor(_Policy(), seed=-1)


def test_rollout_argument_and_misuse_checks_need_no_gpu():
    ro = DA.DeviceRollout(_Policy(), E=5, H=2, device="cpu", seed=1)
    assert ro.observations.shape == (2, 5, 8) and ro.actions.shape == (2, 5, 2)
    assert ro.rewards.dtype == torch.float64 and ro.done.dtype == ro.terminated.dtype == torch.uint8
    with pytest.raises(ValueError, match="obs is a CPU tensor"):
        ro.act(torch.zeros(5, 8))
    with pytest.raises(ValueError, match=r"obs must be \[E = 5\]\[n = 8\]"):
        ro.act(torch.zeros(4, 8))
    with pytest.raises(ValueError, match="rollout's dtype"):
        ro.act(torch.zeros(5, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="record: step 0 has no actions yet"):
        ro.record(torch.zeros(5), torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="tensors: the rollout has 0 of H = 2"):
        ro.tensors()
    ro._acted = True   # as after an act()
    with pytest.raises(ValueError, match="already has its actions"):
        ro.act(torch.zeros(5, 8))
    with pytest.raises(ValueError, match=r"rewards must be a torch tensor \[E = 5\]"):
        ro.record(torch.zeros(4), torch.zeros(5, dtype=torch.uint8))
    ro.record(torch.arange(5.0), torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8))
    assert ro.t == 1 and ro.rewards[0].tolist() == [0, 1, 2, 3, 4]
    assert ro.terminated[0].tolist() == ro.done[0].tolist() == [0, 1, 0, 0, 1]   # terminated=None: every end is one
    ro._acted = True
    ro.record(torch.zeros(5), torch.ones(5, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8))
    assert ro.terminated[1].tolist() == [0] * 5 and ro.done[1].tolist() == [1] * 5
    with pytest.raises(ValueError, match="the rollout is full"):
        ro.act(torch.zeros(5, 8))
    assert len(ro.tensors()) == 5
    ro.reset()
    assert ro.t == 0 and ro.actor._bp is None
    with pytest.raises(ValueError, match="E >= 1"):
        DA.DeviceRollout(_Policy(), E=0, H=2, device="cpu")
    with pytest.raises(ValueError, match="float32 or float64"):
        DA.DeviceRollout(_Policy(), E=2, H=2, device="cpu", dtype=torch.float16)


def test_the_module_and_the_package_export_without_loading_the_library():
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import sys; import mjrl_amd.samplers as S; from mjrl_amd import _lib; "
            "assert S.DeviceActor and S.DeviceRollout and _lib._LIB is None and not _lib._CALLS; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ---- the entry point's own argument checks: before any launch ----

@pytest.fixture(scope="module")
def lib():
    from mjrl_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _act_args(s, obs, obs_f64, E, packed, step, act):
    return (s, obs, obs_f64, E, packed, None, None, None, None, None, 0, step, 0, act, None, None, None, None)


def test_policy_act_null_arguments_fail_loudly(lib):
    from mjrl_amd import _lib
    s = C.byref(_lib.make_shape(8, 2, 64, 64))
    p = C.c_void_p(256)   # never dereferenced: validation happens before any launch
    assert lib.mjrl_policy_act(*_act_args(s, None, 0, 4, p, 0, p)) == _lib.MJRL_EINVAL      # obs
    assert lib.mjrl_policy_act(*_act_args(s, p, 0, 4, p, 0, None)) == _lib.MJRL_EINVAL      # act
    assert lib.mjrl_policy_act(*_act_args(s, p, 0, 4, None, 0, p)) == _lib.MJRL_EINVAL      # packed_theta
    assert lib.mjrl_policy_act(*_act_args(None, p, 0, 4, p, 0, p)) == _lib.MJRL_EINVAL      # shape
    assert lib.mjrl_policy_act(*_act_args(s, p, 0, -1, p, 0, p)) == _lib.MJRL_EINVAL        # E < 0
    assert lib.mjrl_policy_act(*_act_args(s, p, 0, 4, p, -1, p)) == _lib.MJRL_EINVAL        # step < 0
    assert lib.mjrl_policy_act(*_act_args(s, p, 2, 4, p, 0, p)) == _lib.MJRL_EINVAL         # obs_f64
    assert lib.mjrl_policy_act(*_act_args(s, p, -1, 4, p, 0, p)) == _lib.MJRL_EINVAL
    half = list(_act_args(s, p, 0, 4, p, 0, p))
    half[5] = p                                                                               # in_shift without in_scale
    assert lib.mjrl_policy_act(*half) == _lib.MJRL_EINVAL
    assert lib.mjrl_policy_act(*_act_args(s, None, 0, 0, p, 0, None)) == _lib.MJRL_OK       # E == 0: no launch


def test_policy_act_checked_handle_raises_with_the_entry_name(lib):
    from mjrl_amd import _lib
    K = _lib.calls(_lib.load)
    s = _lib.make_shape(8, 2, 64, 64)
    with pytest.raises(_lib.MjrlError, match=r"^mjrl_policy_act failed: invalid argument$"):
        K.mjrl_policy_act(*_act_args(s, None, 0, 4, None, 0, None))
    assert "mjrl_policy_act" not in _lib.QUERIES
