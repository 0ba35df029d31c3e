"""The row-tiled policy fit's C ABI and Python switch without a GPU (csrc/policy_fit_rows.hip,
mjrl_policy_fit_rows_epoch; PPO.fit_backend / BC.fit_backend = "hip_rows"): the entry points
are exported and bound, every refusal comes before any launch, the scratch holds a gradient
per row tile and never shrinks as the minibatch grows, check_fit_backend takes minibatches of
1..16384 rows at the narrow backend's widths, the attribute survives pickling, and the MSE
fit refuses the name before anything touches the GPU library."""
import ctypes as C
import pickle

import pytest

from mjrl_amd import _lib
from test_policy_fit import FAKE, _expert, _never, _policy, _ppo, fit_data, full_net

NAMES = ("mjrl_policy_fit_rows_scratch", "mjrl_policy_fit_rows_epoch")
MAX_BS = 16384


@pytest.fixture(scope="module")
def lib():
    import os
    from mjrl_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_entry_points_are_bound(lib):
    assert _lib.POLICY_FIT_ROWS_MAX_BS == MAX_BS
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert name not in _lib.QUERIES and name not in _lib.STAGE_FUNCS
        assert getattr(_lib.calls(_lib.load), name).errcheck is not None
    # mjrl_policy_fit_epoch's signature without steps_per_launch
    sig = list(_lib.SIGNATURES["mjrl_policy_fit_epoch"])
    del sig[7]
    assert _lib.SIGNATURES["mjrl_policy_fit_rows_epoch"] == sig
    assert _lib.SIGNATURES["mjrl_policy_fit_rows_scratch"] == _lib.SIGNATURES["mjrl_policy_fit_scratch"]


def epoch_args(data=(), **kw):
    """A call that would launch; data: field changes of fit_data, or None for a null structure."""
    a = dict(data=None if data is None else C.byref(fit_data(**dict(data))), idx=FAKE, nmb=2, bs=130,
             net=C.byref(full_net()), hp=C.byref(_lib.Adam(1e-3, 0.9, 0.999, 1e-8, 0.0, 0)), scratch=FAKE,
             grad=None, loss=None, stream=None)
    a.update(kw)
    return tuple(a[k] for k in ("data", "idx", "nmb", "bs", "net", "hp", "scratch", "grad", "loss", "stream"))


# mjrl_policy_fit_epoch's table (test_policy_fit.REFUSED) with the row bound at 16384 and no steps_per_launch
REFUSED = ([dict(bs=0), dict(bs=MAX_BS + 1), dict(bs=-1), dict(nmb=-1), dict(data=None),
            dict(hp=C.byref(_lib.Adam(1e-3, 0.9, 0.999, 1e-8, 0.0, -1)))]
           + [{k: None} for k in ("idx", "net", "hp", "scratch")]
           + [dict(data={k: v}) for k, v in (("n", 0), ("n", -3), ("n", (1 << 24) + 1), ("m", 0), ("m", 65),
                                             ("h0", 0), ("h0", 65), ("h1", 0), ("h1", 65), ("T", -1), ("kind", 2),
                                             ("kind", -1))]
           + [dict(data={k: None}) for k in ("obs", "act", "adv", "in_shift", "in_scale", "out_shift", "out_scale")]
           # PPO: exactly one of ll_old and old_log_std
           + [dict(data=dict(ll_old=None)), dict(data=dict(old_log_std=FAKE))]
           + [dict(data=dict(kind=_lib.POLICY_FIT_BC, obs=None))]
           + [dict(net=C.byref(full_net(hole=(f, i)))) for f in range(3) for i in (0, 3, 6)])


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_bad_arguments_are_refused_before_any_launch(lib, case):
    args = epoch_args(**dict(REFUSED[case]))
    assert lib.mjrl_policy_fit_rows_epoch(*args) == _lib.MJRL_EINVAL
    with pytest.raises(_lib.MjrlError, match=r"^mjrl_policy_fit_rows_epoch failed: invalid argument$"):
        _lib.calls(_lib.load).mjrl_policy_fit_rows_epoch(*args)


def test_no_minibatch_is_ok_without_a_launch(lib):
    # nothing is dereferenced or launched: null row pointers are fine
    nothing = dict(obs=None, act=None, adv=None, in_shift=None, in_scale=None, out_shift=None, out_scale=None)
    for bs in (1, 64, 65, MAX_BS):
        assert lib.mjrl_policy_fit_rows_epoch(*epoch_args(data=nothing, nmb=0, bs=bs, idx=None, net=None, hp=None,
                                                          scratch=None)) == _lib.MJRL_OK
    assert lib.mjrl_policy_fit_rows_epoch(*epoch_args(data=dict(kind=_lib.POLICY_FIT_BC, ll_old=None, adv=None),
                                                      nmb=0)) == _lib.MJRL_OK
    assert lib.mjrl_policy_fit_rows_epoch(*epoch_args(nmb=0, bs=MAX_BS + 1)) == _lib.MJRL_EINVAL
    assert lib.mjrl_policy_fit_rows_epoch(*epoch_args(data=dict(h0=65), nmb=0)) == _lib.MJRL_EINVAL


def test_scratch_size(lib):
    f = C.c_int64()
    for n, m, h0, h1, bs in ((0, 2, 32, 32, 64), (6, 0, 32, 32, 64), (6, 65, 32, 32, 64), (6, 2, 0, 32, 64),
                             (6, 2, 65, 32, 64), (6, 2, 32, 0, 64), (6, 2, 32, 65, 64), (6, 2, 32, 32, 0),
                             (6, 2, 32, 32, -1), (6, 2, 32, 32, MAX_BS + 1), (-1, 2, 32, 32, 1)):
        assert lib.mjrl_policy_fit_rows_scratch(n, m, h0, h1, bs, C.byref(f)) == _lib.MJRL_EINVAL
    assert lib.mjrl_policy_fit_rows_scratch(6, 2, 32, 32, 64, None) == _lib.MJRL_EINVAL
    with pytest.raises(_lib.MjrlError, match=r"^mjrl_policy_fit_rows_scratch failed"):
        _lib.calls(_lib.load).mjrl_policy_fit_rows_scratch(6, 2, 32, 32, MAX_BS + 1, f)
    for n, m, h0, h1 in ((1, 1, 1, 1), (6, 2, 32, 32), (39, 28, 64, 48), (376, 17, 64, 64), (5000, 64, 64, 64)):
        d = h0 * n + h0 + h1 * h0 + h1 + m * h1 + m + m
        prev = 0
        for bs in (1, 64, 65, 128, 129, 4096, MAX_BS):
            assert lib.mjrl_policy_fit_rows_scratch(n, m, h0, h1, bs, C.byref(f)) == _lib.MJRL_OK
            assert f.value >= -(-bs // 64) * d + 1 and f.value >= prev   # a gradient a tile, and the loss
            assert f.value % 4 == 0
            prev = f.value


# ---- the classes ------------------------------------------------------------------------------
def test_check_fit_backend():
    import torch
    from mjrl_amd.algos import _device_sgd as S
    assert S.POLICY_FIT_BACKENDS == ("torch", "hip", "hip_wide")
    assert S.ROWS_BACKEND == "hip_rows" and S.HIP_ROWS_MAX_BATCH == MAX_BS
    pol = _policy()
    opt = torch.optim.Adam(pol.trainable_params, lr=1e-3)
    for mb in (1, 65, MAX_BS):
        assert S.check_fit_backend("PPO", "hip_rows", pol, opt, mb, "cuda:0") is True
    for mb in (0, MAX_BS + 1):
        with pytest.raises(ValueError, match=r'PPO.fit_backend = "hip_rows" takes minibatches of 1\.\.16384 rows'):
            S.check_fit_backend("PPO", "hip_rows", pol, opt, mb, "cuda:0")
    for hidden in ((65, 32), (32, 65), (64, 256)):
        wide = _policy(hidden)
        with pytest.raises(ValueError, match=r"1\.\.64 units"):
            S.check_fit_backend("BC", "hip_rows", wide, torch.optim.Adam(wide.trainable_params), 256, "cuda:0")
    with pytest.raises(ValueError, match="GPU"):
        S.check_fit_backend("BC", "hip_rows", pol, opt, 256, "cpu")
    with pytest.raises(ValueError, match="torch.optim.Adam"):
        S.check_fit_backend("BC", "hip_rows", pol, torch.optim.SGD(pol.trainable_params, lr=1e-3), 256, "cuda:0")
    mean = torch.optim.Adam(pol.model.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="MSE head has no row-tiled kernel"):
        S.check_fit_backend("BC", "hip_rows", pol, mean, 64, "cuda:0", mean_only=True)
    # the other backends keep their ranges
    with pytest.raises(ValueError, match=r'PPO.fit_backend = "hip" takes minibatches of 1\.\.64 rows, not 65'):
        S.check_fit_backend("PPO", "hip", pol, opt, 65, "cuda:0")
    with pytest.raises(ValueError, match=r'PPO.fit_backend = "hip_wide" takes minibatches of 1\.\.64 rows, not 65'):
        S.check_fit_backend("PPO", "hip_wide", pol, opt, 65, "cuda:0")
    with pytest.raises(ValueError, match="fit_backend must be one of"):
        S.check_fit_backend("PPO", "hip_cols", pol, opt, 64, "cuda:0")


def test_fit_backend_survives_pickling():
    from mjrl_amd.algos.behavior_cloning import BC
    from mjrl_amd.algos.ppo_clip import PPO
    for agent in (_ppo(mb_size=256), BC(_expert(), _policy(), batch_size=256)):
        agent.fit_backend = "hip_rows"
        agent._trainer = object()   # whatever it holds is dropped
        c = pickle.loads(pickle.dumps(agent))
        assert c.fit_backend == "hip_rows" and c._trainer is None and c.mb_size == 256
    assert PPO.fit_backend == "torch" and BC.fit_backend == "torch"


def test_the_aliasing_rule_holds_for_the_rows_backend(monkeypatch):
    """PPO._check_backend treats "hip_rows" as a fused backend: a half-shared policy is refused."""
    from mjrl_amd.comm import LocalComm
    from test_policy_fit import _ppo_paths
    a = _ppo(device="cuda:0", mb_size=256)
    a.fit_backend = "hip_rows"
    a._comm = LocalComm()
    a.policy.old_params[0].data = a.policy.trainable_params[0].data
    for name in ("lib", "calls"):
        monkeypatch.setattr(_lib, name, _never)
    monkeypatch.setattr(a, "engine", _never)
    monkeypatch.setattr(a, "trainer", _never)
    with pytest.raises(ValueError, match='PPO.fit_backend = "hip_rows" takes old parameters that share'):
        a.train_from_paths(_ppo_paths())
    a.mb_size = MAX_BS + 1
    with pytest.raises(ValueError, match=r"1\.\.16384"):
        a.train_from_paths(_ppo_paths())


def test_mse_behaviour_cloning_refuses_the_rows_backend(monkeypatch):
    from mjrl_amd.algos.behavior_cloning_2 import BC
    bc = BC(_expert(), _policy(), device="cuda:0")
    bc.fit_backend = "hip_rows"
    monkeypatch.setattr(_lib, "lib", _never)
    monkeypatch.setattr(_lib, "calls", _never)
    monkeypatch.setattr(bc, "trainer", _never)
    with pytest.raises(ValueError, match="MSE head has no row-tiled kernel"):
        bc.train()
