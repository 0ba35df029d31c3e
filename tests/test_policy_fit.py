"""The fused policy fit's C ABI and Python switch without a GPU (csrc/policy_fit.hip,
mjrl_policy_fit_epoch; PPO.fit_backend / BC.fit_backend = "hip"): the entry points
are exported and bound, every refusal comes before any launch, the scratch size is
monotonic, fit_backend defaults to torch and survives pickling, and the classes
refuse what the kernel does not hold before anything touches the GPU library."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from mjrl_amd import _lib

NAMES = ("mjrl_policy_fit_scratch", "mjrl_policy_fit_epoch")
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
    net = _lib.PolicyNet()
    for f, arr in enumerate((net.p, net.exp_avg, net.exp_avg_sq)):
        for i in range(7):
            arr[i] = None if hole == (f, i) else FAKE
    return net


ROWS = ("obs", "act", "adv", "ll_old", "old_log_std", "in_shift", "in_scale", "out_shift", "out_scale")


def fit_data(**kw):
    """A PPO call's data with ll_old; every case below changes one field."""
    d = dict(obs=FAKE, act=FAKE, adv=FAKE, ll_old=FAKE, old_log_std=None, in_shift=FAKE, in_scale=FAKE,
             out_shift=FAKE, out_scale=FAKE, T=200, n=6, m=2, h0=32, h1=32, kind=_lib.POLICY_FIT_PPO, clip=0.2)
    d.update(kw)
    return _lib.PolicyFitData(*[d[k] for k in ROWS + ("T", "n", "m", "h0", "h1", "kind", "clip")])


def epoch_args(data=(), **kw):
    """A call that would launch; data: field changes of fit_data, or None for a null structure."""
    a = dict(data=None if data is None else C.byref(fit_data(**dict(data))), idx=FAKE, nmb=2, bs=64,
             net=C.byref(full_net()), hp=C.byref(_lib.Adam(1e-3, 0.9, 0.999, 1e-8, 0.0, 0)), scratch=FAKE, spl=0,
             grad=None, loss=None, stream=None)
    a.update(kw)
    return tuple(a[k] for k in ("data", "idx", "nmb", "bs", "net", "hp", "scratch", "spl", "grad", "loss", "stream"))


REFUSED = ([dict(bs=0), dict(bs=65), dict(bs=-1), dict(nmb=-1), dict(spl=-1), dict(data=None),
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
    kw = dict(REFUSED[case])
    args = epoch_args(**kw)
    assert lib.mjrl_policy_fit_epoch(*args) == _lib.MJRL_EINVAL
    with pytest.raises(_lib.MjrlError, match=r"^mjrl_policy_fit_epoch failed: invalid argument$"):
        _lib.calls(_lib.load).mjrl_policy_fit_epoch(*args)


def test_no_minibatch_is_ok_without_a_launch(lib):
    # nothing is dereferenced or launched: null row pointers are fine
    nothing = dict(obs=None, act=None, adv=None, in_shift=None, in_scale=None, out_shift=None, out_scale=None)
    assert lib.mjrl_policy_fit_epoch(*epoch_args(data=nothing, nmb=0, idx=None, net=None, hp=None,
                                                 scratch=None)) == _lib.MJRL_OK
    assert lib.mjrl_policy_fit_epoch(*epoch_args(data=dict(kind=_lib.POLICY_FIT_BC, ll_old=None, adv=None),
                                                 nmb=0)) == _lib.MJRL_OK
    assert lib.mjrl_policy_fit_epoch(*epoch_args(nmb=0, bs=65)) == _lib.MJRL_EINVAL
    assert lib.mjrl_policy_fit_epoch(*epoch_args(data=dict(h0=65), nmb=0)) == _lib.MJRL_EINVAL


def test_scratch_size(lib):
    f = C.c_int64()
    for n, m, h0, h1, bs in ((0, 2, 32, 32, 64), (6, 0, 32, 32, 64), (6, 65, 32, 32, 64), (6, 2, 0, 32, 64),
                             (6, 2, 65, 32, 64), (6, 2, 32, 0, 64), (6, 2, 32, 65, 64), (6, 2, 32, 32, 0),
                             (6, 2, 32, 32, 65), (-1, 2, 32, 32, 1)):
        assert lib.mjrl_policy_fit_scratch(n, m, h0, h1, bs, C.byref(f)) == _lib.MJRL_EINVAL
    assert lib.mjrl_policy_fit_scratch(6, 2, 32, 32, 64, None) == _lib.MJRL_EINVAL
    with pytest.raises(_lib.MjrlError, match=r"^mjrl_policy_fit_scratch failed"):
        _lib.calls(_lib.load).mjrl_policy_fit_scratch(6, 2, 32, 32, 65, f)
    for n, m, h0, h1 in ((1, 1, 1, 1), (6, 2, 32, 32), (39, 28, 64, 48), (376, 17, 64, 64), (5000, 64, 64, 64)):
        prev = 0
        for bs in (1, 2, 15, 16, 17, 33, 63, 64):
            assert lib.mjrl_policy_fit_scratch(n, m, h0, h1, bs, C.byref(f)) == _lib.MJRL_OK
            assert f.value >= 1 and f.value >= prev   # the last step's loss
            prev = f.value


# ---- the classes ------------------------------------------------------------------------------
def _policy(hidden=(32, 32), n=6, m=2):
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    return MLP(EnvSpec(n, m, 50, 1), hidden_sizes=hidden, seed=1)


def _expert(n=6, m=2):
    rs = np.random.RandomState(0)
    return [dict(observations=rs.randn(70, n), actions=rs.randn(70, m))]


def _ppo(policy=None, **kw):
    from mjrl_amd.algos.ppo_clip import PPO
    return PPO(None, policy if policy is not None else _policy(), None, **kw)


def _ppo_paths(n=6, m=2):
    rs = np.random.RandomState(0)
    return [dict(observations=rs.randn(70, n), actions=rs.randn(70, m), rewards=rs.randn(70),
                 advantages=rs.randn(70))]


def test_fit_backend_default_and_pickling():
    from mjrl_amd.algos.behavior_cloning import BC
    from mjrl_amd.algos.ppo_clip import PPO
    assert PPO.fit_backend == "torch" and BC.fit_backend == "torch"
    for agent in (_ppo(), BC(_expert(), _policy())):
        assert agent.fit_backend == "torch" and "fit_backend" not in agent.__dict__
        assert pickle.loads(pickle.dumps(agent)).fit_backend == "torch"
        agent.fit_backend = "hip"
        agent._trainer = object()   # whatever it holds is dropped
        c = pickle.loads(pickle.dumps(agent))
        assert c.fit_backend == "hip" and c._trainer is None
    assert PPO.fit_backend == "torch" and BC.fit_backend == "torch"


def _never(*a, **k):
    raise AssertionError("a refusal comes before anything touches the GPU library")


def bc_refusals():
    from mjrl_amd.algos.behavior_cloning import BC
    from mjrl_amd.policies.gaussian_linear import LinearPolicy
    from mjrl_amd.utils.gym_env import EnvSpec
    p = _policy
    sgd = lambda pol: torch.optim.SGD(pol.trainable_params, lr=1e-3)   # noqa: E731
    two = lambda pol: torch.optim.Adam([dict(params=pol.trainable_params[:6]),   # noqa: E731
                                        dict(params=pol.trainable_params[6:])], lr=1e-3)
    ams = lambda pol: torch.optim.Adam(pol.trainable_params, lr=1e-3, amsgrad=True)   # noqa: E731
    mx = lambda pol: torch.optim.Adam(pol.trainable_params, lr=1e-3, maximize=True)   # noqa: E731
    adamw = lambda pol: torch.optim.AdamW(pol.trainable_params, lr=1e-3)   # noqa: E731
    mk = lambda pol, opt=None, dev="cuda:0", **kw: BC(_expert(), pol, device=dev,   # noqa: E731
                                                      optimizer=opt(pol) if opt else None, **kw)
    return [
        ("backend", lambda: mk(p()), "triton", "fit_backend"),
        ("batch0", lambda: mk(p(), batch_size=0), "hip", "1..64"),
        ("batch65", lambda: mk(p(), batch_size=65), "hip", "1..64"),
        ("linear", lambda: mk(LinearPolicy(EnvSpec(6, 2, 50, 1), seed=1)), "hip", "LinearPolicy"),
        ("hidden65", lambda: mk(p((65, 32))), "hip", "1..64"),
        ("hidden128", lambda: mk(p((64, 128))), "hip", "1..64"),
        ("sgd", lambda: mk(p(), sgd), "hip", "torch.optim.Adam"),
        ("adamw", lambda: mk(p(), adamw), "hip", "torch.optim.Adam"),
        ("groups", lambda: mk(p(), two), "hip", "one parameter group"),
        ("amsgrad", lambda: mk(p(), ams), "hip", "amsgrad=False"),
        ("maximize", lambda: mk(p(), mx), "hip", "maximize=False"),
        ("cpu", lambda: mk(p(), dev="cpu"), "hip", "GPU"),
    ]


@pytest.mark.parametrize("case", range(12))
def test_bc_refusals(case, monkeypatch):
    name, make, backend, match = bc_refusals()[case]
    bc = make()
    bc.fit_backend = backend
    monkeypatch.setattr(_lib, "lib", _never)
    monkeypatch.setattr(_lib, "calls", _never)
    monkeypatch.setattr(bc, "trainer", _never)
    with pytest.raises(ValueError, match=match):
        bc.train()


def ppo_refusals():
    from mjrl_amd.policies.gaussian_linear import LinearPolicy
    from mjrl_amd.utils.gym_env import EnvSpec

    def with_opt(opt):
        a = _ppo(device="cuda:0")
        a.optimizer = opt(a.policy)
        return a

    def half_aliased():
        a = _ppo(device="cuda:0")
        a.policy.old_params[0].data = a.policy.trainable_params[0].data
        return a

    def all_aliased():
        a = _ppo(device="cuda:0")
        for o, n in zip(a.policy.old_params, a.policy.trainable_params):
            o.data = n.data
        return a

    return [
        ("backend", lambda: _ppo(device="cuda:0"), "triton", "fit_backend"),
        ("mb0", lambda: _ppo(device="cuda:0", mb_size=0), "hip", "1..64"),
        ("mb128", lambda: _ppo(device="cuda:0", mb_size=128), "hip", "1..64"),
        ("linear", lambda: _ppo(LinearPolicy(EnvSpec(6, 2, 50, 1), seed=1), device="cuda:0"), "hip", "LinearPolicy"),
        ("hidden", lambda: _ppo(_policy((32, 96)), device="cuda:0"), "hip", "1..64"),
        ("sgd", lambda: with_opt(lambda pol: torch.optim.SGD(pol.trainable_params, lr=1e-3)), "hip",
         "torch.optim.Adam"),
        ("groups", lambda: with_opt(lambda pol: torch.optim.Adam(
            [dict(params=pol.trainable_params[:6]), dict(params=pol.trainable_params[6:])], lr=1e-3)), "hip",
         "one parameter group"),
        ("amsgrad", lambda: with_opt(lambda pol: torch.optim.Adam(pol.trainable_params, amsgrad=True)), "hip",
         "amsgrad=False"),
        ("maximize", lambda: with_opt(lambda pol: torch.optim.Adam(pol.trainable_params, maximize=True)), "hip",
         "maximize=False"),
        ("cpu", lambda: _ppo(device="cpu"), "hip", "GPU"),
        ("half-aliased", half_aliased, "hip", "share"),
        ("all-aliased", all_aliased, "hip", "share"),
    ]


@pytest.mark.parametrize("case", range(12))
def test_ppo_refusals(case, monkeypatch):
    from mjrl_amd.comm import LocalComm
    name, make, backend, match = ppo_refusals()[case]
    agent = make()
    agent.fit_backend = backend
    agent._comm = LocalComm()
    monkeypatch.setattr(_lib, "lib", _never)
    monkeypatch.setattr(_lib, "calls", _never)
    monkeypatch.setattr(agent, "engine", _never)
    monkeypatch.setattr(agent, "trainer", _never)
    with pytest.raises(ValueError, match=match):
        agent.train_from_paths(_ppo_paths())


def test_aliasing_patterns_the_hip_backend_takes():
    """What MLP leaves: nothing shared at construction, the six mean-network tensors
    shared (log_std cloned by its clamp) after set_param_values."""
    a = _ppo(device="cuda:0")
    assert a._aliasing() == [False] * 7
    a.policy.set_param_values(a.policy.get_param_values(), set_new=True, set_old=True)
    assert a._aliasing() == [True] * 6 + [False]
