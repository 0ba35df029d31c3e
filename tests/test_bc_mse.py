"""MSE behaviour cloning (mjrl_amd/algos/behavior_cloning_2.py; the reference's
mjrl/algos/behavior_cloning_2.py) without a GPU: the class on the CPU device
against the reference's own run (tests/golden/bc2.npz), what its optimizer holds,
pickling, the C ABI of the fused MSE head (mjrl_policy_mse_epoch: exported, bound,
every refusal before any launch) and the class's refusals before anything touches
the GPU library."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

from mjrl_amd import _lib
from test_bc_ppo import _bc_paths

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAME = "mjrl_policy_mse_epoch"
FAKE = 4096   # a non-null address no refused call dereferences


def run_bc2(device, backend=None):
    from mjrl_amd.algos.behavior_cloning_2 import BC
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    z = np.load(os.path.join(GOLDEN, "bc2.npz"))
    policy = MLP(EnvSpec(6, 3, 120, 1), hidden_sizes=(32, 32), seed=5)
    np.testing.assert_array_equal(policy.get_param_values(), z["init"])
    bc = BC(_bc_paths(z), policy, epochs=2, batch_size=32, lr=1e-3, device=device)
    if backend is not None:
        bc.fit_backend = backend
    np.testing.assert_array_equal(policy.get_param_values(), z["after_init"])
    t = policy.model.transformations
    for k in ("in_shift", "in_scale", "out_shift", "out_scale"):
        np.testing.assert_allclose(t[k], z[k], rtol=1e-12)
    np.random.seed(int(z["np_seed"]))
    bc.train()
    return bc, policy, z


_CPU = []


def cpu_run():
    if not _CPU:
        _CPU.append(run_bc2("cpu"))
    return _CPU[0]


def test_bc2_matches_reference_cpu_device():
    bc, policy, z = cpu_run()
    loss = np.array(bc.logger.log["loss"], dtype=np.float64)
    ref = z["final"]
    print("losses", loss, "reference", z["loss"], "parameters %.3g from the reference's (in norm)" % (
        np.linalg.norm(policy.get_param_values() - ref) / np.linalg.norm(ref)))
    np.testing.assert_allclose(loss, z["loss"], rtol=1e-5)
    assert np.linalg.norm(policy.get_param_values() - ref) <= 1e-5 * np.linalg.norm(ref)
    assert bc.logger.log["epoch"] == [0, 1, 2]
    assert all(isinstance(v, np.float32) for v in bc.logger.log["loss"])
    assert bc.mb_size == 32 and isinstance(bc.loss_function, torch.nn.MSELoss)


def test_loss_is_the_mse_at_the_current_parameters():
    bc, policy, z = cpu_run()
    got = bc.loss(z["obs"], z["act"])
    assert isinstance(got, torch.Tensor) and got.device.type == "cpu" and got.dim() == 0
    with torch.no_grad():
        want = torch.nn.functional.mse_loss(policy.model(torch.from_numpy(z["obs"]).float()),
                                            torch.from_numpy(z["act"]).float())
    np.testing.assert_allclose(float(got), float(want), rtol=1e-6)
    np.testing.assert_allclose(float(got), z["loss"][-1], rtol=1e-5)


def test_optimizer_holds_the_mean_network_and_log_std_stays():
    bc, policy, z = cpu_run()
    groups = bc.optimizer.param_groups
    assert len(groups) == 1 and len(groups[0]["params"]) == 6
    assert all(a is b for a, b in zip(groups[0]["params"], policy.model.parameters()))
    assert all(k is not policy.log_std for k in bc.optimizer.state) and len(bc.optimizer.state) == 6
    m = policy.m
    after = policy.get_param_values()
    assert np.array_equal(after[-m:].view(np.uint32), z["after_init"][-m:].view(np.uint32))
    assert np.array_equal(policy.log_std.data.numpy().view(np.uint32), z["after_init"][-m:].view(np.uint32))
    assert not np.array_equal(after[:-m], z["after_init"][:-m])
    steps = [float(bc.optimizer.state[p]["step"]) for p in policy.model.parameters()]
    assert steps == [2 * int(300 / 32)] * 6


def test_linear_policy_trains_with_the_torch_backend():
    from mjrl_amd.algos.behavior_cloning_2 import BC
    from mjrl_amd.policies.gaussian_linear import LinearPolicy
    from mjrl_amd.utils.gym_env import EnvSpec
    z = np.load(os.path.join(GOLDEN, "bc2.npz"))
    policy = LinearPolicy(EnvSpec(6, 3, 120, 1), seed=1)
    bc = BC(_bc_paths(z), policy, epochs=2, batch_size=32, lr=1e-2, device="cpu")
    ls = policy.get_param_values()[-3:].copy()
    np.random.seed(3)
    bc.train()
    loss = bc.logger.log["loss"]
    assert len(bc.optimizer.param_groups[0]["params"]) == 2 and loss[-1] < loss[0]
    assert np.array_equal(policy.get_param_values()[-3:], ls)


def test_fit_backend_default_and_pickling():
    from mjrl_amd.algos.behavior_cloning_2 import BC
    from test_policy_fit import _expert, _policy
    assert BC.fit_backend == "torch"
    bc = BC(_expert(), _policy())
    assert bc.fit_backend == "torch" and "fit_backend" not in bc.__dict__
    assert pickle.loads(pickle.dumps(bc)).fit_backend == "torch"
    bc.fit_backend = "hip"
    bc._trainer = object()   # whatever it holds is dropped
    c = pickle.loads(pickle.dumps(bc))
    assert c.fit_backend == "hip" and c._trainer is None
    # the clone's optimizer is still bound to the clone's mean network
    assert all(a is b for a, b in zip(c.optimizer.param_groups[0]["params"], c.policy.model.parameters()))
    assert BC.fit_backend == "torch"
    bc2, policy, _ = cpu_run()
    clone = pickle.loads(pickle.dumps(bc2))
    assert bc2._trainer is not None and clone._trainer is None
    np.testing.assert_array_equal(clone.policy.get_param_values(), policy.get_param_values())


# ---- the C ABI -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mjrl_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_entry_point_is_bound(lib):
    assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    assert NAME not in _lib.QUERIES and NAME not in _lib.STAGE_FUNCS
    assert getattr(_lib.calls(_lib.load), NAME).errcheck is not None
    assert C.sizeof(_lib.MeanNet) == C.sizeof(_lib.ValueNet) == 18 * C.sizeof(C.c_void_p)


def full_net(hole=None):
    net = _lib.MeanNet()
    for f, arr in enumerate((net.p, net.exp_avg, net.exp_avg_sq)):
        for i in range(6):
            arr[i] = None if hole == (f, i) else FAKE
    return net


ROWS = ("obs", "act", "adv", "ll_old", "old_log_std", "in_shift", "in_scale", "out_shift", "out_scale")


def fit_data(**kw):
    """What the entry reads, and nothing else: adv / ll_old / old_log_std null, a kind no head has."""
    d = dict(obs=FAKE, act=FAKE, adv=None, ll_old=None, old_log_std=None, in_shift=FAKE, in_scale=FAKE,
             out_shift=FAKE, out_scale=FAKE, T=200, n=6, m=2, h0=32, h1=32, kind=77, clip=0.0)
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
                                             ("h0", 0), ("h0", 65), ("h1", 0), ("h1", 65), ("T", -1))]
           + [dict(data={k: None}) for k in ("obs", "act", "in_shift", "in_scale", "out_shift", "out_scale")]
           + [dict(net=C.byref(full_net(hole=(f, i)))) for f in range(3) for i in (0, 3, 5)])


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_bad_arguments_are_refused_before_any_launch(lib, case):
    args = epoch_args(**dict(REFUSED[case]))
    assert lib.mjrl_policy_mse_epoch(*args) == _lib.MJRL_EINVAL
    with pytest.raises(_lib.MjrlError, match=r"^mjrl_policy_mse_epoch failed: invalid argument$"):
        _lib.calls(_lib.load).mjrl_policy_mse_epoch(*args)


def test_no_minibatch_is_ok_without_a_launch(lib):
    # nothing is dereferenced or launched: null row pointers are fine
    nothing = dict(obs=None, act=None, in_shift=None, in_scale=None, out_shift=None, out_scale=None)
    assert lib.mjrl_policy_mse_epoch(*epoch_args(data=nothing, nmb=0, idx=None, net=None, hp=None,
                                                 scratch=None)) == _lib.MJRL_OK
    # adv = ll_old = old_log_std = NULL and kind = 77: none of them is looked at
    d = fit_data()
    assert (d.adv, d.ll_old, d.old_log_std, d.kind) == (None, None, None, 77)
    assert lib.mjrl_policy_mse_epoch(*epoch_args(nmb=0)) == _lib.MJRL_OK
    assert _lib.calls(_lib.load).mjrl_policy_mse_epoch(*epoch_args(nmb=0)) == _lib.MJRL_OK
    assert lib.mjrl_policy_mse_epoch(*epoch_args(nmb=0, bs=65)) == _lib.MJRL_EINVAL
    assert lib.mjrl_policy_mse_epoch(*epoch_args(data=dict(h0=65), nmb=0)) == _lib.MJRL_EINVAL


# ---- the class's refusals ------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError("a refusal comes before anything touches the GPU library")


def bc2_refusals():
    from mjrl_amd.algos.behavior_cloning_2 import BC
    from mjrl_amd.policies.gaussian_linear import LinearPolicy
    from mjrl_amd.utils.gym_env import EnvSpec
    from test_policy_fit import _expert, _policy as p
    mean = lambda pol: list(pol.model.parameters())   # noqa: E731
    sgd = lambda pol: torch.optim.SGD(mean(pol), lr=1e-3)   # noqa: E731
    two = lambda pol: torch.optim.Adam([dict(params=mean(pol)[:4]), dict(params=mean(pol)[4:])], lr=1e-3)   # noqa: E731
    ams = lambda pol: torch.optim.Adam(mean(pol), lr=1e-3, amsgrad=True)   # noqa: E731
    mx = lambda pol: torch.optim.Adam(mean(pol), lr=1e-3, maximize=True)   # noqa: E731
    adamw = lambda pol: torch.optim.AdamW(mean(pol), lr=1e-3)   # noqa: E731
    seven = lambda pol: torch.optim.Adam(pol.trainable_params, lr=1e-3)   # noqa: E731
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
        ("seven", lambda: mk(p(), seven), "hip", r"policy\.model\.parameters\(\)"),
    ]


@pytest.mark.parametrize("case", range(13))
def test_bc2_refusals(case, monkeypatch):
    name, make, backend, match = bc2_refusals()[case]
    bc = make()
    bc.fit_backend = backend
    monkeypatch.setattr(_lib, "lib", _never)
    monkeypatch.setattr(_lib, "calls", _never)
    monkeypatch.setattr(bc, "trainer", _never)
    with pytest.raises(ValueError, match=match):
        bc.train()
