"""The wide fused policy fit's C ABI and Python switch without a GPU (csrc/policy_fit_wide.hip;
mjrl_policy_fit_wide_epoch, mjrl_policy_mse_wide_epoch; fit_backend = "hip_wide" of PPO, BC and
behavior_cloning_2.BC): the entry points are exported and bound, every refusal comes before any
launch, the scratch size is monotonic, the classes refuse what the kernels do not hold before
anything touches the GPU library, pickling keeps the backend, and the torch route on the CPU
device reproduces the reference's runs at these widths (tests/golden/bc_wide.npz, bc2_wide.npz,
ppo_wide.npz: this pins the fixtures)."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

from mjrl_amd import _lib
from test_policy_fit import FAKE, _expert, _never, _policy, _ppo, _ppo_paths, fit_data, full_net

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ("mjrl_policy_fit_wide_scratch", "mjrl_policy_fit_wide_epoch", "mjrl_policy_mse_wide_epoch")
BC_HIDDEN, PPO_HIDDEN = (96, 160), (128, 128)


@pytest.fixture(scope="module")
def lib():
    from mjrl_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_entry_points_are_bound(lib):
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert name not in _lib.QUERIES and name not in _lib.STAGE_FUNCS
        assert getattr(_lib.calls(_lib.load), name).errcheck is not None


def mean_net(hole=None):
    net = _lib.MeanNet()
    for f, arr in enumerate((net.p, net.exp_avg, net.exp_avg_sq)):
        for i in range(6):
            arr[i] = None if hole == (f, i) else FAKE
    return net


def epoch_args(mse, data=(), **kw):
    """A call that would launch; data: field changes of fit_data (a PPO call with ll_old, here at
    the widths (256, 256)), or None for a null structure."""
    d = dict(h0=256, h1=256)
    if data is not None:
        d.update(dict(data))
    a = dict(data=None if data is None else C.byref(fit_data(**d)), idx=FAKE, nmb=2, bs=64,
             net=C.byref(mean_net() if mse else full_net()), hp=C.byref(_lib.Adam(1e-3, 0.9, 0.999, 1e-8, 0.0, 0)),
             scratch=FAKE, grad=None, loss=None, stream=None)
    a.update(kw)
    return tuple(a[k] for k in ("data", "idx", "nmb", "bs", "net", "hp", "scratch", "grad", "loss", "stream"))


# what both entry points refuse
REFUSED = ([dict(bs=0), dict(bs=65), dict(bs=-1), dict(nmb=-1), dict(data=None),
            dict(hp=C.byref(_lib.Adam(1e-3, 0.9, 0.999, 1e-8, 0.0, -1)))]
           + [{k: None} for k in ("idx", "net", "hp", "scratch")]
           + [dict(data={k: v}) for k, v in (("n", 0), ("n", -3), ("n", (1 << 24) + 1), ("m", 0), ("m", 65),
                                             ("h0", 0), ("h0", 257), ("h1", 0), ("h1", 257), ("T", -1))]
           + [dict(data={k: None}) for k in ("obs", "act", "in_shift", "in_scale", "out_shift", "out_scale")])
# and the heads of mjrl_policy_fit_wide_epoch alone: kind, adv, exactly one of ll_old and old_log_std
REFUSED_FIT = ([dict(data={"kind": 2}), dict(data={"kind": -1}), dict(data={"adv": None}),
                dict(data=dict(ll_old=None)), dict(data=dict(old_log_std=FAKE)),
                dict(data=dict(kind=_lib.POLICY_FIT_BC, obs=None))]
               + [dict(net=C.byref(full_net(hole=(f, i)))) for f in range(3) for i in (0, 3, 6)])
REFUSED_MSE = [dict(net=C.byref(mean_net(hole=(f, i)))) for f in range(3) for i in (0, 3, 5)]
ALL_REFUSED = ([("fit", c) for c in REFUSED + REFUSED_FIT] + [("mse", c) for c in REFUSED + REFUSED_MSE])


@pytest.mark.parametrize("case", range(len(ALL_REFUSED)))
def test_bad_arguments_are_refused_before_any_launch(lib, case):
    head, kw = ALL_REFUSED[case]
    name = "mjrl_policy_mse_wide_epoch" if head == "mse" else "mjrl_policy_fit_wide_epoch"
    args = epoch_args(head == "mse", **dict(kw))
    assert getattr(lib, name)(*args) == _lib.MJRL_EINVAL
    with pytest.raises(_lib.MjrlError, match=r"^%s failed: invalid argument$" % name):
        getattr(_lib.calls(_lib.load), name)(*args)


def test_the_mse_entry_reads_no_head_field(lib):
    """kind, adv, ll_old and old_log_std are the other entry's: with nmb == 0 (nothing launches)
    whatever they hold is accepted."""
    odd = dict(kind=77, adv=None, ll_old=None, old_log_std=None)
    assert lib.mjrl_policy_mse_wide_epoch(*epoch_args(True, data=odd, nmb=0)) == _lib.MJRL_OK


@pytest.mark.parametrize("mse", (False, True))
def test_no_minibatch_is_ok_without_a_launch(lib, mse):
    fn = lib.mjrl_policy_mse_wide_epoch if mse else lib.mjrl_policy_fit_wide_epoch
    # nothing is dereferenced or launched: null row pointers are fine
    nothing = dict(obs=None, act=None, adv=None, in_shift=None, in_scale=None, out_shift=None, out_scale=None)
    assert fn(*epoch_args(mse, data=nothing, nmb=0, idx=None, net=None, hp=None, scratch=None)) == _lib.MJRL_OK
    assert fn(*epoch_args(mse, data=dict(kind=_lib.POLICY_FIT_BC, ll_old=None, adv=None), nmb=0)) == _lib.MJRL_OK
    assert fn(*epoch_args(mse, nmb=0, bs=65)) == _lib.MJRL_EINVAL
    assert fn(*epoch_args(mse, data=dict(h0=257), nmb=0)) == _lib.MJRL_EINVAL


def test_scratch_size(lib):
    f = C.c_int64()
    for n, m, h0, h1, bs in ((0, 2, 32, 32, 64), (6, 0, 32, 32, 64), (6, 65, 32, 32, 64), (6, 2, 0, 32, 64),
                             (6, 2, 257, 32, 64), (6, 2, 32, 0, 64), (6, 2, 32, 257, 64), (6, 2, 32, 32, 0),
                             (6, 2, 32, 32, 65), (-1, 2, 32, 32, 1)):
        assert lib.mjrl_policy_fit_wide_scratch(n, m, h0, h1, bs, C.byref(f)) == _lib.MJRL_EINVAL
    assert lib.mjrl_policy_fit_wide_scratch(6, 2, 32, 32, 64, None) == _lib.MJRL_EINVAL
    with pytest.raises(_lib.MjrlError, match=r"^mjrl_policy_fit_wide_scratch failed"):
        _lib.calls(_lib.load).mjrl_policy_fit_wide_scratch(6, 2, 32, 32, 65, f)
    for n, m, h0, h1 in ((1, 1, 1, 1), (6, 2, 128, 128), (39, 28, 256, 256), (376, 17, 65, 256), (5000, 64, 256, 64)):
        prev = 0
        for bs in (1, 2, 15, 16, 17, 33, 63, 64):
            assert lib.mjrl_policy_fit_wide_scratch(n, m, h0, h1, bs, C.byref(f)) == _lib.MJRL_OK
            # the tiles that cross a launch (a0 twice, a1, g1 for 64 rows of h0 / h1 columns) and the loss
            assert f.value >= 64 * (2 * h0 + 2 * h1) + 1 and f.value >= prev
            prev = f.value


# ---- the classes ------------------------------------------------------------------------------
def test_check_fit_backend_takes_the_wide_widths():
    from mjrl_amd.algos import _device_sgd as S
    assert S.POLICY_FIT_BACKENDS == ("torch", "hip", "hip_wide")
    for hidden in ((65, 32), (64, 128), (256, 256), (1, 1)):
        pol = _policy(hidden)
        opt = torch.optim.Adam(pol.trainable_params, lr=1e-3)
        assert S.check_fit_backend("BC", "hip_wide", pol, opt, 64, "cuda:0") is True
        assert S.check_fit_backend("BC", "torch", pol, opt, 64, "cuda:0") is False
    pol = _policy((65, 32))
    opt = torch.optim.Adam(pol.trainable_params, lr=1e-3)
    with pytest.raises(ValueError, match=r"1\.\.64"):
        S.check_fit_backend("BC", "hip", pol, opt, 64, "cuda:0")
    for name in ("triton", "hip-wide", "wide", None):
        with pytest.raises(ValueError, match="fit_backend"):
            S.check_fit_backend("BC", name, pol, opt, 64, "cuda:0")
    from mjrl_amd import _device_fit
    assert _device_fit.FIT_BACKENDS == ("torch", "hip")   # MLPBaseline's: as it was


def test_fit_backend_pickling_keeps_hip_wide():
    from mjrl_amd.algos.behavior_cloning import BC
    from mjrl_amd.algos.behavior_cloning_2 import BC as BC2
    from mjrl_amd.algos.ppo_clip import PPO
    for agent in (_ppo(_policy((128, 128))), BC(_expert(), _policy((96, 160))), BC2(_expert(), _policy((96, 160)))):
        agent.fit_backend = "hip_wide"
        agent._trainer = object()   # whatever it holds is dropped
        c = pickle.loads(pickle.dumps(agent))
        assert c.fit_backend == "hip_wide" and c._trainer is None
    assert PPO.fit_backend == "torch" and BC.fit_backend == "torch" and BC2.fit_backend == "torch"


def _optimizers(params_of):
    return dict(
        sgd=lambda pol: torch.optim.SGD(params_of(pol), lr=1e-3),
        adamw=lambda pol: torch.optim.AdamW(params_of(pol), lr=1e-3),
        groups=lambda pol: torch.optim.Adam([dict(params=params_of(pol)[:3]), dict(params=params_of(pol)[3:])], lr=1e-3),
        amsgrad=lambda pol: torch.optim.Adam(params_of(pol), lr=1e-3, amsgrad=True),
        maximize=lambda pol: torch.optim.Adam(params_of(pol), lr=1e-3, maximize=True))


OPT_MATCH = dict(sgd="torch.optim.Adam", adamw="torch.optim.Adam", groups="one parameter group",
                 amsgrad="amsgrad=False", maximize="maximize=False")


def bc_refusals(which):
    """(name, constructor, message) of every "hip_wide" refusal of behavior_cloning.BC (which = 1)
    or behavior_cloning_2.BC (which = 2)."""
    from mjrl_amd.policies.gaussian_linear import LinearPolicy
    from mjrl_amd.utils.gym_env import EnvSpec
    if which == 1:
        from mjrl_amd.algos.behavior_cloning import BC
        params_of = lambda pol: list(pol.trainable_params)   # noqa: E731
    else:
        from mjrl_amd.algos.behavior_cloning_2 import BC
        params_of = lambda pol: list(pol.model.parameters())   # noqa: E731
    p = lambda hidden=(128, 96): _policy(hidden)   # noqa: E731
    mk = lambda pol, opt=None, dev="cuda:0", **kw: BC(_expert(), pol, device=dev,   # noqa: E731
                                                      optimizer=opt(pol) if opt else None, **kw)
    out = [
        ("batch0", lambda: mk(p(), batch_size=0), r"1\.\.64"),
        ("batch65", lambda: mk(p(), batch_size=65), r"1\.\.64"),
        ("linear", lambda: mk(LinearPolicy(EnvSpec(6, 2, 50, 1), seed=1)), "LinearPolicy"),
        ("hidden257", lambda: mk(p((257, 32))), r"1\.\.256"),
        ("hidden257b", lambda: mk(p((64, 257))), r"1\.\.256"),
        ("cpu", lambda: mk(p(), dev="cpu"), "GPU"),
    ]
    for name, opt in _optimizers(params_of).items():
        out.append((name, lambda opt=opt: mk(p(), opt), OPT_MATCH[name]))
    return out


BC_CASES = [(w, i) for w in (1, 2) for i in range(11)]


@pytest.mark.parametrize("which,case", BC_CASES)
def test_bc_refusals(which, case, monkeypatch):
    name, make, match = bc_refusals(which)[case]
    bc = make()
    bc.fit_backend = "hip_wide"
    monkeypatch.setattr(_lib, "lib", _never)
    monkeypatch.setattr(_lib, "calls", _never)
    monkeypatch.setattr(bc, "trainer", _never)
    with pytest.raises(ValueError, match=match) as e:
        bc.train()
    assert "hip_wide" in str(e.value)


def test_bc2_refuses_an_optimizer_over_the_seven_tensors(monkeypatch):
    from mjrl_amd.algos.behavior_cloning_2 import BC
    pol = _policy((128, 96))
    bc = BC(_expert(), pol, device="cuda:0", optimizer=torch.optim.Adam(pol.trainable_params, lr=1e-3))
    bc.fit_backend = "hip_wide"
    monkeypatch.setattr(_lib, "calls", _never)
    monkeypatch.setattr(bc, "trainer", _never)
    with pytest.raises(ValueError, match="policy.model.parameters"):
        bc.train()


def ppo_refusals():
    from mjrl_amd.policies.gaussian_linear import LinearPolicy
    from mjrl_amd.utils.gym_env import EnvSpec
    wide = lambda **kw: _ppo(_policy((128, 96)), device="cuda:0", **kw)   # noqa: E731

    def with_opt(opt):
        a = wide()
        a.optimizer = opt(a.policy)
        return a

    def half_aliased():
        a = wide()
        a.policy.old_params[0].data = a.policy.trainable_params[0].data
        return a

    def all_aliased():
        a = wide()
        for o, n in zip(a.policy.old_params, a.policy.trainable_params):
            o.data = n.data
        return a

    # (a PPO agent over a hidden layer of 257 units does not exist: the update engine refuses the
    # policy at construction, engine.kernel_hidden)
    out = [
        ("mb0", lambda: wide(mb_size=0), r"1\.\.64"),
        ("mb65", lambda: wide(mb_size=65), r"1\.\.64"),
        ("linear", lambda: _ppo(LinearPolicy(EnvSpec(6, 2, 50, 1), seed=1), device="cuda:0"), "LinearPolicy"),
        ("all-aliased", all_aliased, "share"),
        ("cpu", lambda: _ppo(_policy((128, 96)), device="cpu"), "GPU"),
        ("half-aliased", half_aliased, "share"),
    ]
    for name, opt in _optimizers(lambda pol: list(pol.trainable_params)).items():
        out.append((name, lambda opt=opt: with_opt(opt), OPT_MATCH[name]))
    return out


@pytest.mark.parametrize("case", range(11))
def test_ppo_refusals(case, monkeypatch):
    from mjrl_amd.comm import LocalComm
    name, make, match = ppo_refusals()[case]
    agent = make()
    agent.fit_backend = "hip_wide"
    agent._comm = LocalComm()
    monkeypatch.setattr(_lib, "lib", _never)
    monkeypatch.setattr(_lib, "calls", _never)
    monkeypatch.setattr(agent, "engine", _never)
    monkeypatch.setattr(agent, "trainer", _never)
    with pytest.raises(ValueError, match=match) as e:
        agent.train_from_paths(_ppo_paths())
    assert "hip_wide" in str(e.value)


# ---- the fixtures: the torch route on the CPU device against the reference's runs ---------------
def bc_paths(z):
    offs = np.concatenate([[0], np.cumsum(z["lengths"])])
    return [dict(observations=z["obs"][offs[i]:offs[i + 1]], actions=z["act"][offs[i]:offs[i + 1]])
            for i in range(len(z["lengths"]))]


def run_bc_wide(which, device, backend="torch"):
    """The fixture's run of behavior_cloning.BC (which = 1) or behavior_cloning_2.BC (2)."""
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    if which == 1:
        from mjrl_amd.algos.behavior_cloning import BC
    else:
        from mjrl_amd.algos.behavior_cloning_2 import BC
    z = np.load(os.path.join(GOLDEN, "bc_wide.npz" if which == 1 else "bc2_wide.npz"))
    assert 300 <= z["obs"].shape[0] <= 600
    policy = MLP(EnvSpec(6, 3, 120, 1), hidden_sizes=BC_HIDDEN, seed=5)
    np.testing.assert_array_equal(policy.get_param_values(), z["init"])
    bc = BC(bc_paths(z), policy, epochs=2, batch_size=32, lr=1e-3, device=device)
    bc.fit_backend = backend
    if which == 2:
        np.testing.assert_array_equal(policy.get_param_values(), z["after_init"])
    t = policy.model.transformations
    for k in ("in_shift", "in_scale", "out_shift", "out_scale"):
        np.testing.assert_allclose(t[k], z[k], rtol=1e-12)
    np.random.seed(int(z["np_seed"]))
    bc.train()
    return bc, policy, z


@pytest.mark.parametrize("which", (1, 2))
def test_bc_wide_fixture_is_the_torch_route_on_the_cpu_device(which):
    bc, policy, z = run_bc_wide(which, "cpu")
    ref = z["final"]
    moved = np.linalg.norm(ref - (z["after_init"] if which == 2 else z["init"])) / np.linalg.norm(ref)
    rel = np.linalg.norm(policy.get_param_values() - ref) / np.linalg.norm(ref)
    print("BC %d wide, CPU device: parameters %.3g from the reference's; the run moved them by %.3g" % (
        which, rel, moved))
    np.testing.assert_allclose(np.array(bc.logger.log["loss"], dtype=np.float64), z["loss"], rtol=1e-5)
    assert rel <= 1e-5
    assert moved >= 0.05   # the 1e-3 of the GPU tests is a small part of what the steps do
    assert bc.logger.log["epoch"] == [0, 1, 2]


def ppo_wide_agent(device, backend="torch"):
    from mjrl_amd.algos.ppo_clip import PPO
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    z = np.load(os.path.join(GOLDEN, "ppo_wide.npz"))
    assert 300 <= z["obs0"].shape[0] <= 600
    policy = MLP(EnvSpec(6, 2, 200, 1), hidden_sizes=PPO_HIDDEN, seed=3, init_log_std=-0.5)
    np.testing.assert_array_equal(policy.get_param_values(), z["init"])
    kw = {} if device is None else dict(device=device)
    ppo = PPO(None, policy, None, clip_coef=0.2, epochs=2, mb_size=64, learn_rate=3e-3, save_logs=True, **kw)
    ppo.fit_backend = backend
    return ppo, policy, z


def ppo_wide_paths(z, it):
    offs = np.concatenate([[0], np.cumsum(z["lengths"])])
    sl = lambda k: [z["%s%d" % (k, it)][offs[i]:offs[i + 1]] for i in range(len(z["lengths"]))]   # noqa: E731
    return [dict(observations=o, actions=a, rewards=r, advantages=v)
            for o, a, r, v in zip(sl("obs"), sl("act"), sl("rew"), sl("adv"))]


def test_ppo_wide_fixture_is_the_torch_route_on_the_cpu_device():
    """test_bc_ppo.py::test_ppo_matches_reference_cpu_device at hidden (128, 128)."""
    ppo, policy, z = ppo_wide_agent("cpu")

    def cpi(o, a, adv):
        LLn, LLo = policy.new_dist_info(o, a)[0], policy.old_dist_info(o, a)[0]
        return torch.mean(torch.exp(LLn - LLo) * torch.from_numpy(adv).float()).detach()

    ppo.CPI_surrogate = cpi
    ppo.kl_old_new = lambda o, a: policy.mean_kl(policy.new_dist_info(o, a), policy.old_dist_info(o, a)).detach()
    ppo.engine = lambda: type("E", (), {"device": torch.device("cpu")})
    for it in range(2):
        assert ppo._aliasing() == ([False] * 7 if it == 0 else [True] * 6 + [False])
        np.random.seed(int(z["np_seed%d" % it]))
        stats = ppo.train_from_paths(ppo_wide_paths(z, it))
        np.testing.assert_allclose(stats, z["base_stats%d" % it], rtol=1e-12)
        ref = z["params%d" % it]
        rel = np.linalg.norm(policy.get_param_values() - ref) / np.linalg.norm(ref)
        print("PPO wide iteration %d, CPU device: parameters %.3g from the reference's" % (it, rel))
        assert rel <= 1e-5, it
        np.testing.assert_allclose(ppo.logger.log["kl_dist"][-1], z["kl_dist%d" % it], rtol=1e-4)
        np.testing.assert_allclose(ppo.logger.log["surr_improvement"][-1], z["surr_improvement%d" % it],
                                   rtol=1e-4, atol=1e-7)
