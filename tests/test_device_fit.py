"""mjrl_amd/_device_fit.py without a GPU (device = "cpu"): the optimizer-state mirror
MLPBaseline and DeviceTrainer share round-trips the moments bit for bit and updates
existing device tensors in place, and the helpers around a fused call read and
advance what the C ABI's mjrl_adam takes."""
import pytest
import torch

from mjrl_amd import _device_fit as F

CPU = torch.device("cpu")


def make(steps, seed=0):
    """A 2-tensor parameter list and its Adam after `steps` real steps."""
    torch.manual_seed(seed)
    params = [torch.randn(3, 4, requires_grad=True), torch.randn(3, requires_grad=True)]
    opt = torch.optim.Adam(params, lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.01)
    for _ in range(steps):
        opt.zero_grad()
        (params[0].pow(2).sum() + params[1].sin().sum()).backward()
        opt.step()
    return params, opt


def mirror(params):
    dev = [torch.zeros_like(p, requires_grad=True) for p in params]
    return dev, torch.optim.Adam(dev, capturable=False)


@pytest.mark.parametrize("steps", [0, 3])
def test_moment_round_trip(steps):
    params, opt = make(steps)
    want = {i: {k: v.clone() for k, v in opt.state[p].items()} for i, p in enumerate(params) if opt.state.get(p)}
    dparams, dopt = mirror(params)
    F.state_to_device(opt, params, dopt, dparams, CPU, True)
    for p in params:
        opt.state.pop(p, None)   # what comes back is the device's, not a leftover
    F.state_to_cpu(opt, params, dopt, dparams)
    assert len(want) == (2 if steps else 0)
    for i, p in enumerate(params):
        if not steps:
            assert not opt.state.get(p) and not dopt.state.get(dparams[i])
            continue
        got = opt.state[p]
        assert torch.equal(got["exp_avg"], want[i]["exp_avg"]) and torch.equal(got["exp_avg_sq"], want[i]["exp_avg_sq"])
        assert torch.is_tensor(got["step"]) and got["step"].shape == () and got["step"].dtype == torch.float32
        assert got["step"].item() == want[i]["step"].item() == steps


def test_stateless_cpu_optimizer_zeroes_the_device_state():
    params, opt = make(3)
    dparams, dopt = mirror(params)
    F.state_to_device(opt, params, dopt, dparams, CPU, True)
    assert all(dopt.state[d]["exp_avg_sq"].abs().sum() > 0 for d in dparams)
    fresh_params, fresh = make(0)
    F.state_to_device(fresh, fresh_params, dopt, dparams, CPU, True)
    for d in dparams:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.count_nonzero(dopt.state[d][k]) == 0, k


def test_second_copy_updates_the_same_tensors():
    params, opt = make(3)
    dparams, dopt = mirror(params)
    F.state_to_device(opt, params, dopt, dparams, CPU, True)
    before = [(id(dopt.state[d][k]), dopt.state[d][k].data_ptr()) for d in dparams for k in ("step", "exp_avg", "exp_avg_sq")]
    params2, opt2 = make(5, seed=1)
    F.state_to_device(opt2, params2, dopt, dparams, CPU, True)
    after = [(id(dopt.state[d][k]), dopt.state[d][k].data_ptr()) for d in dparams for k in ("step", "exp_avg", "exp_avg_sq")]
    assert before == after
    for d, c in zip(dparams, params2):
        assert torch.equal(dopt.state[d]["exp_avg"], opt2.state[c]["exp_avg"])
        assert dopt.state[d]["step"].item() == 5


@pytest.mark.parametrize("tensor_step", [True, False])
def test_fused_call_helpers(tensor_step):
    params, opt = make(0)
    F.ensure_adam_state(opt, params, CPU)
    for p in params:
        st = opt.state[p]
        assert st["exp_avg"].shape == p.shape and torch.count_nonzero(st["exp_avg_sq"]) == 0
        st["step"] = torch.tensor(7.0) if tensor_step else 7.0
    hp = F.adam_hp(opt, params)
    assert (hp.lr, hp.beta1, hp.beta2, hp.eps, hp.weight_decay, hp.step0) == (3e-3, 0.8, 0.95, 1e-6, 0.01, 7)
    kept = [opt.state[p]["step"] for p in params]
    F.advance_steps(opt, params, 5)
    for p, k in zip(params, kept):
        step = opt.state[p]["step"]
        assert float(step) == 12.0 and torch.is_tensor(step) == tensor_step
        assert not tensor_step or step is k   # a tensor counter advances in place
    assert F.adam_hp(opt, params).step0 == 12
