"""What the two minibatch Adam fits share on the Python side: MLPBaseline's value
fit (baselines/mlp_baseline.py) and DeviceTrainer's policy fit (algos/_device_sgd.py).
Each keeps a CPU optimizer as the source of truth and a device optimizer it trains
with, on a captured step graph (torch route) or by one fused call per epoch (hip
route, csrc/value_fit.hip / policy_fit.hip).  Plain functions over (optimizer,
parameter list): the callers own their mirrors, graph keys and index buffers.
"""
import ctypes as C

import torch

from . import _lib
from ._capture import capture

FIT_BACKENDS = ("torch", "hip")
HIP_MAX_BATCH = 64   # rows of a minibatch the fused kernels hold (csrc/value_fit.hip, policy_fit.hip)


# ---- CPU <-> device optimizer state ---------------------------------------------
def state_to_device(cpu_opt, cpu_params, dev_opt, dev_params, device, step_as_tensor):
    """cpu_opt's state of cpu_params -> dev_opt's state of dev_params (same order).
    A device tensor that exists with the same shape is updated by copy_, never
    rebound: a captured graph reads it by address.  A parameter without CPU state
    zeroes the device state it has.  step_as_tensor: a number `step` becomes a
    0-dim f32 device tensor (capturable optimizers)."""
    for d, c in zip(dev_params, cpu_params):
        sc = cpu_opt.state.get(c)
        sd = dev_opt.state[d]
        if not sc:
            for v in sd.values():
                if torch.is_tensor(v):
                    v.zero_()
            continue
        for k, v in sc.items():
            if torch.is_tensor(v):
                v = v.to(device, dtype=torch.float32 if k == "step" else v.dtype)
                if k in sd and torch.is_tensor(sd[k]) and sd[k].shape == v.shape:
                    sd[k].copy_(v)
                else:
                    sd[k] = v.clone()
            else:
                sd[k] = torch.tensor(float(v), dtype=torch.float32, device=device) \
                    if k == "step" and step_as_tensor else v


def state_to_cpu(cpu_opt, cpu_params, dev_opt, dev_params):
    """dev_opt's state -> cpu_opt's (fresh CPU tensors, `step` a 0-dim f32 one)."""
    for d, c in zip(dev_params, cpu_params):
        sd = dev_opt.state.get(d)
        if not sd:
            continue
        sc = cpu_opt.state[c]
        for k, v in sd.items():
            if torch.is_tensor(v):
                sc[k] = torch.tensor(float(v.item())) if k == "step" else v.detach().cpu().clone()
            else:
                sc[k] = v


# ---- the captured step (torch route) ---------------------------------------------
def capture_step(body, params, opt, device):
    """body() -- zero_grad, loss, backward, opt.step() over static buffers -- as a
    captured hipGraph.  The optimizer state has to exist before capture: one warm-up
    step on a side stream, then the capture; the parameters and the state both
    touched are restored whether or not the capture succeeded (a caller that falls
    back to eager steps starts from the untouched state)."""
    saved = [p.detach().clone() for p in params]
    saved_state = {p: {k: v.clone() for k, v in opt.state[p].items() if torch.is_tensor(v)}
                   for p in params if opt.state.get(p)}
    try:
        s = torch.cuda.Stream(device=device)
        s.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(s):
            body()
        torch.cuda.current_stream(device).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with capture(graph):
            body()
    finally:
        with torch.no_grad():
            for p, v in zip(params, saved):
                p.copy_(v)
            for p in params:
                for k, v in opt.state.get(p, {}).items():
                    if torch.is_tensor(v):
                        if p in saved_state and k in saved_state[p]:
                            v.copy_(saved_state[p][k])
                        else:
                            v.zero_()
    return graph


# ---- around a fused call (hip route) ---------------------------------------------
def ensure_adam_state(opt, params, device):
    """step / exp_avg / exp_avg_sq of a fresh optimizer (torch creates them lazily)."""
    for p in params:
        sd = opt.state[p]
        if "exp_avg" not in sd:
            sd["step"] = torch.zeros((), dtype=torch.float32, device=device)
            sd["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            sd["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)


def scratch(cached, query, dims, device):
    """The fused kernels' scratch, made once per mirror: `cached` if there is one,
    else query(*dims, floats) floats of zeros."""
    if cached is not None:
        return cached
    nf = C.c_int64()
    query(*dims, nf)
    return torch.zeros(nf.value, dtype=torch.float32, device=device)


def fill_net(net, opt, params):
    """net (_lib.ValueNet / PolicyNet / MeanNet): the parameters' and moments' device pointers."""
    for i, p in enumerate(params):
        st = opt.state[p]
        net.p[i], net.exp_avg[i], net.exp_avg_sq[i] = p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
    return net


def adam_hp(opt, params):
    """_lib.Adam from the first parameter group and the steps already taken."""
    g = opt.param_groups[0]
    step = opt.state[params[0]]["step"]
    return _lib.Adam(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                     int(step.item() if torch.is_tensor(step) else step))


def advance_steps(opt, params, nmb):
    """Every step counter += nmb (a tensor in place: a captured graph reads it)."""
    for p in params:
        st = opt.state[p]
        if torch.is_tensor(st["step"]):
            st["step"] += nmb
        else:
            st["step"] = st["step"] + nmb
