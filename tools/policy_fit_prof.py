"""Where a fused policy-fit step's time goes: the phase profile of k_pfit
(csrc/policy_fit.hip, s_memtime stamps of thread 0 between the step's barriers)
from the profiling build

    python -m mjrl_amd.build --tag _pfprof --extra=-DMJRL_PFIT_PROF
    MJRL_AMD_LIB=mjrl_amd/lib/libmjrl_amd_pfprof.so python tools/policy_fit_prof.py [--n 376 --m 17]

over `--steps` PPO steps on synthetic rows through the raw entry point.  Prints
cycles per step and shares per phase.  Needs a GPU."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PHASES = ["1 indices, constants", "2 X tile load, chunk 0", "2 layer 0 products, tanh", "3 layer 1", "4 layer 2, z",
          "5 row LL, loss head", "6 d log_std, loss, gmu", "7 g1", "8 g0", "9 X tile reloads (backward)",
          "9 wave 0's jobs + Adam", "9 wait for the other waves", "2 X tile loads, later chunks",
          "9 wait before a reload"]


def main():
    import torch
    from mjrl_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=376)
    ap.add_argument("--m", type=int, default=17)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=1024)
    args = ap.parse_args()
    K = _lib.calls()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=g, device=dev, dtype=torch.float32)   # noqa: E731
    n, m, h, T = args.n, args.m, args.hidden, args.rows
    shapes = [(h, n), (h,), (h, h), (h,), (m, h), (m,), (m,)]
    p = [0.05 * rnd(*s) for s in shapes]
    mo, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    obs, act, adv, ll_old = rnd(T, n), 0.5 * rnd(T, m), rnd(T), -float(m) + rnd(T)
    tf = [torch.zeros(n, device=dev), torch.ones(n, device=dev), torch.zeros(m, device=dev), torch.ones(m, device=dev)]
    idx = torch.randint(0, T, (args.steps, 64), generator=g, device=dev, dtype=torch.int64)
    nf = C.c_int64()
    K.mjrl_policy_fit_scratch(n, m, h, h, 64, nf)
    scratch = torch.zeros(nf.value, dtype=torch.float32, device=dev)
    net = _lib.PolicyNet()
    for i in range(7):
        net.p[i], net.exp_avg[i], net.exp_avg_sq[i] = p[i].data_ptr(), mo[i].data_ptr(), v[i].data_ptr()
    data = _lib.PolicyFitData(obs.data_ptr(), act.data_ptr(), adv.data_ptr(), ll_old.data_ptr(), None,
                              *[t.data_ptr() for t in tf], T, n, m, h, h, _lib.POLICY_FIT_PPO, 0.2)
    K.mjrl_policy_fit_epoch(data, idx, args.steps, 64, net, _lib.Adam(3e-4, 0.9, 0.999, 1e-8, 0.0, 0), scratch, 0, None,
                            None, _lib.stream_ptr())
    torch.cuda.synchronize()
    cyc = scratch[8:8 + 2 * len(PHASES)].cpu().view(torch.int64).numpy()
    if not cyc.any():
        sys.exit("no stamps: MJRL_AMD_LIB must name a library built with -DMJRL_PFIT_PROF")
    tot = float(cyc.sum())
    print("k_pfit phase profile: n %d m %d hidden %d, %d steps, %.0f cycles a step" % (n, m, h, args.steps,
                                                                                      tot / args.steps))
    for name, c in zip(PHASES, cyc):
        print("  %-30s %9.0f  %5.1f%%" % (name, c / args.steps, 100.0 * c / tot))


if __name__ == "__main__":
    main()
