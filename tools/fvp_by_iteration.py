"""FVP accumulate time by CG iteration: the update of `bench.py` (the same batch,
parameters and arguments) run eagerly with UpdateEngine.kernel_timing on, whose
(start, accumulate done, gather done) HIP-event triples come in CG order, ten per
update.  Prints one row per update (accumulate us of iterations 0 .. 9) and the
per-iteration median / max over the updates, to tell one slow launch in ten at a
fixed iteration from slowness spread over all of them.
    python tools/fvp_by_iteration.py [--updates 8] [--config c4] [--paths N]
MJRL_AMD_LIB selects the library build."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from mjrl_amd.engine import UpdateEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="c4", choices=sorted(bench.CONFIGS))
    ap.add_argument("--paths", type=int, default=None)
    args = ap.parse_args()
    cfg = dict(bench.CONFIGS[args.config])
    if args.paths:
        cfg["paths"] = args.paths
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    batch = bench.stage_shard(0, cfg["paths"], dev, bench.baseline_coeffs(cfg), cfg, bench.demo_share(cfg, 0, 1),
                              np.float32)
    eng = UpdateEngine(cfg["n"], cfg["m"], cfg["hidden"], device=dev)
    th = torch.from_numpy(bench.initial_theta(cfg)).to(dev)
    upd = bench.update_args(cfg, cfg["paths"] * cfg["horizon"])
    eng.graphs = False
    eng.kernel_timing = []
    rows = []
    for i in range(args.warmup + args.updates):
        eng.kernel_timing.clear()
        eng.update(batch, th, graph=False, **upd)
        th = eng.vec["theta_new"].clone()
        torch.cuda.synchronize()
        if i >= args.warmup:
            rows.append([1e3 * a.elapsed_time(b) for a, b, _ in eng.kernel_timing])
    k = min(len(r) for r in rows)
    acc = np.array([r[:k] for r in rows])
    print("%s  %s  rows %d: FVP accumulate, us by CG iteration (HIP events)" % (
        os.environ.get("MJRL_AMD_LIB", "default"), args.config, batch.T))
    print("update  " + " ".join("%7d" % i for i in range(k)))
    for u, r in enumerate(acc):
        print("%6d  " % u + " ".join("%7.1f" % x for x in r))
    print("median  " + " ".join("%7.1f" % x for x in np.median(acc, axis=0)))
    print("max     " + " ".join("%7.1f" % x for x in acc.max(axis=0)))
    print("all launches: median %.1f  mean %.1f  max %.1f" % (np.median(acc), acc.mean(), acc.max()))


if __name__ == "__main__":
    main()
