"""PPO.train_from_paths on synthetic paths with fit_backend "torch" (a captured graph
of torch ops per minibatch step) against a fused backend ("hip", csrc/policy_fit.hip,
"hip_wide", csrc/policy_fit_wide.hip, or "hip_rows", csrc/policy_fit_rows.hip), at these shapes:

    swimmer      n = 8, m = 2, hidden (64, 64), 25 paths of 500 rows, class defaults
                 (10 epochs of 195 minibatches of 64 rows: 1,950 Adam steps a call)
    humanoid     n = 376, m = 17, hidden (64, 64), 100 paths of 1000 rows, epochs = 2
                 (3,124 steps a call)
    halfcheetah  n = 17, m = 6, hidden (128, 128), 100 paths of 1000 rows, epochs = 2
                 (3,124 steps a call)
    door         n = 39, m = 28, hidden (256, 256), 200 paths of 200 rows, epochs = 4
                 (2,500 steps a call)

    python tools/policy_fit_bench.py [--alternations 3] [--timeout 300] [--shapes swimmer,humanoid]
                                     [--algo ppo|bc_mse] [--backends torch,hip] [--hidden H0,H1]
                                     [--mb-size ROWS]

--backends names the two backends that alternate (default torch,hip; torch,hip_wide for the wide
shapes, hip,hip_wide to compare the two fused ones where both run); --hidden overrides the
shapes' hidden sizes; --mb-size the minibatch rows (the classes' default is 64; "hip_rows" takes
up to 16384, the other fused backends 64; the steps a call runs shrink accordingly).

--algo bc_mse times behavior_cloning_2.BC.train() (the MSE head, mjrl_policy_mse_epoch)
instead, on synthetic expert paths of the same sizes: class defaults at swimmer (5
epochs: 975 steps a call), epochs = 2 at humanoid (3,124 steps).

The backends alternate: a warm-up pair whose times are dropped, then
`--alternations` pairs.  Every run is a child process of its own under its own
time limit (a run that fails or overruns ends the tool: nothing more is started
on the GPU after it); the child calls train_from_paths once untimed (graph
capture, code-object load; it also leaves the old and new mean networks sharing
storage, the form every later iteration has), then times one call between two
synchronisations, and within it the minibatch epochs alone.  Prints the medians
and ranges as one JSON line.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {   # n, m, paths, rows per path, PPO keyword arguments, hidden sizes
    "swimmer": (8, 2, 25, 500, {}, (64, 64)),
    "humanoid": (376, 17, 100, 1000, dict(epochs=2), (64, 64)),
    "halfcheetah": (17, 6, 100, 1000, dict(epochs=2), (128, 128)),
    "door": (39, 28, 200, 200, dict(epochs=4), (256, 256)),
}
BACKENDS = ("torch", "hip", "hip_wide", "hip_rows")


def child(args):
    import numpy as np
    import torch
    from mjrl_amd.algos import _device_sgd
    from mjrl_amd.algos.ppo_clip import PPO
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.gym_env import EnvSpec
    n, m, npaths, H, kw, hidden = SHAPES[args.shape]
    if args.hidden:
        hidden = tuple(int(h) for h in args.hidden.split(","))
    policy = MLP(EnvSpec(n, m, H, 1), hidden_sizes=hidden, seed=1, init_log_std=-0.5)
    mse = args.algo == "bc_mse"
    if args.mb_size:
        kw = dict(kw, **{"batch_size" if mse else "mb_size": args.mb_size})
    if mse:
        from mjrl_amd.algos.behavior_cloning_2 import BC
        # the constructor reads its paths for the transformations; every timed call gets its own
        rs = np.random.RandomState(9)
        agent = BC([dict(observations=rs.randn(H, n), actions=0.6 * rs.randn(H, m)) for _ in range(npaths)],
                   policy, **kw)
    else:
        agent = PPO(None, policy, None, **kw)
    agent.fit_backend = args.child
    spent = [0.0]

    def timed(fn):
        def run(self, *a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(self, *a, **k)
            torch.cuda.synchronize()
            spent[0] += time.perf_counter() - t0
        return run
    _device_sgd.DeviceTrainer.epoch = timed(_device_sgd.DeviceTrainer.epoch)
    _device_sgd.DeviceTrainer.fused_epoch = timed(_device_sgd.DeviceTrainer.fused_epoch)
    times, epochs_s = [], []
    for it in range(2):   # the first call warms up (not reported)
        rs = np.random.RandomState(10 + it)
        # actions around the fresh policy's mean (its last layer starts at 1e-2 of torch's init)
        paths = [dict(observations=rs.randn(H, n), actions=0.6 * rs.randn(H, m), rewards=rs.randn(H),
                      advantages=rs.randn(H)) for _ in range(npaths)]
        np.random.seed(5 + it)
        spent[0] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mse:
            agent.expert_paths = paths
            agent.train()
        else:
            agent.train_from_paths(paths)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        epochs_s.append(spent[0])
    steps = agent.epochs * int(npaths * H / agent.mb_size)
    theta = policy.get_param_values()
    print(json.dumps(dict(backend=args.child, shape=args.shape, call_s=times[1], epochs_s=epochs_s[1],
                          warmup_s=times[0], steps=steps, hidden=list(hidden), mb_size=agent.mb_size,
                          param_norm=float(np.linalg.norm(theta)),
                          finite=bool(np.all(np.isfinite(theta))))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per run (one child process)")
    ap.add_argument("--shapes", default="swimmer,humanoid")
    ap.add_argument("--algo", choices=("ppo", "bc_mse"), default="ppo")
    ap.add_argument("--shape", default="swimmer", help=argparse.SUPPRESS)
    ap.add_argument("--backends", default="torch,hip", help="the two backends that alternate")
    ap.add_argument("--hidden", default="", help="H0,H1 instead of the shapes' own hidden sizes")
    ap.add_argument("--mb-size", type=int, default=0, help="minibatch rows instead of the classes' 64")
    ap.add_argument("--child", choices=BACKENDS, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    pair_of = tuple(args.backends.split(","))
    if len(pair_of) != 2 or pair_of[0] == pair_of[1] or any(b not in BACKENDS for b in pair_of):
        ap.error("--backends takes two different names of %s" % (BACKENDS,))
    base, other = pair_of
    res = dict(tool="policy_fit_bench", backends=list(pair_of), shapes={})
    if args.algo != "ppo":
        res["algo"] = args.algo
    for shape in args.shapes.split(","):
        runs = {base: [], other: []}
        steps, norm, hidden, mb = 0, {}, None, None
        for pair in range(args.alternations + 1):
            for backend in pair_of:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", backend, "--shape", shape,
                       "--algo", args.algo, "--hidden", args.hidden, "--mb-size", str(args.mb_size)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
                except subprocess.TimeoutExpired:
                    sys.exit("policy_fit_bench: the %s run exceeded %g s; stopping" % (backend, args.timeout))
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-4000:])
                    sys.exit("policy_fit_bench: the %s run failed (exit %d); stopping" % (backend, r.returncode))
                out = json.loads(r.stdout.strip().splitlines()[-1])
                if not out["finite"]:
                    sys.exit("policy_fit_bench: the %s run left non-finite parameters; stopping" % backend)
                steps, norm[backend], hidden, mb = out["steps"], out["param_norm"], out["hidden"], out["mb_size"]
                if pair > 0:   # pair 0 is the warm-up pair
                    runs[backend].append((out["call_s"], out["epochs_s"]))

        def summary(xs):
            return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)
        one = dict(steps=steps, hidden=hidden, mb_size=mb, param_norm=norm)
        for k in pair_of:
            one[k + "_call_s"] = summary([c for c, _ in runs[k]])
            one[k + "_epochs_s"] = summary([e for _, e in runs[k]])
        one["us_per_step"] = {k: 1e6 * one[k + "_epochs_s"]["median"] / max(steps, 1) for k in pair_of}
        # the first backend's median over the second's
        one["speedup_epochs"] = one[base + "_epochs_s"]["median"] / one[other + "_epochs_s"]["median"]
        one["speedup_call"] = one[base + "_call_s"]["median"] / one[other + "_call_s"]["median"]
        res["shapes"][shape] = one
    print(json.dumps(res))


if __name__ == "__main__":
    main()
