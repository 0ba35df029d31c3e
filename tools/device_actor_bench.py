"""One environment step of action sampling for a device rollout, two routes in one
session, at the shapes and batch sizes device rollouts run at.

    python tools/device_actor_bench.py [--repeats 9] [--steps 64] [--out profiles/device_actor/bench.json]

Route A is what the package offered before mjrl_policy_act: mjrl_policy_mean on the
device observations, torch.randn for the noise, one addcmul (mean + sigma * noise)
into the action slab and a copy of the observations into the observation slab: four
launches per step.  Route B is one mjrl_policy_act launch with obs_copy, writing
both slabs.  Shapes (n / m / hidden): Swimmer 8 / 2 / (64, 64), HalfCheetah 17 / 6 /
(128, 128), Humanoid 376 / 17 / (64, 64), door 39 / 28 / (256, 256), each at E = 256,
4096 and 16384 environments, float32.

A sample is `--steps` consecutive steps between two HIP events (the slabs are
[steps][E][...]: every step writes its own rows, as a collection does), divided by
the step count.  Per configuration: one warm-up sample of each route, then
`--repeats` rounds that alternate A and B; the median and the minimum per step of
each route are reported, with the host time to enqueue a step (when the event time
is no larger than it, the route is bound by its launches, not by its kernels) and,
for B, the first-layer weight bytes its tiles read from L2 per step.  The bar, for
E >= 4096: B's median below A's minimum.  Prints one JSON line (also written to
--out) and exits 1 if a bar is missed.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [("swimmer", 8, 2, (64, 64)), ("halfcheetah", 17, 6, (128, 128)), ("humanoid", 376, 17, (64, 64)),
          ("door", 39, 28, (256, 256))]
ENVS = (256, 4096, 16384)
TILE = 16   # rows per workgroup of k_policy_act (csrc/act.hip)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from mjrl_amd import _lib
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.samplers.device_actor import DeviceActor
    from mjrl_amd.utils.gym_env import EnvSpec
    if not torch.cuda.is_available():
        print("device_actor_bench needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    S = args.steps
    results, ok = [], True
    for name, n, m, hidden in SHAPES:
        pol = MLP(EnvSpec(n, m, 1000, 1), hidden_sizes=hidden, seed=0)
        rs = np.random.RandomState(n)
        for mdl in (pol.model, pol.old_model):   # a normalised policy, as trained ones are
            mdl.set_transformations(rs.randn(n), rs.rand(n) + 0.5, 0.1 * rs.randn(m), rs.rand(m) + 0.5)
        actor = DeviceActor(pol, dev, seed=1)
        bp = actor._batched(dev)
        eng, K, st = bp.eng, bp.eng.K, _lib.stream_ptr()
        tr = eng.transforms
        for E in ENVS:
            g = torch.Generator(device=dev).manual_seed(E)
            obs = torch.randn((E, n), generator=g, device=dev)
            obs_slab = torch.empty((S, E, n), device=dev)
            act_slab = torch.empty((S, E, m), device=dev)
            mean, noise = torch.empty((E, m), device=dev), torch.empty((E, m), device=dev)
            sigma = actor.sigma

            def route_a(t):
                K.mjrl_policy_mean(eng.shape, obs, E, bp.packed, *tr, mean, st)
                torch.randn((E, m), out=noise)
                torch.addcmul(mean, sigma, noise, out=act_slab[t])
                obs_slab[t].copy_(obs)

            def route_b(t):
                K.mjrl_policy_act(eng.shape, obs, 0, E, bp.packed, *tr, sigma, 1, t, 0, act_slab[t], None, None,
                                  obs_slab[t], st)

            def sample(route):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                h0 = time.perf_counter()
                e0.record()
                for t in range(S):
                    route(t)
                e1.record()
                host = time.perf_counter() - h0
                torch.cuda.synchronize()
                return 1e3 * e0.elapsed_time(e1) / S, 1e6 * host / S   # us per step: device events, host enqueue

            sample(route_a), sample(route_b)   # warm-up: code objects, allocator
            ta, tb, ha, hb = [], [], [], []
            for _ in range(args.repeats):
                a, h = sample(route_a)
                ta.append(a), ha.append(h)
                b, h = sample(route_b)
                tb.append(b), hb.append(h)
            assert torch.equal(obs_slab[S - 1], obs)
            tiles = (E + TILE - 1) // TILE
            r = dict(shape=name, n=n, m=m, hidden=list(hidden), E=E, steps=S, repeats=args.repeats,
                     a_median_us=statistics.median(ta), a_min_us=min(ta), a_max_us=max(ta),
                     b_median_us=statistics.median(tb), b_min_us=min(tb), b_max_us=max(tb),
                     a_host_enqueue_us=statistics.median(ha), b_host_enqueue_us=statistics.median(hb),
                     a_over_b=statistics.median(ta) / statistics.median(tb),
                     b_tiles=tiles, b_w0_bytes_from_l2=tiles * eng.shape.h0 * eng.shape.np * 4,
                     flop_per_step=2 * E * (eng.shape.np * hidden[0] + hidden[0] * hidden[1] + hidden[1] * eng.shape.mp))
            if E >= 4096:
                r["bar_b_median_below_a_min"] = r["b_median_us"] < r["a_min_us"]
                ok = ok and r["bar_b_median_below_a_min"]
            results.append(r)
            print("%-11s E=%5d  A %8.1f us (min %8.1f, enqueue %6.1f)  B %7.1f us (min %7.1f, enqueue %5.1f)  A/B %5.1f"
                  % (name, E, r["a_median_us"], r["a_min_us"], r["a_host_enqueue_us"], r["b_median_us"], r["b_min_us"],
                     r["b_host_enqueue_us"], r["a_over_b"]), file=sys.stderr)
    out = dict(device=torch.cuda.get_device_name(0), results=results, all_bars_met=ok)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
