"""PPO.train_from_rollout against the host route on the same rollout, and the device
minibatch draw against the host draw: E = 4096 environments x H = 32 steps (131072
rows), mb_size = 4096, 10 epochs (320 Adam steps per update), fit_backend = "hip_rows",
at Swimmer's widths (n = 8, m = 2, hidden (64, 64)) and Humanoid's (376, 17, (64, 64)).

    python tools/ppo_rollout_bench.py [--envs 4096] [--steps 32] [--mb 4096] [--epochs 10] [--alternations 5]

One process per run times, per shape, in alternation (a warm-up round whose times are
dropped, then `--alternations` rounds; a call is timed on the host clock from its start
to a device synchronise after it):
  update_device         PPO.train_from_rollout on the device tensors, minibatch_draw = "numpy";
  update_host           the same rollout through .cpu(), rollout_ingest.rollout_to_paths and
                        train_from_samples (what a PPO user did before the device route);
  update_device_draw    PPO.train_from_rollout with minibatch_draw = "device";
  draw_numpy            one epoch's indices by choice_batches (host draw plus upload);
  draw_device           one epoch's indices by device_choice_batches (one kernel).
Each update variant has an agent of its own (the same initial policy); no baseline fit
in any of them.  Prints one JSON line per shape with medians and minima.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = (("swimmer", 8, 2, (64, 64)), ("humanoid", 376, 17, (64, 64)))


def summary(xs):
    return dict(median_ms=1e3 * statistics.median(xs), min_ms=1e3 * min(xs))


class _Env:
    env_id = "ppo-rollout-bench-v0"


def run(name, n, m, hidden, args):
    import numpy as np
    import torch
    from mjrl_amd.algos._device_sgd import choice_batches, device_choice_batches
    from mjrl_amd.algos.ppo_clip import PPO
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.samplers import rollout_ingest as RI
    from mjrl_amd.utils.gym_env import EnvSpec
    H, E = args.steps, args.envs
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    roll = dict(observations=torch.randn((H, E, n), generator=g, device=dev),
                actions=torch.randn((H, E, m), generator=g, device=dev),
                rewards=torch.randn((H, E), generator=g, device=dev),
                done=(torch.rand((H, E), generator=g, device=dev) < 0.02).to(torch.uint8))
    T = H * E

    def agent(draw):
        spec = EnvSpec(n, m, 1000, 1)
        a = PPO(_Env(), MLP(spec, hidden_sizes=hidden, seed=0), LinearBaseline(spec), epochs=args.epochs,
                mb_size=args.mb, learn_rate=3e-4, seed=1, device=dev)
        a.fit_backend, a.minibatch_draw = "hip_rows", draw
        return a

    a_dev, a_host, a_draw = agent("numpy"), agent("numpy"), agent("device")

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def host_route():
        paths = RI.rollout_to_paths(**{k: v.cpu() for k, v in roll.items()})
        a_host.train_from_samples(paths, 0.995, 0.98)

    first = [0]

    def draw_device():
        _, first[0] = device_choice_batches(1, first[0], T, args.mb, dev)

    variants = dict(
        update_device=lambda: a_dev.train_from_rollout(fit_baseline=False, **roll),
        update_host=host_route,
        update_device_draw=lambda: a_draw.train_from_rollout(fit_baseline=False, **roll),
        draw_numpy=lambda: choice_batches(T, args.mb, dev),
        draw_device=draw_device)
    times = {k: [] for k in variants}
    np.random.seed(0)
    for it in range(args.alternations + 1):   # round 0 warms up
        for k, fn in variants.items():
            t = sync_time(fn)
            if it:
                times[k].append(t)
    res = {k: summary(v) for k, v in times.items()}
    med = lambda k: statistics.median(times[k])
    res.update(shape=name, n=n, m=m, hidden=list(hidden), envs=E, steps=H, rows=T, mb_size=args.mb, epochs=args.epochs,
               adam_steps=args.epochs * (T // args.mb), alternations=args.alternations,
               ratio_update_host_over_device=med("update_host") / med("update_device"),
               ratio_draw_numpy_over_device=med("draw_numpy") / med("draw_device"),
               draws_share_of_update_numpy=args.epochs * med("draw_numpy") / med("update_device"),
               update_saved_by_device_draw_ms=1e3 * (med("update_device") - med("update_device_draw")))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--mb", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=5)
    args = ap.parse_args()
    for shape in SHAPES:
        run(*shape, args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
