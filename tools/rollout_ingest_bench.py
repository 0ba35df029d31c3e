"""DeviceBatch.from_rollout against DeviceBatch.from_paths on the same samples, at
the Humanoid shape: E = 1000 environments x H = 1000 steps (1M rows, n = 376,
m = 17, float32), every environment done every 250 - 1000 steps.

    python tools/rollout_ingest_bench.py [--envs 1000] [--steps 1000] [--n 376] [--m 17] [--alternations 5] [--carry]

One process times three things: from_rollout on the step-major device tensors,
from_paths (float32 staging, reused buffers) on the equivalent host paths
(rollout_ingest.rollout_to_paths, made once, untimed), and the two kernels alone
(mjrl_rollout_segments, mjrl_rollout_pack; device events).  The runs alternate: a
warm-up round whose times are dropped, then `--alternations` rounds.  A call is
timed on the host clock from its start to a device synchronise after it.  Prints
the medians and ranges as one JSON line, with the pack's share of its floor
(bytes read plus bytes written over 8 TB/s) and the ratio to from_paths; exits 1
unless the median of from_rollout is below the minimum of from_paths.  --carry: every
round also times from_rollout with a RolloutCarry (the episodes of the call before
continued; the carry advances from round to round), mjrl_rollout_segments_carry alone
and mjrl_returns_seeded alone on the rollout's paths (one open fragment per env), in
the same alternation, and reports whether the carried route's median lies inside the
plain route's own range; the round then ends with an untimed from_paths and kernel
pair, so that both timed from_rollout calls follow the same work.  Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def summary(xs):
    return dict(median_ms=1e3 * statistics.median(xs), min_ms=1e3 * min(xs), max_ms=1e3 * max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--n", type=int, default=376)
    ap.add_argument("--m", type=int, default=17)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--carry", action="store_true", help="also time the carried route and the seeded returns")
    args = ap.parse_args()
    import numpy as np
    import torch
    from mjrl_amd import _lib
    from mjrl_amd.engine import DeviceBatch
    from mjrl_amd.samplers import rollout_ingest as RI
    H, E, n, m = args.steps, args.envs, args.n, args.m
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    obs = torch.randn((H, E, n), generator=g, device=dev, dtype=torch.float32)
    act = torch.randn((H, E, m), generator=g, device=dev, dtype=torch.float32)
    rew = torch.randn((H, E), generator=g, device=dev, dtype=torch.float32)
    rs = np.random.RandomState(0)
    done = np.zeros((H, E), np.uint8)
    for e in range(E):   # an episode of 250 - 1000 steps after another
        t = -1
        while True:
            t += int(rs.randint(min(250, H), min(1000, H) + 1))
            if t >= H:
                break
            done[t, e] = 1
    d_done = torch.from_numpy(done).to(dev)
    paths = RI.rollout_to_paths(obs, act, rew, done)
    T, P = H * E, len(paths)

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def roll():
        return DeviceBatch.from_rollout(obs, act, rew, d_done, reuse=True)

    def stage():
        return DeviceBatch.from_paths(paths, dev, obs_dtype=np.float32, reuse=True)

    carry = RI.RolloutCarry(E, dev) if args.carry else None

    def roll_carry():
        return DeviceBatch.from_rollout(obs, act, rew, d_done, reuse=True, carry=carry)

    # the kernels alone, on buffers of their own
    K, st = _lib.calls(), _lib.stream_ptr()
    i64 = dict(dtype=torch.int64, device=dev)
    nw, nf = C.c_int64(), C.c_int64()
    K.mjrl_rollout_segments_scratch(E, nw)
    K.mjrl_rollout_pack_scratch(T, n, nf)
    env_row, off, counts = torch.zeros(E + 1, **i64), torch.zeros(T + 1, **i64), torch.zeros(2, **i64)
    term = torch.zeros(T, dtype=torch.uint8, device=dev)
    seg = torch.zeros(max(nw.value, 1), **i64)
    o, a = torch.empty((T, n), dtype=torch.float32, device=dev), torch.empty((T, m), dtype=torch.float32, device=dev)
    r = torch.empty(T, dtype=torch.float64, device=dev)
    rng, part = torch.empty((2, n), dtype=torch.float32, device=dev), torch.empty(nf.value, dtype=torch.float32, device=dev)

    def kernels():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        K.mjrl_rollout_segments(d_done, None, None, H, E, T, env_row, off, term, counts, seg, st)
        ev[1].record()
        K.mjrl_rollout_pack(obs, act, rew, 0, 0, None, env_row, H, E, n, m, T, o, a, r, rng, part, st)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / 1e3, ev[1].elapsed_time(ev[2]) / 1e3

    if args.carry:
        t0, env_path = torch.zeros(T, **i64), torch.zeros(E + 1, **i64)
        steps_k = torch.zeros(E, **i64)
        base = torch.randn(T, generator=g, device=dev, dtype=torch.float64)
        rew64, ret = rew.double().t().contiguous().view(-1), torch.empty(T, dtype=torch.float64, device=dev)

    def carry_kernels():
        """after kernels(): off / term hold the rollout's path table"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        K.mjrl_rollout_segments_carry(d_done, None, None, H, E, T, steps_k, env_row, off, term, t0, env_path, steps_k,
                                      counts, seg, st)
        ev[1].record()
        ev[2].record()
        K.mjrl_returns_seeded(rew64, base, off, term, P, 0.995, ret, st)
        ev[3].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / 1e3, ev[2].elapsed_time(ev[3]) / 1e3

    times = dict(from_rollout=[], from_paths=[], segments=[], pack=[])
    if args.carry:
        times.update(from_rollout_carry=[], segments_carry=[], returns_seeded=[])
    for it in range(args.alternations + 1):   # round 0 warms up
        tr, b = sync_time(roll)
        assert (b.T, b.P) == (T, P)
        tp, b = sync_time(stage)
        assert (b.T, b.P) == (T, P)
        ts, tk = kernels()
        if it:
            for k, v in (("from_rollout", tr), ("from_paths", tp), ("segments", ts), ("pack", tk)):
                times[k].append(v)
        if args.carry:
            tc, b = sync_time(roll_carry)
            assert (b.T, b.P) == (T, P) and b.path_t0 is not None
            tsc, trs = carry_kernels()
            # the next round's plain call then follows what the carried one followed (50 ms
            # of host staging, then the two kernels): a from_rollout that followed another
            # one closely instead measured 0.10-0.12 ms faster, whichever route it took
            stage()
            kernels()
            if it:
                for k, v in (("from_rollout_carry", tc), ("segments_carry", tsc), ("returns_seeded", trs)):
                    times[k].append(v)
    pack_bytes = T * (2 * 4 * (n + m) + 4 + 8)   # rows read and written, f32 reward in, f64 out
    floor = pack_bytes / HBM_BYTES_PER_S
    res = {k: summary(v) for k, v in times.items()}
    res.update(rows=T, paths=P, envs=E, steps=H, n=n, m=m, alternations=args.alternations, pack_bytes=pack_bytes,
               pack_floor_ms=1e3 * floor, pack_floor_fraction=floor / statistics.median(times["pack"]),
               ratio_from_paths_over_from_rollout=statistics.median(times["from_paths"]) /
               statistics.median(times["from_rollout"]))
    ok = statistics.median(times["from_rollout"]) < min(times["from_paths"])
    res["from_rollout_median_below_from_paths_min"] = ok
    if args.carry:
        med = statistics.median(times["from_rollout_carry"])
        res["carry_median_inside_plain_range"] = min(times["from_rollout"]) <= med <= max(times["from_rollout"])
        res["open_paths"] = int((term[:P] == 0).sum())
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
