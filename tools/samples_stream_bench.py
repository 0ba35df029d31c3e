"""sample_mode="samples" staging at the C4v shape (n = 376, m = 17, N = 1,000,000
timesteps, horizon 1000, ragged lengths): what remains after the last environment
step until the DeviceBatch is ready.

    python tools/samples_stream_bench.py [--rows 1000000] [--n 376] [--m 17] [--horizon 1000]
                                         [--slots 64] [--reps 5] [--out FILE]

One process, one session.  A scripted lock-stepped sampler (the schedule of
samplers/samples_schedule.py, trajectories that end at seeded random lengths as
tests/stub_env.py's end by termination, observation rows drawn from a seeded f64
pool) feeds a ChunkSink as the vector sampler does: begin / rows / actions /
reward / finish / abandon per lock step.  Per repetition, alternating:

  sink_batch_s   the last lock step's sink calls have returned -> ChunkSink.batch
                 (paths) and a device synchronise (the tail copies, the run table,
                 mjrl_copy_runs over the four pools);
  from_paths_s   DeviceBatch.from_paths on the same paths (the route samples mode
                 took before), to a device synchronise;

and, on the batch's rows, the two run kernels alone against the indexed kernels on
a padded copy of the same rows ([P H][n], row ep H + t), by device events:

  copy_runs_s / gather_rows_s             the observation plane, [T][n] f32
  finish_runs_s / finish_indexed_s        the value-feature matrix, [T][n + 4] f32

The first repetition warms up and is dropped.  The batch of the sink is compared
with from_paths' bit for bit in every repetition.  Prints medians, minima and the
repetition count as one JSON line (and writes it to --out).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def feed(sink, args, pool_obs, pool_act, lengths):
    """One samples-mode sampling pass into `sink`; returns the accepted paths
    (views of the pools) when the last lock step's sink calls have returned."""
    import numpy as np
    from mjrl_amd.samplers.samples_schedule import SamplesSchedule
    S, H, M = args.slots, args.horizon, len(pool_obs) - args.horizon
    sched = SamplesSchedule(args.rows)
    ep = np.full(S, -1, np.int64)
    t = np.zeros(S, np.int64)
    base = np.zeros(S, np.int64)   # where in the pools the slot's trajectory reads its rows
    done = {}

    def assign(slots):
        for s in slots:
            if not sched.may_start():
                ep[s] = -1
                continue
            k = sched.start()
            ep[s], t[s], base[s] = k, 0, (k * 7919) % M
            sink.begin(s, k)

    assign(range(S))
    while not sched.done:
        live = np.nonzero(ep >= 0)[0]
        tl = t[live]
        src = base[live] + tl
        sink.rows(live, pool_obs[src], tl)
        sink.actions(live, pool_act[src], tl)
        sink.rewards(live, pool_obs[src, 0], tl)
        t[live] += 1
        ended = []
        for s in live.tolist():
            k = int(ep[s])
            sched.step(k)
            if t[s] >= lengths[k]:
                ended.append(s)
        for s in ended:
            k, L = int(ep[s]), int(t[s])
            sink.finish(s, L, L < H)
            b = int(base[s])
            done[k] = dict(observations=pool_obs[b:b + L], actions=pool_act[b:b + L],
                           rewards=pool_obs[b:b + L, 0].copy(), terminated=L < H)
            sched.end(k)
        if sched.done:
            for s in np.nonzero(ep >= 0)[0].tolist():
                if s not in ended:
                    sink.abandon(s)
            break
        assign(ended)
    return [done[k] for k in range(sched.accepted)]


def events(fn, iters):
    """Seconds per call of fn() over `iters` calls between two device events."""
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000, help="N: timesteps per batch")
    ap.add_argument("--n", type=int, default=376)
    ap.add_argument("--m", type=int, default=17)
    ap.add_argument("--horizon", type=int, default=1000)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions (one more warms up)")
    ap.add_argument("--kernel-iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from mjrl_amd import _lib
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.baselines.mlp_baseline import MLPBaseline
    from mjrl_amd.engine import DeviceBatch
    from mjrl_amd.samplers.stream_staging import ChunkSink
    from mjrl_amd.utils.gym_env import EnvSpec
    if not torch.cuda.is_available():
        sys.exit("samples_stream_bench needs a GPU")
    dev = torch.device("cuda:0")
    n, m, H, S = args.n, args.m, args.horizon, args.slots
    rs = np.random.RandomState(0)
    pool_obs = rs.randn(65536 + H, n) * 3.0   # f64 rows that are not float32s, as a simulator's
    pool_act = rs.randn(65536 + H, m)
    # ragged by termination: two trajectories in three end early, uniformly in [H / 20, H)
    count = args.rows // max(H // 20, 1) + S + 1
    lengths = np.where(rs.rand(count) < 2.0 / 3.0, rs.randint(max(H // 20, 1), H, count), H)
    base = LinearBaseline(EnvSpec(n, m, H, 1))
    base._coeffs = rs.randn(n + 4)
    res = dict(tool="samples_stream_bench", rows=args.rows, n=n, m=m, horizon=H, slots=S, reps=args.reps)
    times = {k: [] for k in ("sink_batch_s", "from_paths_s", "copy_runs_s", "gather_rows_s", "finish_runs_s",
                             "finish_indexed_s")}
    K = _lib.calls()
    for rep in range(args.reps + 1):
        sink = ChunkSink(n, m, H, args.rows, dev, baseline=base, nslots=S)
        paths = feed(sink, args, pool_obs, pool_act, lengths)
        t0 = time.perf_counter()
        got = sink.batch(paths)
        torch.cuda.synchronize()
        t_sink = time.perf_counter() - t0
        assert not sink.overflowed
        keep = {k: getattr(got, k).clone() for k in ("obs", "act", "rewards", "baseline", "path_off", "obs_range")}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = DeviceBatch.from_paths(paths, dev, baseline=base, reuse=True)
        torch.cuda.synchronize()
        t_ref = time.perf_counter() - t0
        for k, v in keep.items():
            if not torch.equal(v, getattr(ref, k)):
                sys.exit("samples_stream_bench: the sink's %s differs from from_paths'" % k)
        P, T = len(paths), ref.T
        res.update(paths=P, T=T, chunks_used=sink.next_chunk, chunks=sink.C, chunk_rows=sink.CH)
        # the kernels alone: the pool and its run table against a padded copy and its index
        with torch.cuda.device(dev):
            st = _lib.stream_ptr()
            L = ref.lengths
            offs = np.concatenate([[0], np.cumsum(L)])
            to_pad = np.stack([offs[:-1], np.arange(P) * H, L, np.zeros(P, np.int64)], 1).astype(np.int64)
            pad = torch.zeros((P * H, n), dtype=torch.float32, device=dev)
            K.mjrl_copy_runs(keep["obs"], 4 * n, torch.from_numpy(to_pad).to(dev), P, T, P * H, pad, st)
            idx = torch.from_numpy(np.concatenate([e * H + np.arange(l) for e, l in enumerate(L)]).astype(np.int64)
                                   ).to(dev)
            CH = sink.CH
            nch = -(-L // CH)
            R = int(nch.sum())
            owner = np.repeat(np.arange(P), nch)
            j = np.arange(R) - np.repeat(np.cumsum(nch) - nch, nch)
            runs = np.stack([np.concatenate([r.chunks for r in sink.accepted]).astype(np.int64) * CH,
                             offs[owner] + j * CH, np.minimum(CH, L[owner] - j * CH), j * CH], 1).astype(np.int64)
            d_runs = torch.from_numpy(runs).to(dev)
            out_a, out_b = torch.empty((T, n), dtype=torch.float32, device=dev), torch.empty(
                (T, n), dtype=torch.float32, device=dev)
            t_runs = events(lambda: K.mjrl_copy_runs(sink.obs_pad, 4 * n, d_runs, R, sink.pool_rows, T, out_a, st),
                            args.kernel_iters)
            t_gather = events(lambda: K.mjrl_gather_rows(pad, 4 * n, idx, T, out_b, st), args.kernel_iters)
            if not (torch.equal(out_a, out_b) and torch.equal(out_a, keep["obs"])):
                sys.exit("samples_stream_bench: mjrl_copy_runs and mjrl_gather_rows disagree")
            tab = MLPBaseline.time_table(H, dev)
            f_a, f_b = torch.empty((T, n + 4), dtype=torch.float32, device=dev), torch.empty(
                (T, n + 4), dtype=torch.float32, device=dev)
            t_fruns = events(lambda: K.mjrl_value_features_finish_runs(sink.obs_pad, d_runs, R, n, sink.pool_rows, T, H,
                                                                       tab, f_a, st), args.kernel_iters)
            t_fidx = events(lambda: K.mjrl_value_features_finish(pad, idx, T, n, P * H, H, tab, f_b, st),
                            args.kernel_iters)
            if not torch.equal(f_a, f_b):
                sys.exit("samples_stream_bench: the two feature-matrix kernels disagree")
            res.update(runs=R)
            del pad, idx, out_a, out_b, f_a, f_b
        if rep > 0:   # repetition 0 warms up
            for k, v in zip(times, (t_sink, t_ref, t_runs, t_gather, t_fruns, t_fidx)):
                times[k].append(v)
        del sink, got, ref, keep
    for k, xs in times.items():
        res[k] = dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
