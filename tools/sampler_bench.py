"""The vector sampler with and without environment worker processes
(samplers/env_workers.py), timed on environments of the Humanoid widths (376
observations, 17 actions) whose step busy-waits a given time, as a MuJoCo step
costs 50-100 us: rows/s and the wall time of one lock step for num_workers 0
(every environment in this process) and num_workers K, at several slot counts;
then train_step's post-sampling critical path with the streamed staging fed
through the workers (StreamSink.batch -> update -> readback).

    python tools/sampler_bench.py [--workers 15] [--envs 64 256] [--delays 0 50 100]
                                  [--horizon 100] [--rounds 2] [--post-paths 256 --post-horizon 1000]
                                  [--post-only] [--baseline mlp [--alternations 3]]

--baseline mlp times an MLPBaseline agent instead (sampling, the post-sampling
critical path and the baseline fit), the streamed staging off and on in turn.
Prints one JSON line per configuration and a summary line with the ratios.  The
baseline of every ratio is num_workers=0 in the same run.  Needs a GPU (the
policy forward).  Imported by the workers too (the environment class lives
here): nothing at module level imports torch."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from stub_env import StubEnv   # noqa: E402

N_OBS, N_ACT = 376, 17


class DelayEnv(StubEnv):
    """StubEnv at the Humanoid widths that never terminates; step() spins for
    delay_us microseconds (a stand-in for the physics)."""

    def __init__(self, delay_us, horizon):
        super().__init__(n=N_OBS, m=N_ACT, horizon=horizon, radius=1e30)
        self.delay = delay_us * 1e-6

    def step(self, a):
        t0 = time.perf_counter()
        out = super().step(a)
        while time.perf_counter() - t0 < self.delay:
            pass
        return out


def _env_step_us(env):
    """One step of the environment in this process (its own arithmetic and the spin)."""
    e = env()
    e.reset()
    a = np.zeros(N_ACT)
    t0 = time.perf_counter()
    for _ in range(2000):
        e.step(a)
    return (time.perf_counter() - t0) / 2000 * 1e6


def _time_sampling(policy, env, N, num_envs, workers, reps, sink=None):
    from mjrl_amd.samplers.vector_sampler import sample_paths_vectorized
    kw = dict(env=env, pegasus_seed=1, num_envs=num_envs, num_workers=workers)
    sample_paths_vectorized(min(N, num_envs), policy, 1e6, **kw)   # pool start, first launches
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        paths = sample_paths_vectorized(N, policy, 1e6, sink=sink, **kw)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=15)
    ap.add_argument("--envs", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--delays", type=float, nargs="+", default=[0, 50, 100], help="us per environment step")
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=2, help="trajectories per slot")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--post-paths", type=int, default=256, help="0: skip the post-sampling measurement")
    ap.add_argument("--post-horizon", type=int, default=1000)
    ap.add_argument("--post-delay", type=float, default=50)
    ap.add_argument("--post-only", action="store_true", help="skip the worker / in-process sampling table")
    ap.add_argument("--baseline", choices=("linear", "mlp"), default="linear",
                    help="mlp: an NPG agent with an MLPBaseline, the streamed staging on against off")
    ap.add_argument("--alternations", type=int, default=3, help="--baseline mlp: off / on pairs timed")
    args = ap.parse_args()
    import torch
    import sampler_bench   # the workers unpickle the environment factory by this module's name
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.samplers import env_workers
    from mjrl_amd.utils.gym_env import EnvSpec
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench needs a GPU (the policy forward); none is visible")
    policy = MLP(EnvSpec(N_OBS, N_ACT, args.horizon, 1), hidden_sizes=(64, 64), seed=0, init_log_std=-1.0)
    H = args.horizon
    rows = {}
    for S in ([] if args.post_only else args.envs):
        N = S * args.rounds
        for d in args.delays:
            env = functools.partial(sampler_bench.DelayEnv, d, H)
            step_us = _env_step_us(env)
            for W in (0, args.workers):
                dt, _ = _time_sampling(policy, env, N, S, W, args.reps)
                steps = args.rounds * H                       # lock steps: every trajectory runs the horizon
                world = min(W, S)
                ideal = (S if W == 0 else -(-S // world)) * step_us   # the stepping alone, us per lock step
                r = dict(num_envs=S, step_us=d, env_step_us=round(step_us, 1), num_workers=W, timesteps=N * H,
                         seconds=round(dt, 4), rows_per_s=round(N * H / dt, 1), lock_step_us=round(dt / steps * 1e6, 1),
                         overhead_us_per_lock_step=round(dt / steps * 1e6 - ideal, 1))
                rows[(S, d, W)] = r
                print(json.dumps(r), flush=True)
        env_workers.close_env_pools()
    if not args.post_only:
        summary = [dict(num_envs=S, step_us=d, workers_over_in_process=round(
            rows[(S, d, args.workers)]["rows_per_s"] / rows[(S, d, 0)]["rows_per_s"], 2))
            for S in args.envs for d in args.delays]
        print(json.dumps(dict(summary=summary, num_workers=args.workers)), flush=True)
    if args.post_paths:
        (_post_sampling_mlp if args.baseline == "mlp" else _post_sampling)(args, policy.hidden_sizes, sampler_bench)
    env_workers.close_env_pools()


def _post_sampling_mlp(args, hidden, sampler_bench):
    """An NPG agent with an MLPBaseline, train_step's own stages timed apart, the
    streamed staging off (the finished f64 paths staged after sampling, the
    features rebuilt on the host for the fit) and on (StreamSink with
    value_features), alternating: rows/s while sampling, the post-sampling critical
    path (staging or StreamSink.batch -> value forward -> update -> readback) and
    _fit_baseline; and the sampling alone with the sink fed but no features formed
    (what the feature kernel itself adds to a lock step).  Both routes compute the
    same numbers (tests/test_gpu_value_features.py); every pair starts from the
    same agent state."""
    import copy
    import torch
    from mjrl_amd.algos.npg_cg import NPG
    from mjrl_amd.baselines.mlp_baseline import MLPBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.samplers.stream_staging import StreamSink
    from mjrl_amd.samplers.vector_sampler import sample_paths_vectorized
    from mjrl_amd.utils.gym_env import EnvSpec
    N, H, S = args.post_paths, args.post_horizon, args.envs[0]
    spec = EnvSpec(N_OBS, N_ACT, H, 1)

    class Env:
        env_id = "delay-v0"
    agent = NPG(Env(), MLP(spec, hidden_sizes=hidden, seed=0, init_log_std=-1.0), MLPBaseline(spec),
                normalized_step_size=0.01, seed=1, save_logs=False, device="cuda:0")
    env = functools.partial(sampler_bench.DelayEnv, args.post_delay, H)
    dev = agent.engine().device
    theta0 = agent.policy.get_param_values().copy()
    base0 = copy.deepcopy((agent.baseline.model.state_dict(), agent.baseline.optimizer.state_dict()))

    def one(stream, features=True):
        agent.policy.set_param_values(theta0.copy(), set_new=True, set_old=True)
        agent.baseline.model.load_state_dict(base0[0])
        agent.baseline.optimizer.load_state_dict(copy.deepcopy(base0[1]))
        sinks = []

        def make(n_paths, horizon, nslots):
            sinks.append(StreamSink(N_OBS, N_ACT, horizon, n_paths, dev, baseline=agent.baseline, nslots=nslots,
                                    value_features=features))
            return sinks[-1]
        np.random.seed(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths = sample_paths_vectorized(N, agent.policy, 1e6, env=env, pegasus_seed=1, num_envs=S, device=dev,
                                        sink=make if stream else None, num_workers=args.workers)
        t1 = time.perf_counter()
        if not features:   # the sink's own feed without the feature kernel: sampling only
            torch.cuda.synchronize()
            return dict(stream="no_features", rows_per_s=round(N * H / (t1 - t0), 1), sampling_s=round(t1 - t0, 4))
        if stream:
            agent._stream = sinks[0]
        agent.train_from_samples(paths, 0.995, 0.97)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        agent._fit_baseline(paths)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return dict(stream=stream, rows_per_s=round(N * H / (t1 - t0), 1), sampling_s=round(t1 - t0, 4),
                    post_sampling_ms=round((t2 - t1) * 1e3, 2), fit_baseline_ms=round((t3 - t2) * 1e3, 2))
    for stream in (False, True):   # warm-up: the pool, first launches, the slabs, the captured fit step
        one(stream)
    runs = []
    for _ in range(args.alternations):
        for stream in (False, True):
            runs.append(one(stream))
            print(json.dumps(runs[-1]), flush=True)
        print(json.dumps(one(True, features=False)), flush=True)
    out = dict(timesteps=N * H, num_envs=S, num_workers=args.workers, step_us=args.post_delay)
    for stream in (False, True):
        mine = [r for r in runs if r["stream"] == stream]
        for k in ("rows_per_s", "post_sampling_ms", "fit_baseline_ms"):
            v = [r[k] for r in mine]
            out["%s_%s" % (k, "on" if stream else "off")] = dict(median=float(np.median(v)), min=min(v), max=max(v))
    print(json.dumps(out), flush=True)


def _post_sampling(args, hidden, sampler_bench):
    """From the sampler's return to the update's readback, the sink fed through
    the workers: StreamSink.batch (the last runs' copies, the 1-D slots) and one
    NPG update."""
    import torch
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.engine import UpdateEngine
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.samplers.stream_staging import StreamSink
    from mjrl_amd.utils.gym_env import EnvSpec
    N, H, S = args.post_paths, args.post_horizon, args.envs[0]
    dev = torch.device("cuda:0")
    spec = EnvSpec(N_OBS, N_ACT, H, 1)
    policy = MLP(spec, hidden_sizes=hidden, seed=0, init_log_std=-1.0)
    base = LinearBaseline(spec)
    base._coeffs = np.random.RandomState(1).randn(N_OBS + 4) * 1e-3
    eng = UpdateEngine(N_OBS, N_ACT, hidden, device=dev)
    theta = torch.from_numpy(policy.get_param_values().astype(np.float32)).to(dev)
    env = functools.partial(sampler_bench.DelayEnv, args.post_delay, H)
    out = []
    for rep in range(3):   # the first is the warm-up
        sinks = []

        def make(n_paths, horizon, nslots):
            sinks.append(StreamSink(N_OBS, N_ACT, horizon, n_paths, dev, baseline=base, nslots=nslots))
            return sinks[-1]
        dt, paths = _time_sampling(policy, env, N, S, args.workers, 1, sink=make)
        t0 = time.perf_counter()
        b = sinks[-1].batch(paths)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        eng.update(b, theta.clone(), algo="npg", gamma=0.995, gae_lambda=0.97, n_step_size=0.01, trpo_verbose=False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:
            out.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, dt))
    med = lambda k: round(float(np.median([o[k] for o in out])), 2)   # noqa: E731
    print(json.dumps(dict(post_sampling_ms=med(0), batch_ms=med(1), update_ms=med(2), sampling_s=med(3),
                          timesteps=N * H, num_envs=S, num_workers=args.workers, step_us=args.post_delay)), flush=True)


if __name__ == "__main__":
    main()
