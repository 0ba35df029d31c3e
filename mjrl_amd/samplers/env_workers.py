"""Environment worker processes for the vector sampler (sample_paths_vectorized
with num_workers >= 1): the environments of the lock-stepped batch are stepped by
a pool of processes, as the reference spreads its rollouts over num_cpu processes
(mjrl/samplers/trajectory_sampler.py:65-93), while the controller keeps the
batched device policy forward (one launch per lock step), the assignment of
trajectories to slots and the streamed staging (stream_staging.StreamSink).

  controller (sample_paths)                      worker r (slots lo_r .. hi_r - 1)
  ------------------------------------------     ----------------------------------
  assigns trajectory ep to a free slot, in
  slot order                        --reset-->   seeds the slot's environment with
                                                 seed + ep, holds RandomState(seed + ep),
                                                 resets under that stream as numpy's
                                                 global RNG, writes the observation
  means(obs board, live slots) -> mean board
                                    --step--->   per live slot: mean + scale * randn(m)
  records the step's observation / mean rows,    from the slot's stream, env.step, writes
  feeds the sink (the workers step meanwhile)    action, reward, done flag and the next
                                                 observation (other parity of the board)
  records actions / rewards, ends        <--ok-- the trajectories that ended: done, the
  trajectories, assigns the next ones            stacked env infos, the stream's state

The boards live in one multiprocessing.shared_memory segment (observations f64,
double-buffered by step parity, means f32, actions f64, rewards f64, done flags);
the control messages travel over one pipe pair per worker.  The workers are fresh
interpreters (`python -m mjrl_amd.samplers.env_workers`, started with subprocess
as pool.py starts its GPU workers); this module imports the standard library and
numpy only, so a worker never loads torch or the HIP library and never opens a
GPU.  Each trajectory is the one the in-process loop of vector_sampler.py
produces for the same seed (the same per-trajectory streams, draws and order).

Any failure (a worker that died, an exception in an environment's reset / step,
a reply that did not come within `timeout`) kills every worker, unlinks the
segment, forgets the pool and raises RuntimeError naming the worker and the
phase; the next call starts a fresh pool.
"""
import atexit
import math
import os
import pickle
import subprocess
import sys
import time
import traceback
from multiprocessing import connection, shared_memory

import numpy as np

from .samples_schedule import SamplesSchedule

RUNNING, ENDED, ENDED_DONE = 0, 1, 2   # the done board


# _seed_env and _stack restate vector_sampler's helpers: a worker cannot import
# that module (it imports torch)
def _seed_env(env, seed):
    try:
        env.env._seed(seed)
    except AttributeError:
        env.env.seed(seed)


def _stack(dicts):
    """tensor_utils.stack_tensor_dict_list: a list of (nested) dicts -> a dict of arrays."""
    if not dicts:
        return {}
    out = {}
    for k, v in dicts[0].items():
        vals = [d[k] for d in dicts]
        out[k] = _stack(vals) if isinstance(v, dict) else np.array(vals)
    return out


class _Boards:
    """Byte offsets of the per-slot boards in the shared segment (page-aligned
    fields): obs [2][S][n] f64, mean [S][m] f32, act [S][m] f64, rew [S] f64,
    done [S] u8."""

    def __init__(self, S, n, m):
        self.S, self.n, self.m = S, n, m
        off = 0
        self.fields = {}
        for name, shape, dt in (("obs", (2, S, n), np.float64), ("mean", (S, m), np.float32),
                                ("act", (S, m), np.float64), ("rew", (S,), np.float64), ("done", (S,), np.uint8)):
            self.fields[name] = (off, shape, np.dtype(dt))
            off += -(-int(np.prod(shape)) * np.dtype(dt).itemsize // 4096) * 4096
        self.nbytes = off

    def views(self, buf):
        return {k: np.ndarray(shape, dtype=dt, buffer=buf, offset=off) for k, (off, shape, dt) in self.fields.items()}


def _factory_spec(env):
    """('name', env_name) or ('pickle', bytes) of an environment factory, as it
    travels to the workers; ValueError for a factory that does not pickle."""
    if isinstance(env, str):
        return ("name", env)
    if not callable(env):
        raise ValueError("env must be an environment name or a factory, got %r" % (env,))
    try:
        return ("pickle", pickle.dumps(env, protocol=pickle.HIGHEST_PROTOCOL))
    except Exception as e:
        raise ValueError("the environment factory %r does not pickle (%s: %s); environment workers need a "
                         "module-level callable or a functools.partial of one" % (env, type(e).__name__, e)) from e


class EnvWorkerPool:
    """min(num_workers, nslots) worker processes, each owning a contiguous range
    of the nslots environment slots (one environment per slot), driven from this
    process.  env: an environment name (mjrl.utils.get_environment) or a
    picklable factory; n, m: observation / action widths; timeout: seconds any
    wait for the workers may take."""

    def __init__(self, env, num_workers, nslots, n, m, timeout=900.0):
        spec = _factory_spec(env)   # before any process starts
        self.S, self.n, self.m = int(nslots), int(n), int(m)
        if self.S < 1 or int(num_workers) < 1:
            raise ValueError("EnvWorkerPool needs at least one worker and one slot")
        self.world = W = min(int(num_workers), self.S)
        self.timeout = float(timeout)
        q, r = divmod(self.S, W)
        self.bounds = [(k * q + min(k, r), (k + 1) * q + min(k + 1, r)) for k in range(W)]
        self.owner = np.concatenate([np.full(hi - lo, k, np.int64) for k, (lo, hi) in enumerate(self.bounds)])
        self._boards = _Boards(self.S, self.n, self.m)
        self._procs, self._tx, self._rx = [], [], []
        self._unreg = None
        self.shm = shared_memory.SharedMemory(create=True, size=self._boards.nbytes)
        self.shm_name = self.shm.name
        self.v = self._boards.views(self.shm.buf)
        env_ = dict(os.environ)
        # a worker is one of `world` processes sharing the host's CPUs: no BLAS / OpenMP
        # thread team each
        env_.update(OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
        # the package's own root first: an import through '' (the caller's cwd)
        # does not survive a chdir of the caller
        root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        env_["PYTHONPATH"] = os.pathsep.join([root] + [os.path.abspath(p) for p in sys.path if p and os.path.isdir(p)])
        try:
            for k, (lo, hi) in enumerate(self.bounds):
                c2w_r, c2w_w = os.pipe()
                w2c_r, w2c_w = os.pipe()
                try:
                    cmd = [sys.executable, "-u", "-m", "mjrl_amd.samplers.env_workers", "--rank", str(k),
                           "--rfd", str(c2w_r), "--wfd", str(w2c_w)]
                    self._procs.append(subprocess.Popen(cmd, env=env_, pass_fds=(c2w_r, w2c_w)))
                finally:
                    os.close(c2w_r)
                    os.close(w2c_w)
                    self._tx.append(connection.Connection(c2w_w, readable=False))
                    self._rx.append(connection.Connection(w2c_r, writable=False))
                self._tx[k].send(dict(spec=spec, shm=self.shm_name, S=self.S, n=self.n, m=self.m, lo=lo, hi=hi))
            hello = self._gather(range(W), "start")
            self.hello = [hello[k] for k in range(W)]   # by rank
            self.horizon = self.hello[0]["horizon"]
        except BaseException:
            self._abort()
            raise

    # ---- plumbing -------------------------------------------------------------
    def _gather(self, ranks, phase):
        """One reply from every worker of `ranks`, in any order, as {rank: payload}.
        An error reply, a dead worker or `timeout` seconds without all of them
        raises RuntimeError (the caller aborts the pool)."""
        out = {}
        pending = {self._rx[k]: k for k in ranks}
        t0 = time.time()
        while pending:
            for c in connection.wait(list(pending), timeout=0.25):
                k = pending.pop(c)
                try:
                    msg = c.recv()
                except (EOFError, OSError):
                    self._procs[k].wait()
                    raise RuntimeError("mjrl_amd env worker %d exited with code %s during %s"
                                       % (k, self._procs[k].returncode, phase)) from None
                if msg[0] == "error":
                    raise RuntimeError("mjrl_amd env worker %d failed in %s%s:\n%s"
                                       % (k, msg[1], "" if msg[2] is None else " (slot %d, trajectory %d)" % msg[2],
                                          msg[3]))
                out[k] = msg[1]
            for c, k in pending.items():
                if self._procs[k].poll() is not None and not c.poll(0):
                    raise RuntimeError("mjrl_amd env worker %d exited with code %s during %s"
                                       % (k, self._procs[k].returncode, phase))
            if pending and time.time() - t0 > self.timeout:
                raise RuntimeError("mjrl_amd env workers %s did not answer within %.0f s during %s"
                                   % (sorted(pending.values()), self.timeout, phase))
        return out

    def _send(self, k, msg, phase):
        try:
            self._tx[k].send(msg)
        except (OSError, ValueError):
            raise RuntimeError("mjrl_amd env worker %d is gone (code %s) at %s"
                               % (k, self._procs[k].poll(), phase)) from None

    def alive(self):
        return bool(self._procs) and all(p.poll() is None for p in self._procs)

    def register_host(self):
        """hipHostRegister of the segment (engine.register_host), so the per-step
        copy of the observation board to the device runs as DMA out of it."""
        if self._unreg is None:
            from ..engine import register_host
            self._unreg = register_host(np.ndarray((self.shm.size,), np.uint8, buffer=self.shm.buf)) or False

    def _free_segment(self):
        if self._unreg:
            import torch
            torch.cuda.synchronize()
            self._unreg()
        self._unreg = None
        self.v = None
        if self.shm is not None:
            try:
                self.shm.close()
            except BufferError:
                pass   # still viewed by a frame that is unwinding: the mapping goes with its views
            try:
                self.shm.unlink()
            except FileNotFoundError:
                pass
            self.shm = None

    def _reap(self, grace):
        for c in self._tx:
            try:
                c.close()   # EOF ends a worker that is still listening
            except Exception:
                pass
        for p in self._procs:
            try:
                p.wait(timeout=grace)
            except Exception:
                p.kill()
                p.wait()
        for c in self._rx:
            try:
                c.close()
            except Exception:
                pass
        self._tx, self._rx = [], []
        self._free_segment()
        for key, v in list(_POOLS.items()):
            if v is self:
                del _POOLS[key]

    def _abort(self):
        """After any failure: kill every worker (one may be inside an environment
        step, another hold a stale reply), unlink the segment and forget the pool,
        so the next use starts a fresh one."""
        for p in self._procs:
            if p.poll() is None:
                p.kill()
        self._reap(30)

    def close(self):
        for c in self._tx:
            try:
                c.send(("close",))
            except Exception:
                pass
        self._reap(10)

    # ---- the protocol -----------------------------------------------------------
    def begin(self, cfg):
        """A sampling call starts: cfg = dict(seed, scale, horizon) to every worker."""
        for k in range(self.world):
            self._send(k, ("start", cfg), "start")

    def reset(self, parity, items):
        """items [(slot, ep)]: every slot's worker starts trajectory ep in it and
        writes its first observation into obs[parity][slot]."""
        per = {}
        for slot, ep in items:
            per.setdefault(int(self.owner[slot]), []).append((int(slot), int(ep)))
        for k, its in per.items():
            self._send(k, ("reset", parity, its), "reset")
        self._gather(per, "reset")

    def step_send(self, parity, ranks):
        for k in ranks:
            self._send(k, ("step", parity), "step")

    def step_wait(self, ranks):
        """{slot: (done, env_infos, rng_state)} of the trajectories that ended."""
        ended = {}
        for payload in self._gather(ranks, "step").values():
            for slot, done, einfo, state in payload:
                ended[slot] = (done, einfo, state)
        return ended


_POOLS = {}


def get_env_pool(env, num_workers, nslots, n, m, timeout=900.0):
    """The process-wide pool for this factory, worker count, slot count and
    widths: started on first use, kept across calls, closed at exit.  One pool at
    a time: another key closes the pool before it."""
    key = (_factory_spec(env), min(int(num_workers), int(nslots)), int(nslots), int(n), int(m))
    pool = _POOLS.get(key)
    if pool is not None and not pool.alive():
        pool._abort()
        pool = None
    if pool is None:
        close_env_pools()
        pool = _POOLS[key] = EnvWorkerPool(env, num_workers, nslots, n, m, timeout)
    pool.timeout = float(timeout)
    return pool


@atexit.register
def close_env_pools():
    while _POOLS:
        _, pool = _POOLS.popitem()
        try:
            pool.close()
        except Exception:
            pass


def sample_paths(pool, N, means, log_std, T=1e6, pegasus_seed=None, sink=None, sample_mode="trajectories"):
    """N trajectories (sample_mode="samples": the shortest prefix of trajectories
    with at least N timesteps, samples_schedule.py) on the pool's slots; the paths of
    vector_sampler's in-process loop for the same arguments.

    means(obs [S][n] f64, live int32 [E], out=mean [S][m] f32): the mean provider;
    it writes rows `live` of out (BatchedPolicy.means_slots in production, any
    row-wise forward in a test).  log_std: the policy's log_std_val (f64 [m]).
    sink: as sample_paths_vectorized's."""
    S, n, m = pool.S, pool.n, pool.m
    if sample_mode not in ("trajectories", "samples"):
        raise ValueError("sample_mode must be 'trajectories' or 'samples', got %r" % (sample_mode,))
    if N <= 0:
        return []
    if sample_mode == "samples" and pegasus_seed is None:
        pegasus_seed = 0   # batch_sampler.py:87
    if S != min(S, int(N)):
        raise ValueError("a pool of %d slots for %d trajectories" % (S, N))
    horizon = min(T, pool.horizon)
    H = int(math.ceil(horizon))
    if callable(sink):   # a factory: sink(N, horizon, slots)
        sink = sink(N, int(horizon), S)
    if sink is not None and (sink.N != N or sink.H < horizon or len(sink.buf) < S):
        raise ValueError("StreamSink sized for %d paths x %d steps on %d slots; sampling %d x %d on %d"
                         % (sink.N, sink.H, len(sink.buf), N, horizon, S))
    log_std = np.float64(log_std)
    try:
        return _sample(pool, int(N), means, log_std, horizon, H, pegasus_seed, sink,
                       SamplesSchedule(N) if sample_mode == "samples" else None)
    except BaseException:
        pool._abort()
        raise


def _sample(pool, N, means, log_std, horizon, H, seed, sink, sched=None):
    S, n, m = pool.S, pool.n, pool.m
    v = pool.v
    obs_b, mean_b, act_b, rew_b, done_b = v["obs"], v["mean"], v["act"], v["rew"], v["done"]
    # the live trajectories' rows, [slot][t]; a finished trajectory's are copied out
    h_obs, h_act = np.empty((S, H, n)), np.empty((S, H, m))
    h_rew, h_mean = np.empty((S, H)), np.empty((S, H, m), np.float32)
    ep = np.full(S, -1, np.int64)
    t = np.zeros(S, np.int64)
    # samples mode (sched): the paths and the streams' final states by trajectory
    # index, until the schedule knows which prefix is the batch
    paths = {} if sched is not None else [None] * N
    states = {}
    last_state = None
    next_ep = 0
    pool.begin(dict(seed=seed, scale=np.exp(log_std), horizon=horizon))

    def assign(slots):
        nonlocal next_ep
        items = []
        for s in slots:
            if (not sched.may_start()) if sched is not None else next_ep >= N:
                ep[s] = -1
                continue
            if sched is not None:
                next_ep = sched.start()
            ep[s], t[s] = next_ep, 0
            items.append((s, next_ep))
            if sink is not None:
                sink.begin(s, next_ep)
            next_ep += 1
        return items

    parity = 0
    pool.reset(parity, assign(range(S)))
    while True:
        live = np.nonzero(ep >= 0)[0].astype(np.int32)
        if not len(live):
            break
        O = obs_b[parity]
        means(O, live, out=mean_b)
        ranks = sorted(set(pool.owner[live].tolist()))
        pool.step_send(parity, ranks)
        # while the workers step: this step's rows into the trajectories and the sink
        # (the workers write the next observations into the board's other parity)
        tl = t[live]
        Ol = O[live]
        h_obs[live, tl] = Ol
        h_mean[live, tl] = mean_b[live]
        if sink is not None:
            sink.rows(live, Ol, tl)
        ended = pool.step_wait(ranks)
        al, rl = act_b[live], rew_b[live]
        h_act[live, tl] = al
        h_rew[live, tl] = rl
        if sink is not None:
            sink.actions(live, al, tl)
            for s, ts, r in zip(live.tolist(), tl.tolist(), rl.tolist()):
                sink.reward(s, ts, r)
        t[live] += 1
        if sched is not None:
            for k in ep[live].tolist():
                sched.step(k)
        flagged = live[done_b[live] != RUNNING].tolist()
        if flagged != sorted(ended):
            raise RuntimeError("mjrl_amd env workers: the done board (slots %s) and the workers' replies (slots %s) "
                               "disagree" % (flagged, sorted(ended)))
        for s in flagged:
            done, einfo, state = ended[s]
            L = int(t[s])
            if sink is not None:
                sink.finish(s, L, bool(done))
            mean = h_mean[s, :L]
            paths[ep[s]] = dict(observations=h_obs[s, :L].copy(), actions=h_act[s, :L].copy(),
                                rewards=h_rew[s, :L].copy(),
                                agent_infos=dict(mean=mean.copy(), log_std=np.array([log_std] * L),
                                                 evaluation=mean.copy()),
                                env_infos=einfo, terminated=done)
            if sched is not None:
                states[int(ep[s])] = state
                sched.end(int(ep[s]))
            elif ep[s] == N - 1:
                last_state = state
        if sched is not None and sched.done:
            # the prefix 0..K is the batch; what is still live lies above K (the next
            # call's `start` clears the workers' live sets)
            for s in np.nonzero(ep >= 0)[0].tolist():
                if s not in ended and sink is not None:
                    sink.abandon(s)
            paths = [paths[k] for k in range(sched.accepted)]
            last_state = states[sched.K]
            break
        parity ^= 1
        items = assign(flagged)
        if items:
            pool.reset(parity, items)
    if last_state is not None:
        np.random.set_state(last_state)
    return paths


# ---- the worker side ---------------------------------------------------------------
class _Traj:
    __slots__ = ("ep", "rs", "t", "infos")


def _untrack(shm):
    """The controller owns (and unlinks) the segment: keep this process's
    resource tracker from unlinking it at exit."""
    try:
        from multiprocessing import resource_tracker
        resource_tracker.unregister(shm._name, "shared_memory")
    except Exception:
        pass


def _worker_main(rank, rfd, wfd):
    rx = connection.Connection(rfd, writable=False)
    tx = connection.Connection(wfd, readable=False)
    try:
        a = rx.recv()
        kind, what = a["spec"]
        if kind == "name":
            from mjrl.utils.get_environment import get_environment
            factory = lambda: get_environment(what)   # noqa: E731
        else:
            factory = pickle.loads(what)
        lo, hi, m = a["lo"], a["hi"], a["m"]
        envs = {slot: factory() for slot in range(lo, hi)}
        shm = shared_memory.SharedMemory(name=a["shm"])
        _untrack(shm)
        v = _Boards(a["S"], a["n"], m).views(shm.buf)
        obs_b, mean_b, act_b, rew_b, done_b = v["obs"], v["mean"], v["act"], v["rew"], v["done"]
        hello = dict(rank=rank, pid=os.getpid(), slots=(lo, hi), horizon=envs[lo].horizon,
                     torch="torch" in sys.modules)
    except Exception:
        tx.send(("error", "start", None, traceback.format_exc()))
        return 1
    tx.send(("hello", hello))
    cfg, live = None, {}
    while True:
        try:
            msg = rx.recv()
        except EOFError:   # the controller closed its end, or is gone
            break
        kind, where = msg[0], None
        if kind == "close":
            break
        try:
            if kind == "start":
                cfg, live = msg[1], {}
                seed, scale, horizon = cfg["seed"], cfg["scale"], cfg["horizon"]
            elif kind == "reset":
                parity = msg[1]
                for slot, ep in msg[2]:
                    where = (slot, ep)
                    env = envs[slot]
                    tr = live[slot] = _Traj()
                    tr.ep, tr.t, tr.infos = ep, 0, []
                    if seed is not None:
                        _seed_env(env, seed + ep)
                        tr.rs = np.random.RandomState(seed + ep)
                    else:
                        tr.rs = np.random.RandomState()
                    # the reset sees the trajectory's stream as numpy's global RNG (base_sampler.py:48-58)
                    saved = np.random.get_state()
                    np.random.set_state(tr.rs.get_state())
                    o = env.reset()
                    tr.rs.set_state(np.random.get_state())
                    np.random.set_state(saved)
                    obs_b[parity, slot] = np.asarray(o, dtype=np.float64).ravel()
                    done_b[slot] = RUNNING
                tx.send(("ok", None))
            elif kind == "step":
                nxt = msg[1] ^ 1
                ended = []
                for slot in sorted(live):
                    tr = live[slot]
                    where = (slot, tr.ep)
                    act = mean_b[slot] + scale * tr.rs.randn(m)
                    next_o, r, done, info = envs[slot].step(act)
                    act_b[slot] = act
                    rew_b[slot] = r
                    tr.infos.append(info)
                    tr.t += 1
                    if done == True or tr.t >= horizon:   # noqa: E712 (base_sampler.py:61: done != True)
                        done_b[slot] = ENDED_DONE if done == True else ENDED   # noqa: E712
                        ended.append((slot, done, _stack(tr.infos), tr.rs.get_state()))
                        del live[slot]
                    else:
                        obs_b[nxt, slot] = np.asarray(next_o, dtype=np.float64).ravel()
                tx.send(("ok", ended))
            else:
                raise ValueError("unknown message %r" % (kind,))
        except Exception:
            tx.send(("error", kind, where, traceback.format_exc()))
            return 1
    return 0


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    for k in ("rank", "rfd", "wfd"):
        ap.add_argument("--" + k, type=int, required=True)
    args = ap.parse_args()
    sys.exit(_worker_main(args.rank, args.rfd, args.wfd))
