"""Sampler-fed staging ("have the samplers fill pinned fp32
per-path slabs ... and overlap the H2D with" the rest of sampling).

The reference concatenates the finished f64 paths (npg_cg.py:87-89) and the
policy casts them to f32 on every forward (gaussian_mlp.py:103); the staging
path of engine.DeviceBatch.from_paths does that conversion once, but only after
sampling has finished, so the update waits for a ~3 GB f64 read and a 1.5 GB
PCIe copy at Humanoid 1M.  StreamSink moves that work INTO the
sampling loop of samplers/vector_sampler.py:

  - every lock step, the observation rows of the live environments go through
    ONE native call (mjrl_host_stage_rows_f64x) straight into their
    trajectories' pinned f32 slabs (one double-buffered slab per environment
    slot), folded into the column ranges, with the LinearBaseline prediction of
    each row computed from its f64 values (the coefficients are fixed while a
    batch is sampled: baseline.fit runs after the update) and the exactness
    flag; the actions likewise (f32);
  - every FLUSH_ROWS steps of a trajectory, its completed rows are copied to HBM
    on the staging copy stream at their fixed position (ep * H + t) of a padded
    device slab, and the rest when it ends, while the environments keep
    stepping (so the last lock step leaves at most FLUSH_ROWS rows a slot to
    copy);
  - rewards and the predictions travel the same way (8 bytes a row each);
  - with value_features=True (an MLPBaseline, whose features float32(clip(x) / 10)
    need the f64 x): every lock step, mjrl_value_features_slots forms the live
    rows' features on the device from the step's f64 observations, the board the
    batched policy forward already uploaded when the environments run in worker
    processes (attach_board), the step's rows uploaded from here otherwise, and
    writes each row at its position (ep * H + t) of a padded f32 slab; batch()
    then builds the [T][n + 4] matrix the value network reads in one pass
    (mjrl_value_features_finish), runs the forward on it and keeps it on the
    batch for the fit (batch.value_feat);
  - after sampling, batch() compacts the padded slabs into the contiguous
    layout with one device gather per slot (mjrl_gather_rows; none when every
    trajectory ran the full horizon: the padded slabs are then the batch) and
    stages the path offsets and flags.

The DeviceBatch it returns is bit-identical to DeviceBatch.from_paths on the
same paths (the same f32 rounding, the same per-row prediction arithmetic,
ranges that give the same column scales): tests/test_gpu_stream_staging.py.
What remains after the last environment step is the trajectories' last rows,
the gather, the 1-D slots and the update itself (bench.py e2e_stream).

StreamSink's device slabs are [N paths][H], which sample_mode="samples" cannot
size (the number of paths is known when sampling ends) and which must not fold
rows of trajectories that are later thrown away into the batch's ranges.
ChunkSink (below) is the sink of that mode: the same pinned side, a device pool
of fixed-size chunks sized by rows, per-trajectory ranges and flags, and a
compaction by run table (mjrl_copy_runs, mjrl_value_features_finish_runs):
tests/test_gpu_vector_samples.py, tools/samples_stream_bench.py.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..engine import DeviceBatch, _STAGING, _linear_coeffs


_SLABS = {}
_VF_BUFS = {}   # the value-feature step buffers of one (slots, n, device) at a time


class StreamSink:
    """Receives rows from the vectorised sampler and stages them as they come.

    n, m: observation / action widths; horizon: the longest trajectory; N: the
    number of trajectories; baseline: the agent's value baseline (a
    LinearBaseline's coefficients are used for the predictions, as fixed while
    the batch is sampled); nslots: the sampler's environment slots;
    value_features: form the baseline's observation features on the device while
    sampling (a baseline with predict_features_device: MLPBaseline)."""

    NBUF = 2   # slabs per environment slot: a slot starts its next trajectory while the last one's copy runs
    FLUSH_ROWS = 256   # a live trajectory's completed rows leave for HBM in runs of this many

    def __init__(self, n, m, horizon, N, device, baseline=None, nslots=64, value_features=False):
        self.n, self.m, self.H, self.N = int(n), int(m), int(horizon), int(N)
        self.device = torch.device(device)
        self.baseline = baseline
        self.value_features = bool(value_features)
        if self.value_features and not hasattr(baseline, "predict_features_device"):
            raise ValueError("StreamSink(value_features=True) needs a baseline with predict_features_device "
                             "(MLPBaseline), got %r" % (baseline,))
        c = _linear_coeffs(baseline, self.n)
        self.linear = c is not False
        self.coeffs = None if c is False or c is None else np.ascontiguousarray(c, dtype=np.float64)
        self.S = _lib.stage_calls()
        S, B, H = int(nslots), self.NBUF, self.H
        # pinned per-slot slabs, [slot][buf][H][n] f32 observations, [..][m] actions
        # and [..] f64 predictions, kept across batches (a training loop builds one
        # sink per iteration) with the copy events that guard them
        key = (S, B, H, self.n, self.m)
        ent = _SLABS.get(key)
        if ent is None:
            _SLABS.clear()   # one shape at a time
            pin = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, pin_memory=True)   # noqa: E731
            ent = _SLABS[key] = dict(obs=pin(S, B, H, self.n), act=pin(S, B, H, self.m),
                                     rew=pin(S, B, H, dt=torch.float64), pred=pin(S, B, H, dt=torch.float64),
                                     ev=[[None] * B for _ in range(S)])
        self._obs, self._act, self._rew, self._pred, self._ev = (ent[k] for k in ("obs", "act", "rew", "pred", "ev"))
        self.obs_h, self.act_h, self.rew_h, self.pred_h = (t.numpy() for t in (self._obs, self._act, self._rew,
                                                                               self._pred))
        self._row_ptr0 = self.obs_h.ctypes.data
        self.buf = np.zeros(S, np.int64)
        self.ep = np.full(S, -1, np.int64)
        self.copied = np.zeros(S, np.int64)   # rows of the slot's live trajectory already sent
        self.lo = np.full(self.n, np.inf, np.float32)
        self.hi = np.full(self.n, -np.inf, np.float32)
        self.flag = np.zeros(1, np.int32)
        self.lengths = np.zeros(self.N, np.int64)
        self.term = np.zeros(self.N, np.uint8)
        with torch.cuda.device(self.device):
            slot = lambda name, k, dt: _STAGING.device_slot(name, self.N * H * k, dt, self.device)   # noqa: E731
            self.obs_pad = slot("stream_obs", self.n, np.float32).view(self.N * H, self.n)
            self.act_pad = slot("stream_act", self.m, np.float32).view(self.N * H, self.m)
            self.rew_pad = slot("stream_rew", 1, np.float64)
            self.pred_pad = slot("stream_pred", 1, np.float64) if self.coeffs is not None else None
            self.cs = _STAGING._copy_stream(self.device)
            # the padded slabs may still be read by work queued on the current stream
            self.cs.wait_stream(torch.cuda.current_stream(self.device))
            if self.value_features:
                self._init_value_features(S)
        self.done = False

    # ---- value features (MLPBaseline) -------------------------------------------
    VF_RING = 2   # pinned per-step index (and row) buffers in rotation

    def _init_value_features(self, S):
        """feat_pad [N H][n] f32 in HBM: row ep H + t is float32(clip(x) / 10) of
        the f64 observation, written by mjrl_value_features_slots in the lock step
        that produced it.  Per step the kernel needs dest / live (and, without
        environment workers, the f64 rows themselves): small pinned buffers in
        rotation, each with the event of its last use."""
        n, dev = self.n, self.device
        self.feat_pad = _STAGING.device_slot("stream_vfeat", self.N * self.H * n, np.float32, dev).view(
            self.N * self.H, n)
        key = (S, n, dev)
        ent = _VF_BUFS.get(key)
        if ent is None:
            _VF_BUFS.clear()
            R = self.VF_RING
            # idx[r][0] = dest (int64 [S]), idx[r][1] viewed as int32: live [S]
            ent = _VF_BUFS[key] = dict(h_idx=torch.zeros((R, 2, S), dtype=torch.int64).pin_memory(),
                                       d_idx=torch.zeros((2, S), dtype=torch.int64, device=dev),
                                       h_rows=None, d_rows=None, ev=[None] * R, turn=0)
        self._vf = ent
        self._board = None
        self._vf_ev = None

    def attach_board(self, board):
        """board: the device f64 [S][n] observation board the sampler's policy
        forward uploads every lock step on the current stream
        (BatchedPolicy.obs_board): rows() then reads this step's rows there
        instead of uploading them a second time.  Ignored without value_features."""
        if not self.value_features:
            return
        if board.dtype != torch.float64 or board.dim() != 2 or board.shape[1] != self.n or \
                board.shape[0] < len(self.buf) or board.device != self.feat_pad.device or not board.is_contiguous():
            raise ValueError("StreamSink.attach_board: need a contiguous f64 [>= %d][%d] board on %s"
                             % (len(self.buf), self.n, self.device))
        self._board = board

    def _feature_rows(self, slots, obs, t):
        """mjrl_value_features_slots for this lock step's rows, on the current
        stream: the stream the board upload of this step ran on, so the next
        step's upload (queued behind it) cannot overtake the kernel."""
        vf, E, S = self._vf, len(slots), len(self.buf)
        r = vf["turn"]
        vf["turn"] = (r + 1) % self.VF_RING
        # The pinned buffers of turn r were last read by the copies of VF_RING steps
        # ago: the event recorded behind that step's copies and kernel is waited for
        # before they are rewritten, which is what makes the reuse safe.  (The policy
        # forward of every step in between ends in a synchronise of this stream,
        # BatchedPolicy.means / means_slots, so the wait returns at once.)
        if vf["ev"][r] is not None:
            vf["ev"][r].synchronize()
        h_idx, d_idx = vf["h_idx"][r], vf["d_idx"]
        h = h_idx.numpy()
        h[0, :E] = self.ep[slots] * self.H + t
        live = h[1].view(np.int32)
        with torch.cuda.device(self.device):
            if self._board is not None:
                live[:E] = slots
                src, nsrc = self._board, int(self._board.shape[0])
            else:
                # no environment workers: this step's f64 rows [E][n] go up from here
                if vf["h_rows"] is None:
                    vf["h_rows"] = torch.zeros((self.VF_RING, S, self.n), dtype=torch.float64).pin_memory()
                    vf["d_rows"] = torch.zeros((S, self.n), dtype=torch.float64, device=self.device)
                vf["h_rows"][r].numpy()[:E] = obs
                vf["d_rows"][:E].copy_(vf["h_rows"][r, :E], non_blocking=True)
                live[:E] = np.arange(E, dtype=np.int32)
                src, nsrc = vf["d_rows"], S
            d_idx.copy_(h_idx, non_blocking=True)
            _lib.calls().mjrl_value_features_slots(src, d_idx[1], d_idx[0], E, nsrc, self.n, self.N * self.H,
                                                   self.feat_pad, _lib.stream_ptr())
            ev = vf["ev"][r]
            if ev is None:
                ev = vf["ev"][r] = torch.cuda.Event()
            ev.record()
        self._vf_ev = ev

    # ---- sampler side -------------------------------------------------------
    def begin(self, slot, ep):
        """Slot `slot` starts trajectory `ep`: it writes into its other slab, once
        that slab's previous copy has completed."""
        b = (self.buf[slot] + 1) % self.NBUF
        ev = self._ev[slot][b]
        if ev is not None:
            ev.synchronize()
            self._ev[slot][b] = None
        self.buf[slot] = b
        self.ep[slot] = ep
        self.copied[slot] = 0

    def rows(self, slots, obs, t):
        """Observation rows obs [E, n] (f64) of environments `slots` at path
        indices t (the row each trajectory records at this step)."""
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        slots = np.asarray(slots, np.int64)
        t = np.ascontiguousarray(t, dtype=np.int64)
        E = len(slots)
        if E == 0:
            return
        b = self.buf[slots]
        stride_b, stride_s = self.H * self.n * 4, self.NBUF * self.H * self.n * 4
        ptrs = (C.c_void_p * E)(*(self._row_ptr0 + slots * stride_s + b * stride_b + t * self.n * 4).tolist())
        pred = np.empty(E, np.float64) if self.coeffs is not None else None
        self.S.mjrl_host_stage_rows_f64x(obs, E, self.n, ptrs, self.lo, self.hi,
                                         None if pred is None else self.coeffs, t, pred, self.flag)
        if pred is not None:
            self.pred_h[slots, b, t] = pred
        if self.value_features:
            self._feature_rows(slots, obs, t)
        # row t arriving means rows < t are complete (their actions and rewards were
        # recorded in the previous step): send full runs of them
        due = np.nonzero(t - self.copied[slots] >= self.FLUSH_ROWS)[0]
        for i in due.tolist():
            self._send(int(slots[i]), int(t[i]))

    def actions(self, slots, act, t):
        """Action rows act [E, m] of environments `slots` at path indices t."""
        slots = np.asarray(slots, np.int64)
        self.act_h[slots, self.buf[slots], np.asarray(t, np.int64)] = np.asarray(act, dtype=np.float64)

    def rewards(self, slots, rew, t):
        """Rewards rew [E] (f64) of environments `slots` at path indices t."""
        slots = np.asarray(slots, np.int64)
        self.rew_h[slots, self.buf[slots], np.asarray(t, np.int64)] = np.asarray(rew, dtype=np.float64)

    def reward(self, slot, t, r):
        """One environment's reward at path index t (the sampler's per-step call)."""
        self.rew_h[slot, self.buf[slot], t] = r

    def _send(self, slot, upto):
        """Rows [copied, upto) of slot `slot`'s live trajectory (observations,
        actions, rewards, baseline predictions) to their place in the padded
        device slabs, on the copy stream."""
        ep, b, a = int(self.ep[slot]), int(self.buf[slot]), int(self.copied[slot])
        if upto <= a:
            return
        H = self.H
        with torch.cuda.stream(self.cs):
            self.obs_pad[ep * H + a: ep * H + upto].copy_(self._obs[slot, b, a:upto], non_blocking=True)
            self.act_pad[ep * H + a: ep * H + upto].copy_(self._act[slot, b, a:upto], non_blocking=True)
            self.rew_pad[ep * H + a: ep * H + upto].copy_(self._rew[slot, b, a:upto], non_blocking=True)
            if self.pred_pad is not None:
                self.pred_pad[ep * H + a: ep * H + upto].copy_(self._pred[slot, b, a:upto], non_blocking=True)
        self.copied[slot] = upto

    def finish(self, slot, length, terminated=False):
        """Slot `slot`'s trajectory ended after `length` rows: its rows not sent yet
        leave for HBM now, on the copy stream, while sampling continues."""
        ep, b, Lr = int(self.ep[slot]), int(self.buf[slot]), int(length)
        self.lengths[ep] = Lr
        self.term[ep] = bool(terminated)
        if Lr:
            self._send(slot, Lr)
            ev = torch.cuda.Event()   # covers the trajectory's earlier runs too (one stream, in order)
            ev.record(self.cs)
            self._ev[slot][b] = ev
        self.ep[slot] = -1

    # ---- update side -------------------------------------------------------
    def batch(self, paths, reuse=True):
        """The DeviceBatch of the sampled paths (those this sink received, in
        trajectory order), as DeviceBatch.from_paths would stage them."""
        with torch.cuda.device(self.device):
            return self._batch(paths, reuse)

    def _batch(self, paths, reuse):
        N, H, dev = self.N, self.H, self.device
        lengths = np.array([len(p["rewards"]) for p in paths], dtype=np.int64)
        if len(paths) != N or not np.array_equal(lengths, self.lengths):
            raise ValueError("StreamSink.batch: the paths are not the ones the sink received")
        T = int(lengths.sum())
        cur = torch.cuda.current_stream(dev)
        cur.wait_stream(self.cs)   # every trajectory's copy

        def stage(slot, arrs, ncols, dtype=np.float64):
            return _STAGING.stage(slot, arrs, ncols, dtype, dev, reuse)

        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        off = stage("off", [offs], 0, np.int64)
        term = stage("term", [self.term], 0, np.uint8)
        orange = stage("orange", [np.stack([self.lo, self.hi])], self.n, np.float32)
        pads = [("obs", self.obs_pad, self.n, np.float32), ("act", self.act_pad, self.m, np.float32),
                ("rew", self.rew_pad, 1, np.float64)] + \
            ([("base", self.pred_pad, 1, np.float64)] if self.pred_pad is not None else [])
        out = {}
        idx = None
        if T == N * H:
            # every trajectory ran the full horizon: the padded slabs are the batch
            for name, pad, k, _ in pads:
                out[name] = pad[:T] if k == 1 else pad.view(-1)[:T * k].view(T, k)
        else:
            # compact: row i of the batch is row ep H + (i - off[ep]) of the slabs, one
            # device gather per slot
            start = torch.from_numpy(np.arange(N, dtype=np.int64) * H - offs[:-1]).to(dev)
            idx = torch.arange(T, dtype=torch.int64, device=dev) + torch.repeat_interleave(
                start, torch.from_numpy(lengths).to(dev), output_size=T)
            K = _lib.calls()
            st = _lib.stream_ptr()
            for name, pad, k, dt in pads:
                dst = _STAGING.device_slot(name, T * k, dt, dev) if reuse else \
                    torch.empty(T * k, dtype=torch.float32 if dt == np.float32 else torch.float64, device=dev)
                if T:
                    K.mjrl_gather_rows(pad, k * np.dtype(dt).itemsize, idx, T, dst, st)
                out[name] = dst.view(T, k) if k > 1 else dst
        obs, act, rew = out["obs"], out["act"], out["rew"]
        value_feat = None
        if self.pred_pad is not None:
            base = out["base"]
        elif self.value_features:
            # MLPBaseline: the matrix its network reads, [T][n + 4], in one pass over
            # the feature slab (compaction by the gather's own index, the time columns
            # from the baseline's table), then one forward
            k = self.n + 4
            value_feat = (_STAGING.device_slot("value_feat", T * k, np.float32, dev) if reuse else
                          torch.empty(T * k, dtype=torch.float32, device=dev)).view(T, k)
            if self._vf_ev is not None:
                cur.wait_event(self._vf_ev)   # the last lock step's features
            if T:
                _lib.calls().mjrl_value_features_finish(self.feat_pad, idx, T, self.n, N * H, H,
                                                        self.baseline.time_table(H, dev), value_feat,
                                                        _lib.stream_ptr())
            base = self.baseline.predict_features_device(value_feat)
        elif not self.linear and self.baseline is not None:
            # another baseline: its own predict per path, as DeviceBatch.from_paths
            # (process_samples.py:23)
            base = stage("base", [self.baseline.predict(p) for p in paths], 0)
        else:
            base = _STAGING.device_slot("base", T, np.float64, dev) if reuse else \
                torch.empty(T, dtype=torch.float64, device=dev)
            base.zero_()
        b = DeviceBatch(obs, act, rew, base, off, term, obs_range=orange)
        b.lengths = lengths
        b.obs_inexact = bool(self.flag[0])
        if value_feat is not None:
            b.value_feat = value_feat   # kept for the baseline fit (MLPBaseline.fit_features_device)
        self.done = True
        return b


class _Record:
    """What the sink keeps of a finished trajectory until it is accepted."""
    __slots__ = ("length", "term", "chunks", "lo", "hi", "flag")


class ChunkSink(StreamSink):
    """The sink of sample_mode="samples": N is a number of timesteps, the number of
    trajectories is not known while they are sampled, and some of the rows handed
    in belong to trajectories that are not part of the batch.

    The pinned side is StreamSink's (per-slot slabs [S][2][H], the same native row
    call and prediction per row).  The device side is a pool of C chunks of CH =
    min(FLUSH_ROWS, H) rows for the observations, actions, rewards and predictions
    (and the value features): a trajectory takes its next chunk when its row t
    with t % CH == 0 arrives (from the chunks abandoned trajectories gave back,
    else the next unused one), so every flush and every feature row of the lock
    step has its place, and a flush is split at chunk boundaries.  The column
    ranges and the exactness flag are kept per live trajectory
    (mjrl_host_stage_rows_slots_f64x) and folded into the batch's in trajectory
    order, each as soon as the trajectories before it have ended with fewer than
    N rows (it is then part of the batch whatever follows); abandon(slot) drops a
    live trajectory's and returns its chunks.

    rows_cap: the pool's rows (rounded up to whole chunks); by default
    2 (N + S H): the batch has fewer than N + H rows, the trajectories started
    beyond it fewer than S H, and every trajectory wastes less than CH rows of its
    last chunk, which this covers while P CH <= N + S H.  When no chunk is left
    the sink sets `overflowed`, stops sending and raises nothing; batch() then
    refuses and the caller stages the paths with DeviceBatch.from_paths (the same
    bits).

    batch(paths) takes exactly the prefix the sampler returned, builds a run
    table {pool row, batch row, rows, first time index} of one run per chunk and
    compacts the pools with mjrl_copy_runs (mjrl_value_features_finish_runs for
    the value-feature matrix): no per-row index."""

    ROWS_CAP = None   # the pool's rows when the constructor is given none (None: the default budget)

    def __init__(self, n, m, horizon, N, device, baseline=None, nslots=64, value_features=False, rows_cap=None):
        self.n, self.m, self.H, self.N = int(n), int(m), int(horizon), int(N)
        self.device = torch.device(device)
        self.baseline = baseline
        self.value_features = bool(value_features)
        if self.value_features and not hasattr(baseline, "predict_features_device"):
            raise ValueError("ChunkSink(value_features=True) needs a baseline with predict_features_device "
                             "(MLPBaseline), got %r" % (baseline,))
        c = _linear_coeffs(baseline, self.n)
        self.linear = c is not False
        self.coeffs = None if c is False or c is None else np.ascontiguousarray(c, dtype=np.float64)
        self.S = _lib.stage_calls()
        S, B, H = int(nslots), self.NBUF, self.H
        key = (S, B, H, self.n, self.m)
        ent = _SLABS.get(key)
        if ent is None:
            _SLABS.clear()   # one shape at a time
            pin = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, pin_memory=True)   # noqa: E731
            ent = _SLABS[key] = dict(obs=pin(S, B, H, self.n), act=pin(S, B, H, self.m),
                                     rew=pin(S, B, H, dt=torch.float64), pred=pin(S, B, H, dt=torch.float64),
                                     ev=[[None] * B for _ in range(S)])
        self._obs, self._act, self._rew, self._pred, self._ev = (ent[k] for k in ("obs", "act", "rew", "pred", "ev"))
        self.obs_h, self.act_h, self.rew_h, self.pred_h = (t.numpy() for t in (self._obs, self._act, self._rew,
                                                                               self._pred))
        self._row_ptr0 = self.obs_h.ctypes.data
        self.buf = np.zeros(S, np.int64)
        self.ep = np.full(S, -1, np.int64)
        self.copied = np.zeros(S, np.int64)
        # per live trajectory (by slot): its column ranges, its exactness flag, its chunks
        self.slot_lo = np.full((S, self.n), np.inf, np.float32)
        self.slot_hi = np.full((S, self.n), -np.inf, np.float32)
        self.slot_flag = np.zeros(S, np.int32)
        self.slot_chunks = [[] for _ in range(S)]
        # the batch's: folded from the accepted trajectories, in their order
        self.lo = np.full(self.n, np.inf, np.float32)
        self.hi = np.full(self.n, -np.inf, np.float32)
        self.flag = np.zeros(1, np.int32)
        self.pending = {}     # finished trajectories not accepted (yet), by index
        self.accepted = []    # records of trajectories 0 .. len(accepted) - 1
        self.prefix_rows = 0
        self.CH = CH = max(1, min(int(self.FLUSH_ROWS), H))
        if rows_cap is None:
            rows_cap = self.ROWS_CAP
        cap = 2 * (self.N + S * H) if rows_cap is None else int(rows_cap)
        self.C = C_ = max(1, -(-cap // CH))
        self.pool_rows = R = C_ * CH
        self.next_chunk, self.free_chunks = 0, []
        self.overflowed = False
        with torch.cuda.device(self.device):
            slot = lambda name, k, dt: _STAGING.device_slot(name, R * k, dt, self.device)   # noqa: E731
            self.obs_pad = slot("chunk_obs", self.n, np.float32).view(R, self.n)
            self.act_pad = slot("chunk_act", self.m, np.float32).view(R, self.m)
            self.rew_pad = slot("chunk_rew", 1, np.float64)
            self.pred_pad = slot("chunk_pred", 1, np.float64) if self.coeffs is not None else None
            self.cs = _STAGING._copy_stream(self.device)
            # the pools may still be read by work queued on the current stream
            self.cs.wait_stream(torch.cuda.current_stream(self.device))
            if self.value_features:
                self._init_value_features(S)
        self.done = False

    def _init_value_features(self, S):
        """feat_pad [C CH][n] f32 in HBM, the feature pool: the row of chunk c at
        offset t % CH is float32(clip(x) / 10) of the f64 observation, written by
        mjrl_value_features_slots in the lock step that produced it.  The per-step
        buffers are StreamSink's."""
        n, dev = self.n, self.device
        self.feat_pad = _STAGING.device_slot("chunk_vfeat", self.pool_rows * n, np.float32, dev).view(
            self.pool_rows, n)
        key = (S, n, dev)
        ent = _VF_BUFS.get(key)
        if ent is None:
            _VF_BUFS.clear()
            R = self.VF_RING
            ent = _VF_BUFS[key] = dict(h_idx=torch.zeros((R, 2, S), dtype=torch.int64).pin_memory(),
                                       d_idx=torch.zeros((2, S), dtype=torch.int64, device=dev),
                                       h_rows=None, d_rows=None, ev=[None] * R, turn=0)
        self._vf = ent
        self._board = None
        self._vf_ev = None

    def _feature_rows(self, slots, obs, dest):
        """StreamSink._feature_rows with the rows' places in the pool given."""
        vf, E, S = self._vf, len(slots), len(self.buf)
        r = vf["turn"]
        vf["turn"] = (r + 1) % self.VF_RING
        if vf["ev"][r] is not None:
            vf["ev"][r].synchronize()   # the copies that last read the pinned buffers of this turn
        h_idx, d_idx = vf["h_idx"][r], vf["d_idx"]
        h = h_idx.numpy()
        h[0, :E] = dest
        live = h[1].view(np.int32)
        with torch.cuda.device(self.device):
            if self._board is not None:
                live[:E] = slots
                src, nsrc = self._board, int(self._board.shape[0])
            else:
                if vf["h_rows"] is None:
                    vf["h_rows"] = torch.zeros((self.VF_RING, S, self.n), dtype=torch.float64).pin_memory()
                    vf["d_rows"] = torch.zeros((S, self.n), dtype=torch.float64, device=self.device)
                vf["h_rows"][r].numpy()[:E] = obs
                vf["d_rows"][:E].copy_(vf["h_rows"][r, :E], non_blocking=True)
                live[:E] = np.arange(E, dtype=np.int32)
                src, nsrc = vf["d_rows"], S
            d_idx.copy_(h_idx, non_blocking=True)
            _lib.calls().mjrl_value_features_slots(src, d_idx[1], d_idx[0], E, nsrc, self.n, self.pool_rows,
                                                   self.feat_pad, _lib.stream_ptr())
            ev = vf["ev"][r]
            if ev is None:
                ev = vf["ev"][r] = torch.cuda.Event()
            ev.record()
        self._vf_ev = ev

    # ---- sampler side -------------------------------------------------------
    def begin(self, slot, ep):
        StreamSink.begin(self, slot, ep)
        self.slot_lo[slot] = np.inf
        self.slot_hi[slot] = -np.inf
        self.slot_flag[slot] = 0
        self.slot_chunks[slot] = []

    def _take_chunk(self, slot):
        if self.free_chunks:
            c = self.free_chunks.pop()
        elif self.next_chunk < self.C:
            c = self.next_chunk
            self.next_chunk += 1
        else:
            self.overflowed = True
            return False
        self.slot_chunks[slot].append(c)
        return True

    def rows(self, slots, obs, t):
        if self.overflowed:
            return
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        t = np.ascontiguousarray(t, dtype=np.int64)
        E = len(slots)
        if E == 0:
            return
        for i in np.nonzero(t % self.CH == 0)[0].tolist():
            if not self._take_chunk(int(slots[i])):
                return
        b = self.buf[slots]
        stride_b, stride_s = self.H * self.n * 4, self.NBUF * self.H * self.n * 4
        ptrs = (C.c_void_p * E)(*(self._row_ptr0 + slots * stride_s + b * stride_b + t * self.n * 4).tolist())
        pred = np.empty(E, np.float64) if self.coeffs is not None else None
        self.S.mjrl_host_stage_rows_slots_f64x(obs, E, self.n, ptrs, slots, len(self.buf), self.slot_lo,
                                               self.slot_hi, None if pred is None else self.coeffs, t, pred,
                                               self.slot_flag)
        if pred is not None:
            self.pred_h[slots, b, t] = pred
        if self.value_features:
            chunk = np.array([self.slot_chunks[s][-1] for s in slots.tolist()], np.int64)
            self._feature_rows(slots, obs, chunk * self.CH + t % self.CH)
        due = np.nonzero(t - self.copied[slots] >= self.FLUSH_ROWS)[0]
        for i in due.tolist():
            self._send(int(slots[i]), int(t[i]))

    def _send(self, slot, upto):
        """Rows [copied, upto) of slot `slot`'s live trajectory to their chunks, piece
        by piece between chunk boundaries, on the copy stream."""
        b, a = int(self.buf[slot]), int(self.copied[slot])
        if upto <= a or self.overflowed:
            return
        CH, chunks = self.CH, self.slot_chunks[slot]
        with torch.cuda.stream(self.cs):
            while a < upto:
                e = min(upto, (a // CH + 1) * CH)
                d0 = chunks[a // CH] * CH + a % CH
                d1 = d0 + (e - a)
                self.obs_pad[d0:d1].copy_(self._obs[slot, b, a:e], non_blocking=True)
                self.act_pad[d0:d1].copy_(self._act[slot, b, a:e], non_blocking=True)
                self.rew_pad[d0:d1].copy_(self._rew[slot, b, a:e], non_blocking=True)
                if self.pred_pad is not None:
                    self.pred_pad[d0:d1].copy_(self._pred[slot, b, a:e], non_blocking=True)
                a = e
        self.copied[slot] = upto

    def finish(self, slot, length, terminated=False):
        """Slot `slot`'s trajectory ended after `length` rows: its rows not sent yet
        leave for HBM, and it is accepted once the trajectories before it are."""
        ep, Lr = int(self.ep[slot]), int(length)
        self.ep[slot] = -1
        self._send(slot, Lr)
        self._guard(slot)
        if self.overflowed:
            return
        rec = _Record()
        rec.length, rec.term, rec.chunks = Lr, bool(terminated), self.slot_chunks[slot]
        rec.lo, rec.hi, rec.flag = self.slot_lo[slot].copy(), self.slot_hi[slot].copy(), int(self.slot_flag[slot])
        self.slot_chunks[slot] = []
        self.pending[ep] = rec
        # trajectory k is part of the batch when 0 .. k - 1 have ended with < N rows
        while self.prefix_rows < self.N and len(self.accepted) in self.pending:
            rec = self.pending.pop(len(self.accepted))
            lo, hi = self.lo, self.hi
            np.copyto(lo, rec.lo, where=rec.lo < lo)   # v < lo ? v : lo, as the native fold
            np.copyto(hi, rec.hi, where=rec.hi > hi)
            self.flag[0] |= rec.flag
            self.accepted.append(rec)
            self.prefix_rows += rec.length

    def _guard(self, slot):
        """The event behind the copies out of the slot's current slab, which begin()
        waits for before the slab is written again."""
        if self.copied[slot]:
            ev = torch.cuda.Event()   # covers the trajectory's earlier runs too (one stream, in order)
            ev.record(self.cs)
            self._ev[slot][int(self.buf[slot])] = ev

    def abandon(self, slot):
        """Slot `slot`'s live trajectory is not part of the batch: its ranges and
        flag are dropped, its chunks go back to the pool (copies into them that
        are still queued run before any later one, on the same stream)."""
        self._guard(slot)
        self.free_chunks.extend(self.slot_chunks[slot])
        self.slot_chunks[slot] = []
        self.ep[slot] = -1

    # ---- update side -------------------------------------------------------
    def _batch(self, paths, reuse):
        if self.overflowed:
            raise RuntimeError("ChunkSink.batch: the pool of %d chunks x %d rows overflowed while sampling; stage "
                               "the paths with DeviceBatch.from_paths" % (self.C, self.CH))
        dev, CH = self.device, self.CH
        lengths = np.array([len(p["rewards"]) for p in paths], dtype=np.int64)
        if len(paths) != len(self.accepted) or not np.array_equal(lengths, [r.length for r in self.accepted]):
            raise ValueError("ChunkSink.batch: the paths are not the prefix the sink accepted")
        P, T = len(paths), int(lengths.sum())
        cur = torch.cuda.current_stream(dev)
        cur.wait_stream(self.cs)   # every trajectory's copy

        def stage(slot, arrs, ncols, dtype=np.float64):
            return _STAGING.stage(slot, arrs, ncols, dtype, dev, reuse)

        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        off = stage("off", [offs], 0, np.int64)
        term = stage("term", [np.array([r.term for r in self.accepted], dtype=np.uint8)], 0, np.uint8)
        orange = stage("orange", [np.stack([self.lo, self.hi])], self.n, np.float32)
        # the run table: chunk j of path p holds its rows [j CH, min(L, (j + 1) CH))
        nch = -(-lengths // CH)
        R = int(nch.sum())
        runs = np.zeros((R, 4), np.int64)
        if R:
            owner = np.repeat(np.arange(P), nch)
            j = np.arange(R) - np.repeat(np.cumsum(nch) - nch, nch)
            runs[:, 0] = np.concatenate([r.chunks for r in self.accepted]).astype(np.int64) * CH
            runs[:, 1] = offs[owner] + j * CH
            runs[:, 2] = np.minimum(CH, lengths[owner] - j * CH)
            runs[:, 3] = j * CH
        d_runs = torch.from_numpy(runs).to(dev)
        K, st = _lib.calls(), _lib.stream_ptr()
        pools = [("obs", self.obs_pad, self.n, np.float32), ("act", self.act_pad, self.m, np.float32),
                 ("rew", self.rew_pad, 1, np.float64)] + \
            ([("base", self.pred_pad, 1, np.float64)] if self.pred_pad is not None else [])
        out = {}
        for name, pool, k, dt in pools:
            dst = _STAGING.device_slot(name, T * k, dt, dev) if reuse else \
                torch.empty(T * k, dtype=torch.float32 if dt == np.float32 else torch.float64, device=dev)
            K.mjrl_copy_runs(pool, k * np.dtype(dt).itemsize, d_runs, R, self.pool_rows, T, dst, st)
            out[name] = dst.view(T, k) if k > 1 else dst
        obs, act, rew = out["obs"], out["act"], out["rew"]
        value_feat = None
        if self.pred_pad is not None:
            base = out["base"]
        elif self.value_features:
            k = self.n + 4
            value_feat = (_STAGING.device_slot("value_feat", T * k, np.float32, dev) if reuse else
                          torch.empty(T * k, dtype=torch.float32, device=dev)).view(T, k)
            if self._vf_ev is not None:
                cur.wait_event(self._vf_ev)   # the last lock step's features
            K.mjrl_value_features_finish_runs(self.feat_pad, d_runs, R, self.n, self.pool_rows, T, self.H,
                                              self.baseline.time_table(self.H, dev), value_feat, st)
            base = self.baseline.predict_features_device(value_feat)
        elif not self.linear and self.baseline is not None:
            base = stage("base", [self.baseline.predict(p) for p in paths], 0)
        else:
            base = _STAGING.device_slot("base", T, np.float64, dev) if reuse else \
                torch.empty(T, dtype=torch.float64, device=dev)
            base.zero_()
        b = DeviceBatch(obs, act, rew, base, off, term, obs_range=orange)
        b.lengths = lengths
        b.obs_inexact = bool(self.flag[0])
        if value_feat is not None:
            b.value_feat = value_feat
        self.done = True
        return b
