// ingest.hip — device-resident step-major rollouts cut into the path-major batch
// every other kernel reads (DeviceBatch.from_rollout).
//
// A batched simulator leaves its samples step-major: obs [H][E][n], act [H][E][m],
// rew [H][E], done [H][E], environments that reset themselves.  The reference's
// samplers hand over a list of paths (mjrl/samplers/base_sampler.py:76-83) which
// npg_cg.py:87-89 concatenates path after path.  Here the same batch is formed
// where the samples already are.
//
// The one definition of the cut (restated in NumPy as
// samplers/rollout_ingest.py:segment_rollout_reference):
//   env e has steps[e] valid steps (H when steps is null); a cell (t, e) with
//   t >= steps[e] is never read.  Env e's valid steps are cut after every cell with
//   done != 0; such a path's flag is terminated[t][e] != 0 (1 when terminated is
//   null).  A non-empty remainder is a last path with flag 0.  Paths are ordered
//   env-ascending, then time-ascending, so the row of cell (t, e) is R[e] + t, R the
//   exclusive prefix sum of steps.
//
// The carry (mjrl_rollout_segments_carry): c[e] >= 0 steps env e's running episode had
// taken before cell (0, e).  path_t0[p] = c[e] for env e's path that starts at t = 0,
// else 0: the time origin of the baselines' time features.  env_path[e] is env e's
// first path (env_path[E] = P).  c_next[e], the carry of the next call: c[e] for an
// env with no steps, 0 when its last valid cell is done, else the length of its last
// path (plus c[e] when that path starts at t = 0).  The extra values ride in the same
// three launches.
//
// mjrl_rollout_segments: latency-bound and tiny (three launches: count, scan, write).
// mjrl_rollout_pack: HBM-bound, one wave per destination row.  No atomics anywhere:
// the prefix sums and the column ranges are reduced in one fixed order.
#include "common.h"

using namespace mjrl;

namespace {

constexpr int SEG_THREADS = 256;
constexpr int PACK_MAX_WG = 2048;   // grid-stride past this many workgroups (4 rows in flight each)

__device__ __forceinline__ int64_t valid_steps(const int64_t* __restrict__ steps, int64_t e, int64_t H) {
    if (!steps) return H;
    const int64_t s = steps[e];
    return s < 0 ? 0 : (s > H ? H : s);   // device data: clamped before it bounds a walk
}

// SEG_UNROLL steps of env e's done column from t0 on, the loads issued together (a
// walk that waits for each byte before it asks for the next is one memory latency per
// step); a step at or past s is not read and counts as 0.
constexpr int SEG_UNROLL = 16;
__device__ __forceinline__ void load_done(const uint8_t* __restrict__ done, int64_t t0, int64_t s, int64_t E,
                                          int64_t e, uint8_t (&d)[SEG_UNROLL]) {
#pragma unroll
    for (int j = 0; j < SEG_UNROLL; ++j) {   // t0 < s: step s - 1 is valid, so every load is unconditional
        const int64_t t = t0 + j < s ? t0 + j : s - 1;
        d[j] = done[t * E + e];
    }
#pragma unroll
    for (int j = 0; j < SEG_UNROLL; ++j)
        if (t0 + j >= s) d[j] = 0;
}

// Phase 1.  One lane per env walks its column (lanes of a wave read adjacent e at the
// same t) and counts its paths; its valid rows are its clamped step count.
__global__ void __launch_bounds__(SEG_THREADS) k_seg_count(const uint8_t* __restrict__ done,
                                                           const int64_t* __restrict__ steps, int64_t H, int64_t E,
                                                           int64_t* __restrict__ npaths, int64_t* __restrict__ nrows) {
    const int64_t e = (int64_t)blockIdx.x * SEG_THREADS + threadIdx.x;
    if (e >= E) return;
    const int64_t s = valid_steps(steps, e, H);
    int64_t p = 0, start = 0;
    for (int64_t t0 = 0; t0 < s; t0 += SEG_UNROLL) {
        uint8_t d[SEG_UNROLL];
        load_done(done, t0, s, E, e, d);
#pragma unroll
        for (int j = 0; j < SEG_UNROLL; ++j)
            if (d[j]) {
                ++p;
                start = t0 + j + 1;
            }
    }
    npaths[e] = p + (start < s ? 1 : 0);
    nrows[e] = s;
}

// Phase 2.  One workgroup: exclusive prefix sums of both counts over E, chunk after
// chunk of SEG_THREADS envs with the running totals carried (integer sums: exact in
// any order, taken in one).  Also the table's last entry path_off[P] = T and counts.
__global__ void __launch_bounds__(SEG_THREADS) k_seg_scan(const int64_t* __restrict__ npaths,
                                                          const int64_t* __restrict__ nrows, int64_t E,
                                                          int64_t path_cap, int64_t* __restrict__ path_base,
                                                          int64_t* __restrict__ env_row, int64_t* __restrict__ path_off,
                                                          int64_t* __restrict__ counts,
                                                          int64_t* __restrict__ env_path) {
    __shared__ int64_t sp[SEG_THREADS], sr[SEG_THREADS];
    const int tid = threadIdx.x;
    int64_t cp = 0, cr = 0;   // totals of the chunks before this one (the same in every thread)
    for (int64_t e0 = 0; e0 < E; e0 += SEG_THREADS) {
        const int64_t e = e0 + tid;
        const int64_t vp = e < E ? npaths[e] : 0, vr = e < E ? nrows[e] : 0;
        sp[tid] = vp;
        sr[tid] = vr;
        __syncthreads();
        for (int d = 1; d < SEG_THREADS; d <<= 1) {   // inclusive scan of the chunk
            const int64_t ap = tid >= d ? sp[tid - d] : 0, ar = tid >= d ? sr[tid - d] : 0;
            __syncthreads();
            sp[tid] += ap;
            sr[tid] += ar;
            __syncthreads();
        }
        if (e < E) {
            path_base[e] = cp + sp[tid] - vp;
            env_row[e] = cr + sr[tid] - vr;
            if (env_path) env_path[e] = cp + sp[tid] - vp;
        }
        cp += sp[SEG_THREADS - 1];
        cr += sr[SEG_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) {
        env_row[E] = cr;
        counts[0] = cp;
        counts[1] = cr;
        if (cp <= path_cap) path_off[cp] = cr;
        if (env_path) env_path[E] = cp;
    }
}

// Phase 3.  One lane per env walks again and writes its paths' first rows and flags
// from its base; nothing at or beyond path_cap is written.  With a carry: the time
// origin of each path (path_t0, nullable) and the env's next carry (carry_out,
// nullable).  carry_out may be carry_in: the lane reads its entry before it writes it,
// and no other lane touches it (neither pointer is __restrict__).
__global__ void __launch_bounds__(SEG_THREADS) k_seg_write(const uint8_t* __restrict__ done,
                                                           const uint8_t* __restrict__ terminated,
                                                           const int64_t* __restrict__ steps, int64_t H, int64_t E,
                                                           int64_t path_cap, const int64_t* __restrict__ path_base,
                                                           const int64_t* __restrict__ env_row,
                                                           int64_t* __restrict__ path_off,
                                                           uint8_t* __restrict__ path_term,
                                                           const int64_t* carry_in, int64_t* __restrict__ path_t0,
                                                           int64_t* carry_out) {
    const int64_t e = (int64_t)blockIdx.x * SEG_THREADS + threadIdx.x;
    if (e >= E) return;
    const int64_t s = valid_steps(steps, e, H);
    const int64_t r0 = env_row[e];
    int64_t c = carry_in ? carry_in[e] : 0;
    c = c < 0 ? 0 : c;   // device data: clamped as the steps are
    int64_t p = path_base[e], start = 0;
    for (int64_t t0 = 0; t0 < s; t0 += SEG_UNROLL) {
        uint8_t d[SEG_UNROLL];
        load_done(done, t0, s, E, e, d);
#pragma unroll
        for (int j = 0; j < SEG_UNROLL; ++j)
            if (d[j]) {
                const int64_t t = t0 + j;
                if (p >= 0 && p < path_cap) {
                    path_off[p] = r0 + start;
                    path_term[p] = terminated ? (uint8_t)(terminated[t * E + e] != 0) : (uint8_t)1;
                    if (path_t0) path_t0[p] = start == 0 ? c : 0;
                }
                ++p;
                start = t + 1;
            }
    }
    if (start < s && p >= 0 && p < path_cap) {
        path_off[p] = r0 + start;
        path_term[p] = 0;
        if (path_t0) path_t0[p] = start == 0 ? c : 0;
    }
    // start is now the first step of the env's last path, or s when its last cell is done
    if (carry_out) carry_out[e] = s == 0 ? c : (start >= s ? 0 : (s - start) + (start == 0 ? c : 0));
}

// ---- the transposing pack ----

template <typename V> struct Lanes;
template <> struct Lanes<float> { static constexpr int W = 1; };
template <> struct Lanes<float2> { static constexpr int W = 2; };
template <> struct Lanes<float4> { static constexpr int W = 4; };

__device__ __forceinline__ float at(const float& v, int) { return v; }
__device__ __forceinline__ float at(const float2& v, int j) { return j ? v.y : v.x; }
__device__ __forceinline__ float at(const float4& v, int j) { return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w)); }
__device__ __forceinline__ void put(float& v, int, float x) { v = x; }
__device__ __forceinline__ void put(float2& v, int j, float x) { (j ? v.y : v.x) = x; }
__device__ __forceinline__ void put(float4& v, int j, float x) { (j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w))) = x; }

// the host staging pass's fold (csrc/stage.cpp): a NaN compares false and is skipped
__device__ __forceinline__ float fold_min(float v, float lo) { return v < lo ? v : lo; }
__device__ __forceinline__ float fold_max(float v, float hi) { return v > hi ? v : hi; }

template <typename V>
__device__ __forceinline__ void copy_words(const void* __restrict__ s, void* __restrict__ d, int nw, int lane) {
    const V* __restrict__ sv = (const V*)s;
    V* __restrict__ dv = (V*)d;
    for (int c = lane; c < nw; c += 64) dv[c] = sv[c];
}

// Destination row r of the path-major batch is cell (t, e) with R[e] <= r < R[e + 1],
// t = r - R[e] (steps null: every env has H rows, e = r / H).  One wave per row per
// grid stride in x; blockIdx.y is the block of 64 words of the observation row the
// wave moves, and the waves of block 0 also move the row's actions and reward.
// obs / act rows move as words of V / of act_wb bytes (bit copies: f32 and f64
// alike).  RANGE (f32 observations): every lane folds the words it moves into its
// columns' (min, max); the workgroup's four waves are folded in wave order into
// part [gridDim.x][2][n].  A row whose cell falls outside [0, H) x [0, E) is skipped.
template <typename V, bool RANGE>
__global__ void __launch_bounds__(256) k_rollout_pack(const V* __restrict__ obs, const char* __restrict__ act,
                                                      const void* __restrict__ rew, int rew_f64,
                                                      const int64_t* __restrict__ steps,
                                                      const int64_t* __restrict__ env_row, int64_t H, int64_t E,
                                                      int nv, int act_bytes, int act_wb, int64_t T,
                                                      V* __restrict__ obs_out, char* __restrict__ act_out,
                                                      double* __restrict__ rew_out, float* __restrict__ part) {
    constexpr int W = Lanes<V>::W;
    __shared__ V slo[RANGE ? 256 : 1], shi[RANGE ? 256 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;   // this lane's word of the observation row
    const bool first = blockIdx.y == 0;
    V lo, hi;
    if (RANGE)
        for (int j = 0; j < W; ++j) {
            put(lo, j, INFINITY);
            put(hi, j, -INFINITY);
        }
    const int64_t nwv = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < T; r += nwv) {
        int64_t e, t;
        if (steps) {
            int64_t a = 0, b = E;   // the last e in [0, E) with R[e] <= r (R is non-decreasing)
            while (b - a > 1) {
                const int64_t mid = (a + b) >> 1;
                if (env_row[mid] <= r) a = mid; else b = mid;
            }
            e = a;
            t = r - env_row[e];
            if (t < 0 || t >= valid_steps(steps, e, H)) continue;
        } else {
            e = r / H;
            t = r - e * H;
            if (e >= E) continue;
        }
        const int64_t cell = t * E + e;
        if (c < nv) {
            const V v = obs[cell * nv + c];
            obs_out[r * nv + c] = v;
            if (RANGE)
                for (int j = 0; j < W; ++j) {
                    put(lo, j, fold_min(at(v, j), at(lo, j)));
                    put(hi, j, fold_max(at(v, j), at(hi, j)));
                }
        }
        if (first) {
            const char* __restrict__ as = act + cell * act_bytes;
            char* __restrict__ ad = act_out + r * act_bytes;
            if (act_wb == 16) copy_words<float4>(as, ad, act_bytes / 16, lane);
            else if (act_wb == 8) copy_words<float2>(as, ad, act_bytes / 8, lane);
            else copy_words<float>(as, ad, act_bytes / 4, lane);
            if (lane == 0) rew_out[r] = rew_f64 ? ((const double*)rew)[cell] : (double)((const float*)rew)[cell];
        }
    }
    if (RANGE) {
        slo[threadIdx.x] = lo;
        shi[threadIdx.x] = hi;
        __syncthreads();
        if (wave == 0 && c < nv) {
            for (int w = 1; w < 4; ++w) {
                const V l = slo[w * 64 + lane], h = shi[w * 64 + lane];
                for (int j = 0; j < W; ++j) {
                    put(lo, j, fold_min(at(l, j), at(lo, j)));
                    put(hi, j, fold_max(at(h, j), at(hi, j)));
                }
            }
            V* __restrict__ p = (V*)(part + (int64_t)blockIdx.x * 2 * nv * W);
            p[c] = lo;
            p[nv + c] = hi;
        }
    }
}

// out [2][n] from part [G][2][n]: one wave per column, lane l folds the workgroups
// l, l + 64, ... in order, then the lanes are folded by a fixed butterfly.
__global__ void __launch_bounds__(256) k_range_reduce(const float* __restrict__ part, int G, int n,
                                                      float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= n) return;
    float lo = INFINITY, hi = -INFINITY;
    for (int g = lane; g < G; g += 64) {
        lo = fold_min(part[((int64_t)g * 2) * n + col], lo);
        hi = fold_max(part[((int64_t)g * 2 + 1) * n + col], hi);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fold_min(__shfl_xor(lo, d, 64), lo);
        hi = fold_max(__shfl_xor(hi, d, 64), hi);
    }
    if (lane == 0) {
        out[col] = lo;
        out[n + col] = hi;
    }
}

int pack_grid(int64_t T) {
    const int64_t g = (T + 3) / 4;
    return (int)(g < 1 ? 1 : (g > PACK_MAX_WG ? PACK_MAX_WG : g));
}

// widest word (16 / 8 / 4 bytes) that divides a row of `bytes` and every address in `a`
int word_bytes(int64_t bytes, uintptr_t a) {
    if (bytes % 16 == 0 && a % 16 == 0) return 16;
    if (bytes % 8 == 0 && a % 8 == 0) return 8;
    return 4;
}

template <typename V>
void launch_pack(bool range, dim3 g, hipStream_t st, const void* obs, const void* act, const void* rew, int rew_f64,
                 const int64_t* steps, const int64_t* env_row, int64_t H, int64_t E, int nv, int act_bytes, int act_wb,
                 int64_t T, void* obs_out, void* act_out, double* rew_out, float* part) {
    if (range)
        hipLaunchKernelGGL((k_rollout_pack<V, true>), g, dim3(256), 0, st, (const V*)obs, (const char*)act, rew, rew_f64,
                           steps, env_row, H, E, nv, act_bytes, act_wb, T, (V*)obs_out, (char*)act_out, rew_out, part);
    else
        hipLaunchKernelGGL((k_rollout_pack<V, false>), g, dim3(256), 0, st, (const V*)obs, (const char*)act, rew,
                           rew_f64, steps, env_row, H, E, nv, act_bytes, act_wb, T, (V*)obs_out, (char*)act_out,
                           rew_out, part);
}

}  // namespace

extern "C" {

int mjrl_rollout_segments_scratch(int64_t E, int64_t* words) {
    if (E < 0 || !words) return MJRL_EINVAL;
    *words = 3 * E;   // paths per env, rows per env, first path of each env
    return MJRL_OK;
}

int mjrl_rollout_segments_carry(const uint8_t* done, const uint8_t* terminated, const int64_t* steps, int64_t H,
                                int64_t E, int64_t path_cap, const int64_t* episode_steps_in, int64_t* env_row,
                                int64_t* path_off, uint8_t* path_term, int64_t* path_t0, int64_t* env_path,
                                int64_t* episode_steps_out, int64_t* counts, int64_t* scratch, void* stream) {
    if (H < 0 || E < 0 || path_cap < 0 || !env_row || !path_off || !counts) return MJRL_EINVAL;
    if (E > 0 && (!scratch || (H > 0 && !done))) return MJRL_EINVAL;
    if (path_cap > 0 && !path_term) return MJRL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int64_t* npaths = scratch;
    int64_t* nrows = scratch + E;
    int64_t* path_base = scratch + 2 * E;
    const unsigned g = (unsigned)((E + SEG_THREADS - 1) / SEG_THREADS);
    if (g) hipLaunchKernelGGL(k_seg_count, dim3(g), dim3(SEG_THREADS), 0, st, done, steps, H, E, npaths, nrows);
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(SEG_THREADS), 0, st, npaths, nrows, E, path_cap, path_base, env_row,
                       path_off, counts, env_path);
    if (g)
        hipLaunchKernelGGL(k_seg_write, dim3(g), dim3(SEG_THREADS), 0, st, done, terminated, steps, H, E, path_cap,
                           path_base, env_row, path_off, path_term, episode_steps_in, path_t0, episode_steps_out);
    return (int)hipGetLastError();
}

int mjrl_rollout_segments(const uint8_t* done, const uint8_t* terminated, const int64_t* steps, int64_t H, int64_t E,
                          int64_t path_cap, int64_t* env_row, int64_t* path_off, uint8_t* path_term, int64_t* counts,
                          int64_t* scratch, void* stream) {
    return mjrl_rollout_segments_carry(done, terminated, steps, H, E, path_cap, nullptr, env_row, path_off, path_term,
                                       nullptr, nullptr, nullptr, counts, scratch, stream);
}

int mjrl_rollout_pack_scratch(int64_t T, int32_t n, int64_t* floats) {
    if (T < 0 || n <= 0 || !floats) return MJRL_EINVAL;
    *floats = (int64_t)pack_grid(T) * 2 * n;
    return MJRL_OK;
}

int mjrl_rollout_pack(const void* obs, const void* act, const void* rew, int32_t obs_f64, int32_t rew_f64,
                      const int64_t* steps, const int64_t* env_row, int64_t H, int64_t E, int32_t n, int32_t m,
                      int64_t T, void* obs_out, void* act_out, double* rew_out, float* obs_range, float* scratch,
                      void* stream) {
    if (H < 0 || E < 0 || T < 0 || n <= 0 || m <= 0) return MJRL_EINVAL;
    if ((obs_f64 != 0 && obs_f64 != 1) || (rew_f64 != 0 && rew_f64 != 1)) return MJRL_EINVAL;
    if (T > 0 && (!obs || !act || !rew || !obs_out || !act_out || !rew_out || H == 0 || E == 0)) return MJRL_EINVAL;
    if (steps ? !env_row : T != H * E) return MJRL_EINVAL;   // without steps every cell is a row
    if (obs_range && (obs_f64 || !scratch)) return MJRL_EINVAL;   // the ranges are those of f32 rows
    hipStream_t st = (hipStream_t)stream;
    const int G = pack_grid(T);
    if (T > 0) {
        const int es = obs_f64 ? 8 : 4;
        const int64_t obs_bytes = (int64_t)n * es;
        const int act_bytes = m * es;
        const int wb = word_bytes(obs_bytes, (uintptr_t)obs | (uintptr_t)obs_out | (obs_range ? (uintptr_t)scratch : 0));
        const int act_wb = word_bytes(act_bytes, (uintptr_t)act | (uintptr_t)act_out);
        const int nv = (int)(obs_bytes / wb);
        const dim3 g((unsigned)G, (unsigned)((nv + 63) / 64));
        const bool range = obs_range != nullptr;
        if (wb == 16)
            launch_pack<float4>(range, g, st, obs, act, rew, rew_f64, steps, env_row, H, E, nv, act_bytes, act_wb, T,
                                obs_out, act_out, rew_out, scratch);
        else if (wb == 8)
            launch_pack<float2>(range, g, st, obs, act, rew, rew_f64, steps, env_row, H, E, nv, act_bytes, act_wb, T,
                                obs_out, act_out, rew_out, scratch);
        else
            launch_pack<float>(range, g, st, obs, act, rew, rew_f64, steps, env_row, H, E, nv, act_bytes, act_wb, T,
                               obs_out, act_out, rew_out, scratch);
    }
    if (obs_range)   // T == 0: no partials, the ranges stay (+inf, -inf) as the host pass leaves them
        hipLaunchKernelGGL(k_range_reduce, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, scratch, T > 0 ? G : 0,
                           (int)n, obs_range);
    return (int)hipGetLastError();
}

}  // extern "C"
