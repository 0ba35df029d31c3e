// policy_fit_wide.hip — policy_fit.hip's minibatch Adam step (phases 1-9 of its header comment)
// for hidden layers up to 256 units wide, sliced over workgroups (fit_backend = "hip_wide";
// mjrl_policy_fit_wide_epoch, mjrl_policy_mse_wide_epoch).
//
// A [64][256] f32 tile is 64 KB, so a0, a1, g0 and g1 cannot share one workgroup's LDS as they
// do in k_pfit.  The work of a step is spread over one workgroup per 16 hidden units instead,
// and EVERY dependency between workgroups is a kernel boundary: no grid barrier, no flag, no
// spin loop, no atomic, no cooperative launch, no persistent kernel.  Every launch is bounded
// work of one step.  The tiles that cross a boundary live in the scratch (row pitch 256):
// a0 of even steps, a0 of odd steps, a1, g1, the loss.
//
// Step k is three launches on one stream:
//   k_wide_l0  grid ceil(h0 / 16), workgroup u owns units 16u .. 16u + 15 of layer 0.
//       UPDATE (of step k - 1): its 16 columns of g0 = (g1 W1) o (1 - a0^2) from the previous
//       head's g1 and the W1 that step used (layer 1 is updated by the NEXT launch), then
//       dW0 = g0^T [xhat, 1] of its units over the re-gathered X tile, chunk by chunk, with Adam
//       on exactly those elements.  FORWARD: its columns of a0 = tanh(xhat W0^T + b0) for step
//       k's minibatch, from the rows of W0 it has just written.
//   k_wide_l1  grid ceil(h1 / 16), the same for layer 1: dW1 = g1^T [a0, 1] of its units with
//       the previous step's a0, Adam, then its columns of a1 = tanh(a0 W1^T + b1).
//   k_wide_head<MSE>  one workgroup: mu, z, the loss head, gmu, g1 = (gmu W2) o (1 - a1^2), the
//       step's loss, and behind a barrier dW2 / db2 / d log_std with Adam (k_pfit's phases 1,
//       4 - 7 and layer 2's part of 9, the same code).
// a0 is double-buffered: a fused k_wide_l0 launch writes step k's a0 while the launches around
// it still read step k - 1's.  An epoch is l0<F> l1<F>, then head l0<U,F> l1<U,F> per step,
// the last pair <U> alone, so a call leaves nothing behind but the loss.
//
// Arithmetic (the contract of policy_fit.hip and value_fit.hip): products on
// v_mfma_f32_16x16x4_f32, one accumulator per output tile and k in ascending order, row sums of
// the heads in f64, every sum in one fixed order, no atomic; Adam is fit.h's adam_step /
// wgrad_tail with step t's bias corrections formed on the host in f64 from t alone.  UPDATE and
// FORWARD are run-time flags of one code object, so the same state and arguments give the same
// bits however a run is split into calls.  Rows bs .. 63 and a row whose index is outside
// [0, T) are masked: nothing of obs / act / adv / ll_old is read for them, their dL/dLL is 0
// (so are their rows of gmu, g1 and g0), the mean still divides by bs.
#include "fit.h"

using namespace mjrl;

namespace {

constexpr int WR = 64;                 // padded minibatch rows
constexpr int WH = 256;                // largest hidden width
constexpr int WM = 64;                 // largest action width
constexpr int WP = WH;                 // row pitch of the tiles in the scratch
constexpr int WTILE = WR * WP;         // floats of one of them
constexpr int TLD = WH + 4;            // LDS row pitch of a [64][256] tile: rows 4 banks apart
constexpr int ZLD = WM + 4;            // of the [64][64] z / gmu tile
constexpr int XCW = 256;               // columns of the X tile held in LDS at a time (pitch TLD)
constexpr int WT = 512;                // threads of every workgroup
constexpr int WW = WT / 64;            // waves
constexpr int A1_OFF = 2 * WTILE, G1_OFF = 3 * WTILE, LOSS_OFF = 4 * WTILE;
constexpr int64_t W_SCRATCH = 4 * (int64_t)WTILE + 64;
constexpr int PF_BC = 0, PF_PPO = 1;
constexpr double HALF_LOG_2PI = 0.91893853320467274178;

struct WideArgs {
    const float *obs, *act, *adv, *ll_old, *old_ls;
    const float *in_shift, *in_scale, *out_shift, *out_scale;
    const int64_t* idx;               // the call's first minibatch
    int64_t T;
    float* p[7];                      // W0, b0, W1, b1, W2, b2, log_std (torch order)
    float* m[7];
    float* v[7];
    float* scratch;
    int64_t scap;                     // floats of scratch (debug build: checked)
    float* grad;                      // null or the [d] gradient of the step this launch writes into
    float* loss;                      // null or the head's loss slot
    int64_t kU, kF;                   // minibatch of the update half / of the forward half and the head
    int n, na, h0, h1, bs, kind;      // na: the action width m
    int update, forward;
    int vx, vw0, vw1, vw2;            // 16-byte loads of obs rows / W0 / W1 / W2 rows allowed
    float clip_lo, clip_hi;           // float(1 - c), float(1 + c)
    AdamK hp;                         // of the step whose Adam this launch runs
};

// float offset of step k's a0 in the scratch
__device__ __forceinline__ int a0_off(int64_t k) { return (k & 1) ? WTILE : 0; }

// row index of minibatch k's row r, or -1 for a masked row
__device__ __forceinline__ int64_t mb_row(const WideArgs& a, int64_t k, int r) {
    if (r >= a.bs) return -1;
    const int64_t i = a.idx[k * a.bs + r];
    return i >= 0 && i < a.T ? i : -1;
}

// the gathered, normalised X tile of chunk c for the rows s_row: 8 threads per row, zero-filled
// to a multiple of 16 columns (k_pfit's load_chunk)
__device__ __forceinline__ void stage_x(const WideArgs& a, const int64_t* s_row, float* Xs, int c, int tid) {
    const int n = a.n;
    const int c0 = c * XCW, cw = n - c0 < XCW ? (n - c0 > 0 ? n - c0 : 0) : XCW;
    const int cwp = round_up(cw, 16);
    const int xr = tid >> 3, xc = tid & 7;
    const int64_t xi = s_row[xr];
    const float* const xrow = a.obs + (xi >= 0 ? xi : 0) * n + c0;
    if (a.vx) {
        float4 xb[XCW / 32];
#pragma unroll
        for (int i = 0; i < XCW / 32; ++i) {
            const int col = 4 * (xc + 8 * i);
            xb[i] = float4{0.f, 0.f, 0.f, 0.f};
            if (xi >= 0 && col < cw) xb[i] = *reinterpret_cast<const float4*>(xrow + col);
        }
#pragma unroll
        for (int i = 0; i < XCW / 32; ++i) {
            const int col = 4 * (xc + 8 * i);
            if (col >= cwp) continue;
            float4 o = float4{0.f, 0.f, 0.f, 0.f};
            if (xi >= 0 && col < cw) {   // cw % 4 == 0 here
                const float4 sh = *reinterpret_cast<const float4*>(a.in_shift + c0 + col);
                const float4 sc = *reinterpret_cast<const float4*>(a.in_scale + c0 + col);
                o.x = (xb[i].x - sh.x) / (sc.x + 1e-8f);
                o.y = (xb[i].y - sh.y) / (sc.y + 1e-8f);
                o.z = (xb[i].z - sh.z) / (sc.z + 1e-8f);
                o.w = (xb[i].w - sh.w) / (sc.w + 1e-8f);
            }
            *reinterpret_cast<float4*>(Xs + xr * TLD + col) = o;
        }
    } else {
#pragma unroll 8
        for (int i = 0; i < XCW / 8; ++i) {
            const int col = xc + 8 * i;
            if (col >= cwp) continue;
            float o = 0.f;
            if (xi >= 0 && col < cw) o = (xrow[col] - a.in_shift[c0 + col]) / (a.in_scale[c0 + col] + 1e-8f);
            Xs[xr * TLD + col] = o;
        }
    }
}

// columns 0 .. cols - 1 (a multiple of 16) of the scratch tile at float offset off into LDS, pitch TLD
__device__ __forceinline__ void stage_tile(const WideArgs& a, int off, int cols, float* Ts, int tid) {
    const int c4n = cols / 4;
    for (int e = tid; e < WR * c4n; e += WT) {
        const int row = e / c4n, c4 = e % c4n;
        MJRL_SLAB_CHECK(off + row * WP + 4 * c4 + 3, a.scap);
        *reinterpret_cast<float4*>(Ts + row * TLD + 4 * c4) =
            *reinterpret_cast<const float4*>(a.scratch + off + row * WP + 4 * c4);
    }
}

// One weight-gradient job of a wave and Adam on its elements (k_pfit's wgrad_job): the 16
// units 16 ublk .. + 15 of the layer whose weight tensor is t (U units, K inputs) against the
// 16 columns col0 .. + 15 of [input, 1].  gl: this job's 16 columns of the layer's upstream
// tile (pitch gld), bl / bld / boff: the input tile and the input column of its column 0.  A
// lane's accumulator register i belongs to the weight [unit 4 q + i][col] (col < K), to that
// unit's bias (col == K) or to nothing.  The upstream rows of masked rows are 0, so the
// column of ones is 1 in every row.
__device__ __forceinline__ void wide_job(const WideArgs& a, int t, int U, int K, int ublk, int col0, const float* gl,
                                         int gld, const float* bl, int bld, int boff, int64_t gw, int64_t gb, int r,
                                         int q) {
    float *const pw = a.p[t], *const mw = a.m[t], *const vw = a.v[t];
    float *const pb = a.p[t + 1], *const mb = a.m[t + 1], *const vb = a.v[t + 1];
    const int col = col0 + r;
    const int colc = col < K ? col : K - 1;
    float pm[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int unit = 16 * ublk + 4 * q + i, uc = unit < U ? unit : U - 1;
        const bool bias = col == K;
        const unsigned e = bias ? (unsigned)uc : (unsigned)uc * K + colc;
        pm[i][0] = (bias ? pb : pw)[e];
        pm[i][1] = (bias ? mb : mw)[e];
        pm[i][2] = (bias ? vb : vw)[e];
    }
    const int lc = col < K ? col - boff : 0;   // a tile column that exists (col >= K: not used)
    floatx4 acc = zero4();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int row = 4 * s + q;
        const float b = bl[row * bld + lc];
        acc = mfma4(gl[row * gld + r], col < K ? b : (col == K ? 1.f : 0.f), acc);
    }
    if (col <= K) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int unit = 16 * ublk + 4 * q + i;
            if (unit >= U) continue;
            wgrad_tail(pm[i], acc[i], unit, K, col, a.hp, pw, mw, vw, pb, mb, vb, a.grad, gw, gb);
        }
    }
}

// ---- layer 0 -------------------------------------------------------------------------------
__global__ void __launch_bounds__(WT) k_wide_l0(WideArgs a) {
    __shared__ __attribute__((aligned(16))) float Ts[WR * TLD];   // g1, then xhat chunk by chunk
    __shared__ float gs[WR * 16];                                 // this workgroup's columns of g0
    __shared__ int64_t s_ru[WR], s_rf[WR];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int u = blockIdx.x;
    const int n = a.n, h0 = a.h0, h1 = a.h1;
    const int UB1 = (h1 + 15) / 16;
    float *const W0 = a.p[0], *const b0 = a.p[1];
    const float* const W1 = a.p[2];

    // ---- round trip 1: the row indices ----
    if (tid < WR)
        s_ru[tid] = a.update ? mb_row(a, a.kU, tid) : -1;
    else if (tid < 2 * WR)
        s_rf[tid - WR] = a.forward ? mb_row(a, a.kF, tid - WR) : -1;

    if (a.update) {
        // g0's columns of this workgroup: rows 16 w .. + 15 by wave w < 4, k over all of g1
        stage_tile(a, G1_OFF, 16 * UB1, Ts, tid);
        __syncthreads();
        if (w < 4) {
            const int col = 16 * u + r;
            floatx4 acc = zero4();
#pragma unroll 4
            for (int g = 0; g < UB1; ++g) {
                const int j = 16 * g + 4 * q;
                const float4 b = ldwt4(W1, h1, h0, j, col);
                const float4 av = *reinterpret_cast<const float4*>(Ts + (16 * w + r) * TLD + j);
                acc = mfma_k16(av, b, acc);
            }
            const float* const a0u = a.scratch + a0_off(a.kU);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = 16 * w + 4 * q + k;
                float gv = 0.f;
                if (col < h0) {
                    MJRL_SLAB_CHECK(a0_off(a.kU) + row * WP + col, a.scap);
                    const float av = a0u[row * WP + col];
                    gv = acc[k] * (1.f - av * av);
                }
                gs[row * 16 + r] = gv;
            }
        }
        // dW0 / db0 of the units 16 u .. + 15 and Adam, one 16-column block of [xhat, 1] a job
        const int64_t o_b0 = (int64_t)h0 * n;
        const int cb0 = n / 16 + 1, nchunk = n / XCW + 1;   // the column of ones (col n) counts
        for (int c = 0; c < nchunk; ++c) {
            __syncthreads();   // the products before have read Ts (and written gs)
            if (n > c * XCW) {   // (a chunk holding only the column of ones needs no tile)
                stage_x(a, s_ru, Ts, c, tid);
                __syncthreads();
            }
            const int nb0 = cb0 - c * (XCW / 16) < XCW / 16 ? cb0 - c * (XCW / 16) : XCW / 16;
            for (int j = w; j < nb0; j += WW)
                wide_job(a, 0, h0, n, u, c * XCW + 16 * j, gs, 16, Ts, TLD, c * XCW, 0, o_b0, r, q);
        }
    }

    if (a.forward) {
        __syncthreads();   // W0 / b0 as this workgroup's waves have just written them; Ts is free; s_rf
        floatx4 acc = zero4();
        const int nchunk = (n + XCW - 1) / XCW;
        for (int c = 0; c < nchunk; ++c) {
            if (c > 0) __syncthreads();
            stage_x(a, s_rf, Ts, c, tid);
            __syncthreads();
            if (w < 4) {
                const int c0 = c * XCW, cw = n - c0 < XCW ? n - c0 : XCW, ng = (cw + 15) / 16;
#pragma unroll 4
                for (int g = 0; g < ng; ++g) {
                    const float4 b = ldw4(W0, h0, n, 16 * u + r, c0 + 16 * g + 4 * q, a.vw0);
                    const float4 av = *reinterpret_cast<const float4*>(Ts + (16 * w + r) * TLD + 16 * g + 4 * q);
                    acc = mfma_k16(av, b, acc);
                }
            }
        }
        if (w < 4) {
            const int col = 16 * u + r;
            const float bias = col < h0 ? b0[col] : 0.f;
            float* const a0f = a.scratch + a0_off(a.kF);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = 16 * w + 4 * q + k;
                MJRL_SLAB_CHECK(a0_off(a.kF) + row * WP + col, a.scap);
                a0f[row * WP + col] = col < h0 ? tanhf(acc[k] + bias) : 0.f;
            }
        }
    }
}

// ---- layer 1 -------------------------------------------------------------------------------
__global__ void __launch_bounds__(WT) k_wide_l1(WideArgs a) {
    __shared__ __attribute__((aligned(16))) float As[WR * TLD];   // a0 of the update step, then of the forward step
    __shared__ float gs[WR * 16];                                 // this workgroup's columns of g1
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int u = blockIdx.x;
    const int n = a.n, h0 = a.h0, h1 = a.h1;
    const int UB0 = (h0 + 15) / 16;
    float *const W1 = a.p[2], *const b1 = a.p[3];

    if (a.update) {
        stage_tile(a, a0_off(a.kU), 16 * UB0, As, tid);
        for (int e = tid; e < WR * 16; e += WT) {
            MJRL_SLAB_CHECK(G1_OFF + (e >> 4) * WP + 16 * u + (e & 15), a.scap);
            gs[e] = a.scratch[G1_OFF + (e >> 4) * WP + 16 * u + (e & 15)];
        }
        __syncthreads();
        const int64_t o_W1 = (int64_t)h0 * n + h0, o_b1 = o_W1 + (int64_t)h1 * h0;
        const int CB1 = h0 / 16 + 1;   // column blocks of [a0, 1]
        for (int j = w; j < CB1; j += WW) wide_job(a, 2, h1, h0, u, 16 * j, gs, 16, As, TLD, 0, o_W1, o_b1, r, q);
    }

    if (a.forward) {
        if (a.update) __syncthreads();   // W1 / b1 as this workgroup's waves have just written them; As is free
        stage_tile(a, a0_off(a.kF), 16 * UB0, As, tid);
        __syncthreads();
        if (w < 4) {
            floatx4 acc = zero4();
#pragma unroll 4
            for (int g = 0; g < UB0; ++g) {
                const float4 b = ldw4(W1, h1, h0, 16 * u + r, 16 * g + 4 * q, a.vw1);
                const float4 av = *reinterpret_cast<const float4*>(As + (16 * w + r) * TLD + 16 * g + 4 * q);
                acc = mfma_k16(av, b, acc);
            }
            const int col = 16 * u + r;
            const float bias = col < h1 ? b1[col] : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = 16 * w + 4 * q + k;
                MJRL_SLAB_CHECK(A1_OFF + row * WP + col, a.scap);
                a.scratch[A1_OFF + row * WP + col] = col < h1 ? tanhf(acc[k] + bias) : 0.f;
            }
        }
    }
}

// ---- the head: k_pfit's phases 1, 4 - 7 and layer 2's part of 9 on a 256-wide a1 --------------
// MSE: the mean-squared-error head (behavior_cloning_2.py:46-50) on the six tensors of the mean
// network; p[6] / m[6] / v[6] are null there and nothing touches them.
template <bool MSE>
__global__ void __launch_bounds__(WT) k_wide_head(WideArgs a) {
    __shared__ __attribute__((aligned(16))) float a1s[WR * TLD];
    __shared__ __attribute__((aligned(16))) float zs[WR * ZLD];    // z, then gmu
    __shared__ int64_t s_row[WR];                                  // row index, -1: masked
    __shared__ double s_lossd[WR], s_q[WM], s_lsum[2];             // s_q: 1 - (sigma / sigma_old)^2
    __shared__ float s_gll[WR], s_sig[WM], s_gsc[WM];              // dL/dLL; sigma; out_scale / sigma
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int m = a.na, h1 = a.h1, bs = a.bs;
    const int UB1 = (h1 + 15) / 16, UB2 = (m + 15) / 16, MP = 16 * UB2;
    const bool aliased = a.kind == PF_PPO && a.old_ls != nullptr;
    float *const W2 = a.p[4], *const b2 = a.p[5], *const ls = a.p[6];
    const int64_t o_W2 = (int64_t)a.h0 * a.n + a.h0 + (int64_t)h1 * a.h0 + h1, o_b2 = o_W2 + (int64_t)m * h1,
                  o_ls = o_b2 + m;
    const int ub = w & 3, rb0 = 2 * (w >> 2);   // mu: wave w owns unit block w & 3, row blocks 2 (w >> 2), + 1

    // ---- 1: the row indices, the per-column constants; a1 into LDS ----
    if (w == 0) {
        s_row[lane] = mb_row(a, a.kF, lane);
    } else if (MSE) {
        if (w == 1) s_gsc[lane] = lane < m ? a.out_scale[lane] : 0.f;   // sigma is 1: log_std is not read
    } else if (w == 1) {
        const float lsv = lane < m ? ls[lane] : 0.f;
        const float sg = expf(lsv);
        float olsv = 0.f;
        double qq = 0.0;
        if (aliased && lane < m) {
            olsv = a.old_ls[lane];
            const double rr = (double)sg / (double)expf(olsv);
            qq = 1.0 - rr * rr;
        }
        s_sig[lane] = sg;
        s_gsc[lane] = lane < m ? a.out_scale[lane] / sg : 0.f;
        s_q[lane] = qq;
        const double s0 = wave_sum((double)lsv), s1 = wave_sum((double)olsv);
        if (lane == 0) {
            s_lsum[0] = s0;
            s_lsum[1] = s1;
        }
    }
    stage_tile(a, A1_OFF, 16 * UB1, a1s, tid);
    __syncthreads();

    // ---- 4: mu = (a1 W2^T + b2) out_scale + out_shift, z = (act - mu) / sigma ----
    if (ub < UB2) {
        floatx4 acc[2] = {zero4(), zero4()};
#pragma unroll 4
        for (int g = 0; g < UB1; ++g) {
            const float4 b = ldw4(W2, m, h1, 16 * ub + r, 16 * g + 4 * q, a.vw2);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float4 av = *reinterpret_cast<const float4*>(a1s + (16 * (rb0 + i) + r) * TLD + 16 * g + 4 * q);
                acc[i] = mfma_k16(av, b, acc[i]);
            }
        }
        const int col = 16 * ub + r;
        const bool in = col < m;
        const float bias = in ? b2[col] : 0.f, osc = in ? a.out_scale[col] : 0.f, osh = in ? a.out_shift[col] : 0.f;
        const float sg = MSE ? 1.f : s_sig[col];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = 16 * (rb0 + i) + 4 * q + k;
                const int64_t xi = s_row[row];
                float z = 0.f;
                if (in && xi >= 0) {   // nothing of act is read for a masked row
                    const float mu = (acc[i][k] + bias) * osc + osh;
                    z = a.act[xi * m + col] - mu;
                    if (!MSE) z = z / sg;
                }
                zs[row * ZLD + col] = z;
            }
    }
    __syncthreads();

    // ---- 5: per row LL, the loss head, dL/dLL: 8 lanes per row, 8 columns each ----
    {
        const int row = tid >> 3, part = tid & 7;
        double sz = 0.0, sd = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = 8 * part + j;
            if (col < m) {
                const double z = (double)zs[row * ZLD + col];
                sz += z * z;
                if (!MSE) sd += z * z * s_q[col];
            }
        }
        sz += __shfl_xor(sz, 1, 64);
        if (!MSE) sd += __shfl_xor(sd, 1, 64);
        sz += __shfl_xor(sz, 2, 64);
        if (!MSE) sd += __shfl_xor(sd, 2, 64);
        sz += __shfl_xor(sz, 4, 64);
        if (!MSE) sd += __shfl_xor(sd, 4, 64);
        if (part == 0) {
            const int64_t xi = s_row[row];
            float gll = 0.f;
            double lrow = 0.0;
            if (MSE) {
                // the row's term is sum z^2 / m, z = act - mu; -2 / (bs m) in gll's place makes
                // gmu below 2 (mu - act) out_scale / (bs m)
                if (xi >= 0) {
                    gll = -2.f / (float)(bs * m);
                    lrow = sz / (double)m;
                }
            } else if (xi >= 0) {
                const double LL = -0.5 * sz - s_lsum[0] - (double)m * HALF_LOG_2PI;
                if (a.kind == PF_BC) {
                    gll = -1.f / (float)bs;
                    lrow = -LL;
                } else {
                    // LL - LL_old; aliased: the same mu under old_log_std, no gradient through it
                    const double dll = aliased ? -0.5 * sd - (s_lsum[0] - s_lsum[1]) : LL - (double)a.ll_old[xi];
                    const float LR = (float)exp(dll);
                    const float adv = a.adv[xi];
                    const float LRc = LR < a.clip_lo ? a.clip_lo : (LR > a.clip_hi ? a.clip_hi : LR);
                    const float s1 = LR * adv, s2 = LRc * adv;
                    // torch's min / clamp: a tie passes the whole gradient, the clipped branch none
                    gll = s1 <= s2 ? -(adv * LR) / (float)bs : 0.f;
                    lrow = -(double)(s1 < s2 ? s1 : s2);
                }
            }
            s_gll[row] = gll;
            s_lossd[row] = lrow;
        }
    }
    __syncthreads();

    // ---- 6: d log_std (wave 0), the step's loss (wave 1); then gmu in place of z ----
    float dls = 0.f;
    if (!MSE && w == 0) {
        if (lane < m) {
            double s = 0.0;
            for (int row = 0; row < WR; ++row) {
                const double z = (double)zs[row * ZLD + lane];
                s += (double)s_gll[row] * (z * z - 1.0);
            }
            dls = (float)s;
        }
    } else if (w == 1) {
        const double tot = wave_sum(s_lossd[lane]) / (double)bs;
        if (lane == 0) {
            MJRL_SLAB_CHECK(LOSS_OFF, a.scap);
            a.scratch[LOSS_OFF] = (float)tot;
            if (a.loss) *a.loss = (float)tot;
        }
    }
    __syncthreads();
    for (int e = tid; e < WR * MP; e += WT) {
        const int row = e / MP, col = e % MP;
        zs[row * ZLD + col] = s_gll[row] * (zs[row * ZLD + col] * s_gsc[col]);
    }
    __syncthreads();

    // ---- 7: g1 = (gmu W2) o (1 - a1^2) for the next launches: wave w the unit blocks w, w + 8 ----
    for (int ubb = w; ubb < UB1; ubb += WW) {
        floatx4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
        const int col = 16 * ubb + r;
        for (int g = 0; g < UB2; ++g) {
            const int j = 16 * g + 4 * q;
            const float4 b = ldwt4(W2, m, h1, j, col);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 av = *reinterpret_cast<const float4*>(zs + (16 * i + r) * ZLD + j);
                acc[i] = mfma_k16(av, b, acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = 16 * i + 4 * q + k;
                const float av = a1s[row * TLD + col];
                MJRL_SLAB_CHECK(G1_OFF + row * WP + col, a.scap);
                a.scratch[G1_OFF + row * WP + col] = col < h1 ? acc[i][k] * (1.f - av * av) : 0.f;
            }
    }
    __syncthreads();   // every read of this step's W2 / b2 / log_std is behind us

    // ---- 9 (layer 2): dW2 = gmu^T [a1, 1] as 16 x 16 jobs with Adam, log_std's Adam ----
    if (!MSE && w == 0 && lane < m) {
        float p1, m1, v1;
        adam_step(ls[lane], a.m[6][lane], a.v[6][lane], dls, a.hp, p1, m1, v1);
        if (a.grad) a.grad[o_ls + lane] = dls;
        ls[lane] = p1;
        a.m[6][lane] = m1;
        a.v[6][lane] = v1;
    }
    const int CB2 = h1 / 16 + 1;   // column blocks of [a1, 1]
    for (int j = w; j < UB2 * CB2; j += WW)
        wide_job(a, 4, m, h1, j / CB2, 16 * (j % CB2), zs + 16 * (j / CB2), ZLD, a1s, TLD, 0, o_W2, o_b2, r, q);
}

// What both entry points share once their arguments are checked: the sizes, the row and
// transformation pointers, the 16-byte-load flags, then the launches of nmb steps.  a.p / m / v,
// a.adv / ll_old / old_ls, a.kind and the clip range are the caller's.
template <bool MSE>
int run_wide(WideArgs& a, const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
             const mjrl_adam* hp, float* scratch, float* grad_out, float* loss_out, void* stream) {
    const int n = data->n, m = data->m, h0 = data->h0, h1 = data->h1;
    hipStream_t st = (hipStream_t)stream;
    a.obs = data->obs;
    a.act = data->act;
    a.in_shift = data->in_shift;
    a.in_scale = data->in_scale;
    a.out_shift = data->out_shift;
    a.out_scale = data->out_scale;
    a.idx = idx;
    a.T = data->T;
    a.scratch = scratch;
    a.scap = W_SCRATCH;
    a.n = n;
    a.na = m;
    a.h0 = h0;
    a.h1 = h1;
    a.bs = bs;
    const int64_t d = (int64_t)h0 * n + h0 + (int64_t)h1 * h0 + h1 + (int64_t)m * h1 + m + (MSE ? 0 : m);
    const auto al16 = [](const void* p) { return (uintptr_t)p % 16 == 0; };
    a.vx = n % 4 == 0 && al16(data->obs) && al16(data->in_shift) && al16(data->in_scale);
    a.vw0 = n % 4 == 0 && al16(a.p[0]);
    a.vw1 = h0 % 4 == 0 && al16(a.p[2]);
    a.vw2 = h1 % 4 == 0 && al16(a.p[4]);
    a.hp = adam_consts(hp);
    const dim3 g0((h0 + 15) / 16), g1((h1 + 15) / 16), blk(WT);
    a.grad = nullptr;
    a.loss = nullptr;
    a.kU = a.kF = 0;
    a.update = 0;
    a.forward = 1;
    hipLaunchKernelGGL(k_wide_l0, g0, blk, 0, st, a);
    hipLaunchKernelGGL(k_wide_l1, g1, blk, 0, st, a);
    for (int64_t k = 0; k < nmb; ++k) {
        adam_bias(hp, k, a.hp.step_size, a.hp.bc2s);
        a.grad = grad_out ? grad_out + k * d : nullptr;
        a.loss = loss_out ? loss_out + k : nullptr;
        a.kU = a.kF = k;
        hipLaunchKernelGGL(k_wide_head<MSE>, dim3(1), blk, 0, st, a);
        a.kF = k + 1;
        a.update = 1;
        a.forward = k + 1 < nmb;
        hipLaunchKernelGGL(k_wide_l0, g0, blk, 0, st, a);
        hipLaunchKernelGGL(k_wide_l1, g1, blk, 0, st, a);
    }
    return (int)hipGetLastError();
}

// the checks both entry points make on what they both read; nmb > 0: the pointers too
bool sizes_ok(const mjrl_policy_fit_data* data, int64_t nmb, int32_t bs) {
    if (!data || bs < 1 || bs > WR || nmb < 0) return false;
    const int n = data->n, m = data->m, h0 = data->h0, h1 = data->h1;
    // n <= 2^24: the kernels index a tensor's elements with 32 bits
    return n > 0 && n <= (1 << 24) && m >= 1 && m <= WM && h0 >= 1 && h0 <= WH && h1 >= 1 && h1 <= WH && data->T >= 0;
}

bool pointers_ok(const mjrl_policy_fit_data* data, const int64_t* idx, const void* net, const mjrl_adam* hp,
                 const float* scratch) {
    if (!idx || !net || !hp || !scratch || hp->step0 < 0) return false;
    return data->obs && data->act && data->in_shift && data->in_scale && data->out_shift && data->out_scale;
}

}  // namespace

extern "C" {

int mjrl_policy_fit_wide_scratch(int32_t n, int32_t m, int32_t h0, int32_t h1, int32_t bs, int64_t* floats) {
    if (n <= 0 || m < 1 || m > WM || h0 < 1 || h0 > WH || h1 < 1 || h1 > WH || bs < 1 || bs > WR || !floats)
        return MJRL_EINVAL;
    *floats = W_SCRATCH;
    return MJRL_OK;
}

int mjrl_policy_fit_wide_epoch(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
                               const mjrl_policy_net* net, const mjrl_adam* hp, float* scratch, float* grad_out,
                               float* loss_out, void* stream) {
    if (!sizes_ok(data, nmb, bs)) return MJRL_EINVAL;
    if (data->kind != MJRL_POLICY_FIT_BC && data->kind != MJRL_POLICY_FIT_PPO) return MJRL_EINVAL;
    if (data->kind == MJRL_POLICY_FIT_PPO && (!data->ll_old == !data->old_log_std)) return MJRL_EINVAL;
    if (nmb == 0) return MJRL_OK;
    if (!pointers_ok(data, idx, net, hp, scratch)) return MJRL_EINVAL;
    if (data->kind == MJRL_POLICY_FIT_PPO && !data->adv) return MJRL_EINVAL;
    WideArgs a;
    if (!net_ptrs(net, a.p, a.m, a.v)) return MJRL_EINVAL;
    a.adv = data->adv;
    a.ll_old = data->kind == MJRL_POLICY_FIT_PPO ? data->ll_old : nullptr;
    a.old_ls = data->kind == MJRL_POLICY_FIT_PPO ? data->old_log_std : nullptr;
    a.kind = data->kind == MJRL_POLICY_FIT_PPO ? PF_PPO : PF_BC;
    a.clip_lo = (float)(1.0 - data->clip);
    a.clip_hi = (float)(1.0 + data->clip);
    return run_wide<false>(a, data, idx, nmb, bs, hp, scratch, grad_out, loss_out, stream);
}

int mjrl_policy_mse_wide_epoch(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
                               const mjrl_mean_net* net, const mjrl_adam* hp, float* scratch, float* grad_out,
                               float* loss_out, void* stream) {
    if (!sizes_ok(data, nmb, bs)) return MJRL_EINVAL;
    if (nmb == 0) return MJRL_OK;
    if (!pointers_ok(data, idx, net, hp, scratch)) return MJRL_EINVAL;
    WideArgs a;
    float *p6[6], *m6[6], *v6[6];
    if (!net_ptrs(net, p6, m6, v6)) return MJRL_EINVAL;
    for (int i = 0; i < 6; ++i) {
        a.p[i] = p6[i];
        a.m[i] = m6[i];
        a.v[i] = v6[i];
    }
    a.p[6] = a.m[6] = a.v[6] = nullptr;   // no log_std in this net: the MSE instantiation never touches them
    a.adv = a.ll_old = a.old_ls = nullptr;   // data's adv / ll_old / old_log_std / kind / clip are not read
    a.kind = PF_BC;
    a.clip_lo = a.clip_hi = 1.f;
    return run_wide<true>(a, data, idx, nmb, bs, hp, scratch, grad_out, loss_out, stream);
}

}  // extern "C"
