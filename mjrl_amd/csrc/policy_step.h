// policy_step.h — what the fused minibatch Adam fits of the Gaussian MLP policy share
// (policy_fit.hip: one workgroup, widths up to 64; policy_fit_wide.hip: three kernels a step,
// widths up to 256; policy_fit_rows.hip: one workgroup per 64 rows of a minibatch of up to 16384,
// two kernels a step): the argument block, the tile constants, the places of the tensors in a flat
// gradient, the gathered X tile, the chain products (forward, tanh epilogue, backward with its
// 1 - a^2 epilogue), the weight-gradient product with its two jobs and phase 9's walk over them,
// the loss heads with log_std's part of the step, and the host's checks and argument filling.
//
// The policy is Linear(n, h0) - tanh - Linear(h0, h1) - tanh - Linear(h1, m) plus log_std[m] in
// torch's layouts and order.  A step trains on bs <= 64 rows named by a device index buffer
// (policy_fit_rows.hip: a row tile holds 64 of a step's bs rows); rows
// bs .. 63 and a row whose index is outside [0, T) are masked: nothing of obs / act / adv / ll_old
// is read for them, their dL/dLL is 0, the mean still divides by bs.  template <bool MSE>: false,
// BC's -mean LL or PPO's clipped surrogate on the seven tensors; true, the MSE head of
// mjrl/algos/behavior_cloning_2.py:46-50, L = sum (mu - act)^2 / (bs m), on the six tensors of
// the mean network (sigma is 1, log_std is never read, p[6] / m[6] / v[6] are null).
#pragma once

#include "fit.h"

namespace mjrl {

constexpr int PS_ROWS = 64;           // padded minibatch rows
constexpr int PS_NA = 64;             // largest action width
constexpr int PS_XCW = 256;           // columns of the X tile held in LDS at a time
constexpr int PS_XLD = PS_XCW + 4;    // its row pitch
constexpr int PS_H = 64;              // largest hidden width of the one-workgroup chains (k_pfit, k_pfr_grad)
constexpr int PS_LD = PS_H + 4;       // LDS row pitch of their [64][64] tiles: rows 4 banks apart
constexpr int PS_THREADS = 512;       // threads of every workgroup
constexpr int PF_BC = 0, PF_PPO = 1;
constexpr double HALF_LOG_2PI = 0.91893853320467274178;

// what every kernel of both files is told (each file's own block extends it)
struct StepArgs {
    const float *obs, *act, *adv, *ll_old, *old_ls;
    const float *in_shift, *in_scale, *out_shift, *out_scale;
    const int64_t* idx;               // minibatch 0 of the launch (policy_fit) / of the call (wide)
    int64_t T;
    float *p[7], *m[7], *v[7];        // W0, b0, W1, b1, W2, b2, log_std (torch order) and their Adam moments
    float* scratch;
    int64_t scap;                     // floats of scratch (debug build: checked)
    float* grad;                      // null or a [d] gradient: the launch's first / the one the launch writes
    float* loss;                      // null or a loss slot: the launch's first / the head's
    int64_t d;                        // floats of a step's gradient (in k_pfit's own block: its MSE head 0.3 % slower)
    int n, na, h0, h1, bs, kind;      // na: the action width m
    int vx, vw0, vw1, vw2;            // 16-byte loads of obs rows / W0 / W1 / W2 rows allowed
    float clip_lo, clip_hi;           // float(1 - c), float(1 + c)
    AdamK hp;                         // the step-independent part (policy_fit) / of the step the launch updates
};

// The flat places of b0, W1, b1, W2, b2 and log_std in a step's gradient (torch parameter order,
// W0 at 0) and d, its floats (MSE: no log_std).
struct GradAt {
    int64_t b0, W1, b1, W2, b2, ls, d;
};
__host__ __device__ __forceinline__ GradAt grad_at(int n, int m, int h0, int h1, bool mse) {
    GradAt o;
    o.b0 = (int64_t)h0 * n;
    o.W1 = o.b0 + h0;
    o.b1 = o.W1 + (int64_t)h1 * h0;
    o.W2 = o.b1 + h1;
    o.b2 = o.W2 + (int64_t)m * h1;
    o.ls = o.b2 + m;
    o.d = o.ls + (mse ? 0 : m);
    return o;
}

// row index of minibatch k's row r, or -1 for a masked row
__device__ __forceinline__ int64_t mb_row(const StepArgs& a, int64_t k, int r) {
    if (r >= a.bs) return -1;
    const int64_t i = a.idx[k * a.bs + r];
    return i >= 0 && i < a.T ? i : -1;
}

// the gathered, normalised X tile of chunk c for the rows s_row into Xs (pitch LD): 8 threads
// per row, zero-filled to a multiple of 16 columns; n: the caller's copy of a.n
template <int LD>
__device__ __forceinline__ void stage_x(const StepArgs& a, int n, const int64_t* s_row, float* Xs, int c, int tid) {
    constexpr int XCW = PS_XCW;
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
            *reinterpret_cast<float4*>(Xs + xr * LD + col) = o;
        }
    } else {
#pragma unroll 8
        for (int i = 0; i < XCW / 8; ++i) {
            const int col = xc + 8 * i;
            if (col >= cwp) continue;
            float o = 0.f;
            if (xi >= 0 && col < cw) o = (xrow[col] - a.in_shift[c0 + col]) / (a.in_scale[c0 + col] + 1e-8f);
            Xs[xr * LD + col] = o;
        }
    }
}

// ---- the chain products: a lane is (r, q) = (lane & 15, lane >> 4) of its wave, which owns the
// 16 units 16 ub .. + 15 of a layer and the NB row blocks rb0 .. + NB - 1 of 16 rows ----------------
// acc[i] += A[rows of block rb0 + i][16 g + 4 q ..] . W[unit][k0 + 16 g + 4 q ..] over g = 0 .. ng - 1,
// k ascending; A: an LDS tile of pitch LD, W: a [U][K] weight tensor, vec: its vw flag
template <int LD, int NB>
__device__ __forceinline__ void chain_fwd(floatx4 (&acc)[NB], const float* A, int rb0, const float* W, int U, int K,
                                          int ub, int k0, int ng, int vec, int r, int q) {
#pragma unroll 4
    for (int g = 0; g < ng; ++g) {
        const float4 b = ldw4(W, U, K, 16 * ub + r, k0 + 16 * g + 4 * q, vec);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const float4 av = *reinterpret_cast<const float4*>(A + (16 * (rb0 + i) + r) * LD + 16 * g + 4 * q);
            acc[i] = mfma_k16(av, b, acc[i]);
        }
    }
}

// Layer 0's products over the column chunks of the gathered X tile Xs (pitch LD; load(c) stages
// chunk c, a barrier on either side of it), by the waves that are active; stamp: as in wgrad_walk
template <int LD, int NB, class Load, class Stamp>
__device__ __forceinline__ void chain_fwd_x(floatx4 (&acc)[NB], const float* Xs, bool active, int rb0, const float* W0,
                                            int h0, int n, int ub, int vec, int r, int q, const Load& load,
                                            const Stamp& stamp) {
    constexpr int XCW = PS_XCW;
    const int nchunk_f = (n + XCW - 1) / XCW;
    for (int c = 0; c < nchunk_f; ++c) {
        if (c > 0) __syncthreads();   // the previous chunk's products have read Xs
        load(c);
        __syncthreads();
        stamp(c == 0 ? 1 : 12);
        if (active) {
            const int c0 = c * XCW, cw = n - c0 < XCW ? n - c0 : XCW;
            chain_fwd<LD, NB>(acc, Xs, rb0, W0, h0, n, ub, c0, (cw + 15) / 16, vec, r, q);
        }
    }
}

// tanh(acc + b) of the wave's two row blocks into the LDS tile dst (pitch LD), 0 in the columns from U on
template <int LD>
__device__ __forceinline__ void chain_tanh(const floatx4 (&acc)[2], float* dst, int rb0, const float* b, int U, int ub,
                                           int r, int q) {
    const int col = 16 * ub + r;
    const float bias = col < U ? b[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            dst[(16 * (rb0 + i) + 4 * q + k) * LD + col] = col < U ? tanhf(acc[i][k] + bias) : 0.f;
}

// acc[i] += G[rows of block rb0 + i][16 g + 4 q ..] . W[16 g + 4 q ..][col] over g = 0 .. ng - 1: the
// upstream LDS tile G (pitch LD) through the transpose of the [U][K] weight tensor W
template <int LD, int NB>
__device__ __forceinline__ void chain_bwd_prod(floatx4 (&acc)[NB], const float* G, int rb0, const float* W, int U,
                                               int K, int col, int ng, int r, int q) {
    for (int g = 0; g < ng; ++g) {
        const int j = 16 * g + 4 * q;
        const float4 b = ldwt4(W, U, K, j, col);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const float4 av = *reinterpret_cast<const float4*>(G + (16 * (rb0 + i) + r) * LD + j);
            acc[i] = mfma_k16(av, b, acc[i]);
        }
    }
}

// dst = (G W) o (1 - act^2) for the wave's unit block of the K inputs of W and its two row blocks;
// G, act, dst: LDS tiles of pitch LD
template <int LD>
__device__ __forceinline__ void chain_bwd(const float* G, const float* W, int U, int K, int ng, const float* act,
                                          float* dst, int ub, int rb0, int r, int q) {
    floatx4 acc[2] = {zero4(), zero4()};
    const int col = 16 * ub + r;
    chain_bwd_prod<LD, 2>(acc, G, rb0, W, U, K, col, ng, r, q);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = 16 * (rb0 + i) + 4 * q + k;
            const float av = act[row * LD + col];
            dst[row * LD + col] = col < K ? acc[i][k] * (1.f - av * av) : 0.f;
        }
}

// ---- the weight gradients ------------------------------------------------------------------------
// The product of one weight-gradient job of a wave: the 16 units of a layer (K inputs) at the tile
// columns goff .. + 15 of the upstream tile gl (pitch gld) against the columns col - r .. + 15 of
// [input, 1]; bl / bld / boff: the input tile, its pitch and the input column of its column 0.  A
// lane's accumulator register i belongs to the weight [unit 4 q + i][col] (col < K), to that
// unit's bias (col == K) or to nothing; the upstream rows of masked rows are 0, so the column of
// ones is 1 in every row.
__device__ __forceinline__ floatx4 wgrad_prod(int K, int col, const float* gl, int gld, int goff, const float* bl,
                                              int bld, int boff, int r, int q) {
    const int lc = col < K ? col - boff : 0;   // a tile column that exists (col >= K: not used)
    floatx4 acc = zero4();
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int row = 4 * s + q;
        const float b = bl[row * bld + lc];
        acc = mfma4(gl[row * gld + goff + r], col < K ? b : (col == K ? 1.f : 0.f), acc);
    }
    return acc;
}

// One job and Adam (hp) on its elements: the 16 units 16 ublk .. + 15 of the layer whose weight
// tensor is t (U units, K inputs) against the 16 columns col0 .. + 15 of [input, 1] (wgrad_prod).
// grad: null or the step's gradient, gw / gb the layer's places in it.
__device__ __forceinline__ void wgrad_job(const StepArgs& a, const AdamK& hp, float* grad, int t, int U, int K,
                                          int ublk, int col0, const float* gl, int gld, int goff, const float* bl,
                                          int bld, int boff, int64_t gw, int64_t gb, int r, int q) {
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
    const floatx4 acc = wgrad_prod(K, col, gl, gld, goff, bl, bld, boff, r, q);
    if (col <= K) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int unit = 16 * ublk + 4 * q + i;
            if (unit >= U) continue;
            wgrad_tail(pm[i], acc[i], unit, K, col, hp, pw, mw, vw, pb, mb, vb, grad, gw, gb);
        }
    }
}

// The job without the step (policy_fit_rows.hip: Adam follows a kernel boundary, on the gradients
// of all row tiles folded): the same accumulator goes to its flat place gw / gb of one row tile's
// [d] slice of the scratch, which starts at float off.
__device__ __forceinline__ void wgrad_store_job(const StepArgs& a, int64_t off, int U, int K, int ublk, int col0,
                                                const float* gl, int gld, int goff, const float* bl, int bld,
                                                int boff, int64_t gw, int64_t gb, int r, int q) {
    const int col = col0 + r;
    const floatx4 acc = wgrad_prod(K, col, gl, gld, goff, bl, bld, boff, r, q);
    if (col <= K) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int unit = 16 * ublk + 4 * q + i;
            if (unit >= U) continue;
            const int64_t e = off + (col < K ? gw + (int64_t)unit * K + col : gb + unit);
            MJRL_SLAB_CHECK(e, a.scap);
            a.scratch[e] = acc[i];
        }
    }
}

// the LDS tiles of a one-workgroup chain: xhat (one chunk of columns, pitch PS_XLD), then pitch PS_LD
struct ChainTiles {
    float *Xs, *a0s, *a1s, *g0s, *g1s, *zs;   // zs: z, then gmu
};

// Phase 9's walk of wave w (of PS_THREADS / 64) over the 16 x 16 jobs of a step: dW2 = gmu^T [a1, 1],
// dW1 = g1^T [a0, 1], dW0 = g0^T [xhat, 1] chunk by chunk, the last forward chunk first (it is
// still in LDS); the bias sums ride along as a column of ones.  load(c): stage chunk c of xhat;
// job(t, U, K, jub, col0, gl, bl, bld, boff, gw, gb): the units 16 jub .. + 15 of the layer whose
// weight tensor is t (upstream tile gl, pitch PS_LD) against 16 columns of [input, 1];
// stamp(i): the phase profile's stamp i (profiling builds of k_pfit).
template <class Load, class Job, class Stamp>
__device__ __forceinline__ void wgrad_walk(int n, int m, int h0, int h1, int w, const ChainTiles& t, const GradAt& o,
                                           const Load& load, const Job& job, const Stamp& stamp) {
    constexpr int XCW = PS_XCW;
    const int UB0 = (h0 + 15) / 16, UB1 = (h1 + 15) / 16, UB2 = (m + 15) / 16;   // unit blocks
    const int CB2 = h1 / 16 + 1, CB1 = h0 / 16 + 1;   // column blocks of [a1, 1], [a0, 1]
    const int nj2 = UB2 * CB2, nj1 = UB1 * CB1;
    const int nchunk_b = n / XCW + 1;   // backward chunks: the column of ones (col n) counts
    int resident = (n + XCW - 1) / XCW - 1;   // the last forward chunk
    for (int c = nchunk_b - 1; c >= 0; --c) {
        if (c != resident && n > c * XCW) {   // (a chunk holding only the column of ones needs no tile)
            stamp(10);
            __syncthreads();   // the previous chunk's jobs have read Xs
            stamp(13);
            load(c);
            __syncthreads();
            resident = c;
            stamp(9);
        }
        const int cb0 = n / 16 + 1 - c * (XCW / 16);          // layer 0's column blocks from this chunk on
        const int nb0 = cb0 < XCW / 16 ? cb0 : XCW / 16;
        const int nj0 = UB0 * nb0;
        const int nj = nj0 + (c == nchunk_b - 1 ? nj2 + nj1 : 0);   // the first chunk visited carries layers 2 and 1
        for (int j = w; j < nj; j += PS_THREADS / 64) {
            if (j < nj0)
                job(0, h0, n, j / nb0, c * XCW + 16 * (j % nb0), t.g0s, t.Xs, PS_XLD, c * XCW, 0, o.b0);
            else if (j < nj0 + nj2)
                job(4, m, h1, (j - nj0) / CB2, 16 * ((j - nj0) % CB2), t.zs, t.a1s, PS_LD, 0, o.W2, o.b2);
            else
                job(2, h1, h0, (j - nj0 - nj2) / CB1, 16 * ((j - nj0 - nj2) % CB1), t.g1s, t.a0s, PS_LD, 0, o.W1, o.b1);
        }
    }
}

// ---- the head: one wave's or one workgroup's part each, the callers' barriers between them ----
// The per-column constants, by one wave: s_sig = sigma, s_gsc = out_scale / sigma, s_q =
// 1 - (sigma / sigma_old)^2 (aliased: PPO with old_log_std), s_lsum = sum log_std, sum old_log_std.
template <bool MSE>
__device__ __forceinline__ void head_consts(const StepArgs& a, bool aliased, int lane, float* s_sig, float* s_gsc,
                                            double* s_q, double* s_lsum) {
    const int m = a.na;
    if (MSE) {
        s_gsc[lane] = lane < m ? a.out_scale[lane] : 0.f;   // sigma is 1: log_std is not read
    } else {
        const float lsv = lane < m ? a.p[6][lane] : 0.f;
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
}

// The epilogue of the mu product of a wave that owns unit block ub and the row blocks rb0, + 1:
// mu = (acc + b2) out_scale + out_shift, z = (act - mu) / sigma (MSE: act - mu) into zs (pitch ZLD)
template <bool MSE, int ZLD>
__device__ __forceinline__ void head_z(const StepArgs& a, const floatx4 (&acc)[2], int ub, int rb0, int r, int q,
                                       const float* s_sig, const int64_t* s_row, float* zs) {
    const int m = a.na;
    const int col = 16 * ub + r;
    const bool in = col < m;
    const float bias = in ? a.p[5][col] : 0.f, osc = in ? a.out_scale[col] : 0.f, osh = in ? a.out_shift[col] : 0.f;
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

// Per row LL, the loss head, dL/dLL (s_gll), the row's loss term (s_lossd): 8 lanes a row, 8 columns each
template <bool MSE, int ZLD>
__device__ __forceinline__ void head_rows(const StepArgs& a, bool aliased, int tid, const float* zs, const double* s_q,
                                          const double* s_lsum, const int64_t* s_row, float* s_gll, double* s_lossd) {
    const int m = a.na, bs = a.bs;
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

// d log_std of column lane over the 64 rows (0 from column m on), by one wave
template <int ZLD>
__device__ __forceinline__ float head_dls(int m, int lane, const float* zs, const float* s_gll) {
    if (lane >= m) return 0.f;
    double s = 0.0;
    for (int row = 0; row < PS_ROWS; ++row) {
        const double z = (double)zs[row * ZLD + lane];
        s += (double)s_gll[row] * (z * z - 1.0);
    }
    return (float)s;
}

// d log_std (wave 0: the value returned) and the step's loss (wave 1) into scratch[slot] and *loss (or null)
template <bool MSE, int ZLD>
__device__ __forceinline__ float head_sums(const StepArgs& a, int w, int lane, const float* zs, const float* s_gll,
                                           const double* s_lossd, int slot, float* loss) {
    float dls = 0.f;
    if (!MSE && w == 0) {
        dls = head_dls<ZLD>(a.na, lane, zs, s_gll);
    } else if (w == 1) {
        const double tot = wave_sum(s_lossd[lane]) / (double)a.bs;
        if (lane == 0) {
            MJRL_SLAB_CHECK(slot, a.scap);
            a.scratch[slot] = (float)tot;
            if (loss) *loss = (float)tot;
        }
    }
    return dls;
}

// gmu = dL/dLL z out_scale / sigma in place of z, over the MP = round_up(m, 16) columns
template <int ZLD>
__device__ __forceinline__ void head_gmu(float* zs, const float* s_gll, const float* s_gsc, int MP, int tid) {
    for (int e = tid; e < PS_ROWS * MP; e += PS_THREADS) {
        const int row = e / MP, col = e % MP;
        zs[row * ZLD + col] = s_gll[row] * (zs[row * ZLD + col] * s_gsc[col]);
    }
}

// log_std's Adam for lane < m of one wave; dls into grad[o_ls + lane] (grad may be null)
__device__ __forceinline__ void log_std_adam(const StepArgs& a, const AdamK& hp, float dls, int lane, float* grad,
                                             int64_t o_ls) {
    float p1, m1, v1;
    adam_step(a.p[6][lane], a.m[6][lane], a.v[6][lane], dls, hp, p1, m1, v1);
    if (grad) grad[o_ls + lane] = dls;
    a.p[6][lane] = p1;
    a.m[6][lane] = m1;
    a.v[6][lane] = v1;
}

// ---- host: the sizes a file's entry points take (hidden widths up to max_hidden, minibatches
// of up to max_rows rows: PS_ROWS but for the row-tiled policy_fit_rows.hip) ----------------------
inline bool widths_ok(int32_t n, int32_t m, int32_t h0, int32_t h1, int32_t bs, int max_hidden,
                      int max_rows = PS_ROWS) {
    return n > 0 && m >= 1 && m <= PS_NA && h0 >= 1 && h0 <= max_hidden && h1 >= 1 && h1 <= max_hidden && bs >= 1 &&
           bs <= max_rows;
}

// the body of a scratch query
inline int scratch_query(int32_t n, int32_t m, int32_t h0, int32_t h1, int32_t bs, int max_hidden, int64_t need,
                         int64_t* floats, int max_rows = PS_ROWS) {
    if (!widths_ok(n, m, h0, h1, bs, max_hidden, max_rows) || !floats) return MJRL_EINVAL;
    *floats = need;
    return MJRL_OK;
}

// the checks the entry points make on what they all read; nmb > 0: the pointers too
inline bool sizes_ok(const mjrl_policy_fit_data* data, int64_t nmb, int32_t bs, int max_hidden,
                     int max_rows = PS_ROWS) {
    if (!data || nmb < 0 || data->T < 0) return false;
    // n <= 2^24: the kernels index a tensor's elements with 32 bits
    return widths_ok(data->n, data->m, data->h0, data->h1, bs, max_hidden, max_rows) && data->n <= (1 << 24);
}

inline bool pointers_ok(const mjrl_policy_fit_data* data, const int64_t* idx, const void* net, const mjrl_adam* hp,
                        const float* scratch) {
    if (!idx || !net || !hp || !scratch || hp->step0 < 0) return false;
    return data->obs && data->act && data->in_shift && data->in_scale && data->out_shift && data->out_scale;
}

// An entry point's checks, then everything of the argument block that does not change from
// launch to launch: the net's pointers, the head (MSE: data's adv / ll_old / old_log_std / kind /
// clip are not read), the rows, the sizes with d, the 16-byte-load flags, Adam's step-independent
// part.  MJRL_OK with nmb == 0: nothing was filled and nothing is to run.
template <bool MSE, class Net>
inline int step_args(StepArgs& a, const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb,
                     int32_t bs, const Net* net, const mjrl_adam* hp, float* scratch, int64_t scap, int max_hidden,
                     int max_rows = PS_ROWS) {
    if (!sizes_ok(data, nmb, bs, max_hidden, max_rows)) return MJRL_EINVAL;
    const bool ppo = !MSE && data->kind == MJRL_POLICY_FIT_PPO;
    if (!MSE && data->kind != MJRL_POLICY_FIT_BC && !ppo) return MJRL_EINVAL;
    if (ppo && (!data->ll_old == !data->old_log_std)) return MJRL_EINVAL;
    if (nmb == 0) return MJRL_OK;
    if (!pointers_ok(data, idx, net, hp, scratch)) return MJRL_EINVAL;
    if (ppo && !data->adv) return MJRL_EINVAL;
    constexpr int NT = MSE ? 6 : 7;
    float *p[NT], *m[NT], *v[NT];
    if (!net_ptrs(net, p, m, v)) return MJRL_EINVAL;
    a.p[6] = a.m[6] = a.v[6] = nullptr;   // MSE: no log_std in the net, and the MSE kernels never touch these
    for (int i = 0; i < NT; ++i) {
        a.p[i] = p[i];
        a.m[i] = m[i];
        a.v[i] = v[i];
    }
    a.adv = MSE ? nullptr : data->adv;
    a.ll_old = ppo ? data->ll_old : nullptr;
    a.old_ls = ppo ? data->old_log_std : nullptr;
    a.kind = ppo ? PF_PPO : PF_BC;
    a.clip_lo = MSE ? 1.f : (float)(1.0 - data->clip);
    a.clip_hi = MSE ? 1.f : (float)(1.0 + data->clip);
    const int n = data->n, na = data->m, h0 = data->h0, h1 = data->h1;
    a.obs = data->obs;
    a.act = data->act;
    a.in_shift = data->in_shift;
    a.in_scale = data->in_scale;
    a.out_shift = data->out_shift;
    a.out_scale = data->out_scale;
    a.idx = idx;
    a.T = data->T;
    a.scratch = scratch;
    a.scap = scap;
    a.grad = a.loss = nullptr;
    a.n = n;
    a.na = na;
    a.h0 = h0;
    a.h1 = h1;
    a.bs = bs;
    a.d = grad_at(n, na, h0, h1, MSE).d;
    const auto al16 = [](const void* q) { return (uintptr_t)q % 16 == 0; };
    a.vx = n % 4 == 0 && al16(data->obs) && al16(data->in_shift) && al16(data->in_scale);
    a.vw0 = n % 4 == 0 && al16(a.p[0]);
    a.vw1 = h0 % 4 == 0 && al16(a.p[2]);
    a.vw2 = h1 % 4 == 0 && al16(a.p[4]);
    a.hp = adam_consts(hp);
    return MJRL_OK;
}

}  // namespace mjrl
