// value_fit.hip — MLPBaseline's minibatch Adam steps as hand-written kernels
// (mjrl/baselines/mlp_baseline.py:83-96).
//
// The network is Linear(F, 128) - ReLU - Linear(128, 128) - ReLU - Linear(128, 1),
// F = n + 4, the loss the MSE of a minibatch of bs <= 64 rows drawn through a
// permutation.  One step is two launches on one stream, and every dependency
// between steps and between layers is a kernel boundary: no workgroup waits for
// another inside a launch (no grid barrier, no flag, no spin loop).
//
//   k_vfit_slice<UPDATE, FORWARD>   grid 8, 8 waves.  Workgroup u owns hidden units
//       16u .. 16u + 15 of both hidden layers (rows of W0, b0, W1, b1 and their
//       Adam moments).  UPDATE: from the previous chain launch's g0, g1 and the
//       a0 they were computed from, dW0 = g0^T X, db0 = colsum g0, dW1 = g1^T a0,
//       db1 = colsum g1 of its units (the bias sums ride along as a column of
//       ones), then Adam on exactly those elements.  FORWARD: its 16 columns of
//       a0 = relu(X W0^T + b0) for the next minibatch, with the rows of W0 it has
//       just updated.
//   k_vfit_chain                    one workgroup, 8 waves.  a1 = relu(a0 W1^T + b1),
//       out = a1 W2^T + b2, dout = 2 (out - y) / bs, g1 = (dout W2) o [a1 > 0],
//       g0 = (g1 W1) o [a0 > 0], dW2, db2, Adam on W2 / b2 (after their use), the
//       step's loss.
//
// An epoch of nmb steps: slice<F>, chain, slice<U, F>, chain, ..., slice<U>.
//
// A launch starts with cold caches (the eight slices run on eight XCDs, each with
// its own L2) and a round trip to memory costs about as much as all of a slice's
// arithmetic, so the slice kernel is laid out by dependent round trips, not by
// flops: the row indices first, then everything else it will read in one burst
// (the gathered X tile, a0, g0 / g1 into LDS; the forward half's X fragments and
// the parameters and moments of every element it will update into registers),
// then the products out of LDS and registers.
//
// Arithmetic: the matrix products are v_mfma_f32_16x16x4_f32 (exact f32, a
// k-ordered fma chain; the forward products split k over accumulators and over
// two waves whose partial sums are added in one fixed order), the k dimension
// zero-padded in the loads, not in memory.  Every sum has one order, there is no
// atomic, so a run is a function of its inputs, bit for bit.  The minibatch is
// padded to 64 rows; a padded row and a row whose index is outside [0, T) are
// masked (nothing of X / Y is read for them, their dout is 0).
//
// Adam, the operand loaders and the tail of an update job are fit.h's, shared with
// policy_fit.hip.
#include "fit.h"

using namespace mjrl;

namespace {

constexpr int VH = 128;               // hidden width (the reference's)
constexpr int VR = 64;                // padded minibatch rows
constexpr int VLD = VH + 4;           // LDS row pitch of the chain's [64][128] tiles
constexpr int VTILE = VR * VH;        // floats of a0 / g0 / g1 in the scratch
// scratch: a0 of even steps, g0, g1, the last step's loss (and padding), a0 of odd steps.  a0 is
// double-buffered because a fused slice launch reads all of step k's a0 in every workgroup
// while each workgroup writes its columns of step k + 1's.
constexpr int64_t VSCRATCH = 4 * (int64_t)VTILE + 64;
constexpr int A0_ODD = 3 * VTILE + 64;
constexpr int SLICE_THREADS = 512, CHAIN_THREADS = 512;
constexpr int SW = SLICE_THREADS / 64;        // waves of a slice workgroup
constexpr int XCW = 384;              // columns of the gathered X tile held in LDS at a time
constexpr int XLD = XCW + 16;         // its row pitch; = 16 mod 64: the four rows of an MFMA operand
constexpr int ALD = VH + 16;          //   read land 16 banks apart.  a0's pitch likewise
constexpr int JW = (XCW / 16 + VH / 16 + 1 + SW - 1) / SW;   // update jobs of a wave per X chunk
constexpr int TPR = SLICE_THREADS / VR;       // threads staging one row of the X tile
constexpr int KS = SW / 4;            // forward half: waves splitting k (times four row blocks)
constexpr int FG = XCW / 16 / KS;     // forward k groups of a wave per 384 columns

struct VfitArgs {
    const float* X;
    const float* Y;
    int64_t T;
    const int64_t* perm;
    float* p[6];                      // W0, b0, W1, b1, W2, b2 (torch order)
    float* m[6];
    float* v[6];
    float* scratch;                   // see VSCRATCH
    int64_t scap;                     // floats of scratch (debug build: checked)
    float* grad;                      // null or the update step's [d] gradient
    float* loss;                      // null or the step's loss slot
    int64_t kU, kF;                   // minibatch of the update half / of the forward half
    int F, bs, vec;                   // vec: 16-byte loads of X / W0 rows allowed
    AdamK hp;
};

// float offset of step k's a0 in the scratch
__device__ __forceinline__ int a0_off(int64_t k) { return (k & 1) ? A0_ODD : 0; }

// row index of minibatch k's row r, or -1 for a masked row
__device__ __forceinline__ int64_t mb_row(const VfitArgs& a, int64_t k, int r) {
    if (r >= a.bs) return -1;
    const int64_t i = a.perm[k * a.bs + r];
    return i >= 0 && i < a.T ? i : -1;
}

// An update job: one 16-column block of [X, 1] (layer 0) or of [a0, 1] (layer 1) for
// this workgroup's 16 units.  A lane's accumulator register i belongs to the weight
// [unit 4 q + i][col] (col < K), to that unit's bias (col == K, the column of ones) or
// to nothing.  The tensors are wave-uniform and the element offsets 32-bit, so every
// access is a scalar base plus a lane offset (no per-element 64-bit addresses to hold).
struct Job {
    float *pw, *mw, *vw, *pb, *mb, *vb;   // weight and bias tensors, their moments
    int64_t gw, gb;                       // their places in the flat gradient
    int K, col;                           // the layer's input width, this lane's column
};
__device__ __forceinline__ Job make_job(const VfitArgs& a, bool l0, int col) {
    const int64_t gb0 = (int64_t)VH * a.F, gW1 = gb0 + VH, gb1 = gW1 + (int64_t)VH * VH;
    const int w = l0 ? 0 : 2;
    return Job{a.p[w], a.m[w], a.v[w], a.p[w + 1], a.m[w + 1], a.v[w + 1], l0 ? 0 : gW1, l0 ? gb0 : gb1,
               l0 ? a.F : VH, col};
}

template <bool UPDATE, bool FORWARD>
__global__ void __launch_bounds__(SLICE_THREADS) k_vfit_slice(VfitArgs a) {
    __shared__ int64_t s_ru[VR], s_rf[VR];
    // UPDATE: the gathered X tile (one chunk of columns); FORWARD, after it: the k-split partials
    __shared__ __attribute__((aligned(16))) float Xs[UPDATE ? VR * XLD : KS * VR * 16];
    __shared__ __attribute__((aligned(16))) float a0s[UPDATE ? VR * ALD : 4];
    __shared__ float gs[UPDATE ? 2 * VR * 16 : 2];   // this workgroup's columns of g0, then of g1
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int u = blockIdx.x, F = a.F;
    const bool vec = a.vec != 0;
    const float* const a0u = a.scratch + a0_off(a.kU);   // the update half's a0 (read)
    float* const a0f = a.scratch + a0_off(a.kF);         // the forward half's (written)
    const float* const g0 = a.scratch + VTILE;
    const float* const g1 = a.scratch + 2 * VTILE;

    // ---- round trip 1: the row indices ----
    if (tid < VR) {
        if (UPDATE) s_ru[tid] = mb_row(a, a.kU, tid);
    } else if (tid < 2 * VR) {
        if (FORWARD) s_rf[tid - VR] = mb_row(a, a.kF, tid - VR);
    }
    __syncthreads();

    // forward half: wave (frb, fkq) multiplies rows 16 frb .. + 15 by the k groups fkq, fkq + KS, ...
    const int frb = w & 3, fkq = w >> 2, ng = (F + 15) / 16;
    const int64_t fxi = FORWARD ? s_rf[16 * frb + r] : -1;
    const float* const fxrow = a.X + (fxi >= 0 ? fxi : 0) * F;
    float4 fx[FG];
    auto load_fx = [&](int gbase) {
#pragma unroll
        for (int i = 0; i < FG; ++i) fx[i] = float4{0.f, 0.f, 0.f, 0.f};
        if (fxi >= 0) {   // nothing of X is read for a masked row
#pragma unroll
            for (int i = 0; i < FG; ++i) {
                const int g = gbase + fkq + KS * i;
                if (g < ng) fx[i] = ld4(fxrow, 16 * g + 4 * q, F, vec);   // wave-uniform
            }
        }
    };

    if (UPDATE) {
        // layer 0's 16-column blocks of [X, 1] (the last holds the column of ones), 24 per X chunk
        const int cb0 = F / 16 + 1, nchunk = (cb0 + XCW / 16 - 1) / (XCW / 16);
        for (int c = 0; c < nchunk; ++c) {
            const int c0 = c * XCW, cw = F - c0 < XCW ? (F - c0 > 0 ? F - c0 : 0) : XCW;
            const int nb0 = cb0 - c * (XCW / 16) < XCW / 16 ? cb0 - c * (XCW / 16) : XCW / 16;
            const int nj = nb0 + (c == 0 ? VH / 16 + 1 : 0);   // chunk 0 carries layer 1's blocks of [a0, 1] too
            if (c > 0) __syncthreads();                         // the previous chunk's products have read Xs

            // ---- round trip 2: everything this chunk reads, in one burst ----
            // this thread's share of the X tile: row tid / TPR, 16-byte words TPR apart (one
            // address, constant offsets)
            constexpr int XN = XCW / TPR;
            const int xr = tid / TPR, xc = tid % TPR;
            const int64_t xi = s_ru[xr];
            const float* const xrow = a.X + (xi >= 0 ? xi : 0) * F + c0;
            float4 xb[XN / 4];
            const int cw4 = cw / 4;
            if (vec) {
#pragma unroll
                for (int i = 0; i < XN / 4; ++i) xb[i] = float4{0.f, 0.f, 0.f, 0.f};
                if (xi >= 0 && cw4 > 0) {
#pragma unroll
                    for (int i = 0; i < XN / 4; ++i) {
                        const int c4 = xc + TPR * i;
                        xb[i] = *reinterpret_cast<const float4*>(xrow + 4 * (c4 < cw4 ? c4 : cw4 - 1));
                    }
                }
            } else {
                // rows that allow no 16-byte loads: single columns straight into LDS (a
                // round trip of their own ahead of the burst)
#pragma unroll 8
                for (int i = 0; i < XN; ++i) {
                    const int col = xc + TPR * i;
                    Xs[xr * XLD + col] = xi >= 0 && col < cw ? xrow[col] : 0.f;
                }
            }
            constexpr int AN = VTILE / 4 / SLICE_THREADS, GN = VR * 16 / SLICE_THREADS;
            float4 at[AN];
            float gt[2][GN];
            if (c == 0) {
#pragma unroll
                for (int i = 0; i < AN; ++i) {
                    const int e = tid + SLICE_THREADS * i;
                    MJRL_SLAB_CHECK(a0_off(a.kU) + 4 * e + 3, a.scap);
                    at[i] = *reinterpret_cast<const float4*>(a0u + 4 * e);
                }
#pragma unroll
                for (int i = 0; i < GN; ++i) {
                    const int e = tid + SLICE_THREADS * i, ge = (e >> 4) * VH + 16 * u + (e & 15);
                    MJRL_SLAB_CHECK(2 * VTILE + ge, a.scap);
                    gt[0][i] = g0[ge];
                    gt[1][i] = g1[ge];
                }
            }
            // the parameters and moments of this wave's jobs w, w + SW, ...: every lane loads the
            // weight of its (clamped) column; the block holding the column of ones loads the
            // biases too (wave-uniform) and the lane of that column keeps them
            float pm[JW][4][3];
#pragma unroll
            for (int jj = 0; jj < JW; ++jj) {
                const int j = w + SW * jj;
                if (j >= nj) continue;
                const bool l0 = j < nb0;
                const int blk = l0 ? c * (XCW / 16) + j : j - nb0;
                const Job jb = make_job(a, l0, blk * 16 + r);
                const int colc = jb.col < jb.K ? jb.col : jb.K - 1;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned unit = 16 * u + 4 * q + i, e = unit * jb.K + colc;
                    pm[jj][i][0] = jb.pw[e];
                    pm[jj][i][1] = jb.mw[e];
                    pm[jj][i][2] = jb.vw[e];
                }
                if (blk == jb.K / 16) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned unit = 16 * u + 4 * q + i;
                        const float pb = jb.pb[unit], mb = jb.mb[unit], vb = jb.vb[unit];
                        const bool ones = jb.col == jb.K;
                        pm[jj][i][0] = ones ? pb : pm[jj][i][0];
                        pm[jj][i][1] = ones ? mb : pm[jj][i][1];
                        pm[jj][i][2] = ones ? vb : pm[jj][i][2];
                    }
                }
            }
            if (vec) {
#pragma unroll
                for (int i = 0; i < XN / 4; ++i) {
                    const int c4 = xc + TPR * i;
                    *reinterpret_cast<float4*>(Xs + xr * XLD + 4 * c4) = c4 < cw4 ? xb[i] : float4{0.f, 0.f, 0.f, 0.f};
                }
            }
            if (c == 0) {
#pragma unroll
                for (int i = 0; i < AN; ++i) {
                    const int e = tid + SLICE_THREADS * i;
                    *reinterpret_cast<float4*>(a0s + (e / (VH / 4)) * ALD + 4 * (e % (VH / 4))) = at[i];
                }
#pragma unroll
                for (int i = 0; i < GN; ++i) {
                    gs[tid + SLICE_THREADS * i] = gt[0][i];
                    gs[VR * 16 + tid + SLICE_THREADS * i] = gt[1][i];
                }
            }
            __syncthreads();
            // the forward half's X fragments arrive behind the products below (issued
            // here, not in the burst: the tile's staging registers are free again)
            if (FORWARD && c == 0) load_fx(0);

            // ---- the products out of LDS, Adam on the loaded elements ----
#pragma unroll
            for (int jj = 0; jj < JW; ++jj) {
                const int j = w + SW * jj;
                if (j >= nj) continue;
                __builtin_amdgcn_sched_barrier(0);   // one job's operands in registers at a time
                const bool l0 = j < nb0;
                const Job jb = make_job(a, l0, (l0 ? c * (XCW / 16) + j : j - nb0) * 16 + r);
                const int K = jb.K, col = jb.col;   // col: of [X, 1] / [a0, 1]
                const int colc = col < K ? col : K - 1;
                const float* const gl = gs + (l0 ? 0 : VR * 16);
                const float* const bl = l0 ? Xs + (colc - c0) : a0s + colc;
                const int bld = l0 ? XLD : ALD;
                floatx4 acc[2] = {zero4(), zero4()};
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int row = 4 * s + q;
                    const float ones = s_ru[row] >= 0 ? 1.f : 0.f;
                    const float b = bl[row * bld];
                    acc[s & 1] = mfma4(gl[row * 16 + r], col < K ? b : (col == K ? ones : 0.f), acc[s & 1]);
                }
                if (col <= K) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned unit = 16 * u + 4 * q + i;
                        wgrad_tail(pm[jj][i], acc[0][i] + acc[1][i], unit, K, col, a.hp, jb.pw, jb.mw, jb.vw, jb.pb, jb.mb,
                                   jb.vb, a.grad, jb.gw, jb.gb);
                    }
                }
            }
        }
        if (FORWARD) __syncthreads();   // W0 / b0 as this workgroup's waves have just written them; Xs is free
    } else {
        load_fx(0);
    }

    if (FORWARD) {
        const float* const wrow = a.p[0] + (int64_t)(16 * u + r) * F;
        floatx4 acc[2] = {zero4(), zero4()};
        for (int gbase = 0; gbase < ng; gbase += KS * FG) {
            if (gbase > 0) load_fx(gbase);
            float4 wb[FG];
#pragma unroll
            for (int i = 0; i < FG; ++i) {
                const int g = gbase + fkq + KS * i;
                wb[i] = float4{0.f, 0.f, 0.f, 0.f};
                if (g < ng) wb[i] = ld4(wrow, 16 * g + 4 * q, F, vec);   // wave-uniform
            }
#pragma unroll
            for (int i = 0; i < FG; ++i) acc[i & 1] = mfma_k16(fx[i], wb[i], acc[i & 1]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) Xs[(fkq * VR + 16 * frb + 4 * q + i) * 16 + r] = acc[0][i] + acc[1][i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < VR * 16 / SLICE_THREADS; ++i) {
            const int e = tid + SLICE_THREADS * i, row = e >> 4, cu = e & 15;
            float pre = Xs[e];
#pragma unroll
            for (int k = 1; k < KS; ++k) pre += Xs[k * VR * 16 + e];
            pre += a.p[1][16 * u + cu];
            MJRL_SLAB_CHECK(a0_off(a.kF) + row * VH + 16 * u + cu, a.scap);
            a0f[row * VH + 16 * u + cu] = s_rf[row] >= 0 && pre > 0.f ? pre : 0.f;
        }
    }
}

__global__ void __launch_bounds__(CHAIN_THREADS) k_vfit_chain(VfitArgs a) {
    __shared__ __attribute__((aligned(16))) float a0s[VR * VLD];
    __shared__ __attribute__((aligned(16))) float a1s[VR * VLD];
    __shared__ __attribute__((aligned(16))) float g1s[VR * VLD];
    __shared__ float w2s[VH], douts[VR], ys[VR];
    __shared__ double sq[VR];
    __shared__ int valid[VR];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const float* const a0 = a.scratch + a0_off(a.kF);
    float* const g0 = a.scratch + VTILE;
    float* const g1 = a.scratch + 2 * VTILE;
    const float* const W1 = a.p[2];

    // ---- stage a0, W2, the targets; W2 / b2's moments for the Adam step below ----
    const int64_t xi = tid < VR ? mb_row(a, a.kF, tid) : -1;
    for (int e = tid; e < VTILE / 4; e += CHAIN_THREADS) {
        const int row = e / (VH / 4), c4 = e % (VH / 4);
        MJRL_SLAB_CHECK(a0_off(a.kF) + e * 4 + 3, a.scap);
        *reinterpret_cast<float4*>(a0s + row * VLD + 4 * c4) = *reinterpret_cast<const float4*>(a0 + e * 4);
    }
    float p2 = 0.f, m2 = 0.f, v2 = 0.f;   // thread t < 128: W2[t]; thread 128: b2
    if (tid <= VH) {
        const int t = tid < VH ? 4 : 5, e = tid < VH ? tid : 0;
        p2 = a.p[t][e];
        m2 = a.m[t][e];
        v2 = a.v[t][e];
    }
    const float b2 = a.p[5][0];
    if (tid < VH) w2s[tid] = p2;
    const float yv = xi >= 0 ? a.Y[xi] : 0.f;   // stored behind the first product: its round trip hides there
    if (tid < VR) valid[tid] = xi >= 0;
    __syncthreads();

    // ---- a1 = relu(a0 W1^T + b1): wave w the columns 16 w .. 16 w + 15, all 64 rows ----
    {
        floatx4 acc[4][1];
        zero_acc(acc);
        const int col = 16 * w + r;
        const float bias = a.p[3][col];
        gemm_tile<4, 1>(acc, a0s, VLD, 0, 0, 1, 4, W1, VH, w, 8, 0, VH, lane);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float pre = acc[rb][0][i] + bias;
                a1s[(16 * rb + 4 * q + i) * VLD + col] = pre > 0.f ? pre : 0.f;
            }
    }
    if (tid < VR) ys[tid] = yv;
    __syncthreads();

    // ---- out = a1 W2^T + b2, dout = 2 (out - y) / bs: 8 lanes per row, 16 columns each ----
    {
        const int row = tid >> 3, part = tid & 7;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) s += a1s[row * VLD + 16 * part + j] * w2s[16 * part + j];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (part == 0) {
            const float d = valid[row] ? (s + b2) - ys[row] : 0.f;
            douts[row] = 2.f * d / (float)a.bs;
            sq[row] = (double)d * (double)d;
        }
    }
    __syncthreads();

    // ---- loss, g1 = (dout W2) o [a1 > 0], dW2, db2, Adam on W2 / b2 ----
    if (w == 7) {
        const double tot = wave_sum(sq[lane]) / (double)a.bs;
        if (lane == 0) {
            MJRL_SLAB_CHECK(3 * VTILE, a.scap);
            a.scratch[3 * VTILE] = (float)tot;
            if (a.loss) *a.loss = (float)tot;
        }
    }
    for (int e = tid; e < VTILE; e += CHAIN_THREADS) {
        const int row = e / VH, col = e % VH;
        const float g = a1s[row * VLD + col] > 0.f ? douts[row] * w2s[col] : 0.f;
        g1s[row * VLD + col] = g;
        MJRL_SLAB_CHECK(2 * VTILE + e, a.scap);
        g1[e] = g;
    }
    if (tid <= VH) {
        const int64_t gW2 = (int64_t)VH * a.F + VH + (int64_t)VH * VH + VH;
        float s = 0.f;
        if (tid < VH)
            for (int row = 0; row < VR; ++row) s += douts[row] * a1s[row * VLD + tid];
        else
            for (int row = 0; row < VR; ++row) s += douts[row];
        if (a.grad) a.grad[gW2 + tid] = s;
        const int t = tid < VH ? 4 : 5, e = tid < VH ? tid : 0;
        float p1, m1, v1;
        adam_step(p2, m2, v2, s, a.hp, p1, m1, v1);
        a.p[t][e] = p1;
        a.m[t][e] = m1;
        a.v[t][e] = v1;
    }
    __syncthreads();

    // ---- g0 = (g1 W1) o [a0 > 0]: wave w the columns 16 w .. 16 w + 15 ----
    {
        floatx4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
        const int col = 16 * w + r;
#pragma unroll 4
        for (int g = 0; g < VH / 16; ++g) {
            const int j = 16 * g + 4 * q;
            float4 b;
            b.x = W1[(j + 0) * VH + col];
            b.y = W1[(j + 1) * VH + col];
            b.z = W1[(j + 2) * VH + col];
            b.w = W1[(j + 3) * VH + col];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const float4 av = *reinterpret_cast<const float4*>(g1s + (16 * rb + r) * VLD + j);
                acc[rb] = mfma_k16(av, b, acc[rb]);
            }
        }
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 16 * rb + 4 * q + i;
                MJRL_SLAB_CHECK(VTILE + row * VH + col, a.scap);
                g0[row * VH + col] = a0s[row * VLD + col] > 0.f ? acc[rb][i] : 0.f;
            }
    }
}

}  // namespace

extern "C" {

int mjrl_value_mlp_scratch(int32_t n, int32_t bs, int64_t* floats) {
    if (n <= 0 || bs < 1 || bs > VR || !floats) return MJRL_EINVAL;
    *floats = VSCRATCH;
    return MJRL_OK;
}

int mjrl_value_mlp_epoch(const float* X, const float* Y, int64_t T, int32_t n, const int64_t* perm, int64_t nmb,
                         int32_t bs, const mjrl_value_net* net, const mjrl_adam* hp, float* scratch, float* grad_out,
                         float* loss_out, void* stream) {
    // n <= 2^24: the kernels index a tensor's elements with 32 bits
    if (n <= 0 || n > (1 << 24) || bs < 1 || bs > VR || T < 0 || nmb < 0) return MJRL_EINVAL;
    if (nmb == 0) return MJRL_OK;
    if (!X || !Y || !perm || !net || !hp || !scratch || hp->step0 < 0) return MJRL_EINVAL;
    VfitArgs a;
    if (!net_ptrs(net, a.p, a.m, a.v)) return MJRL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int F = n + 4;
    const int64_t d = (int64_t)VH * F + VH + (int64_t)VH * VH + VH + VH + 1;
    a.X = X;
    a.Y = Y;
    a.T = T;
    a.perm = perm;
    a.scratch = scratch;
    a.scap = VSCRATCH;
    a.F = F;
    a.bs = bs;
    a.vec = F % 4 == 0 && ((uintptr_t)X | (uintptr_t)net->p[0]) % 16 == 0;
    a.hp = adam_consts(hp);
    a.grad = nullptr;
    a.loss = nullptr;
    a.kU = a.kF = 0;
    hipLaunchKernelGGL((k_vfit_slice<false, true>), dim3(VH / 16), dim3(SLICE_THREADS), 0, st, a);
    for (int64_t k = 0; k < nmb; ++k) {
        adam_bias(hp, k, a.hp.step_size, a.hp.bc2s);
        a.grad = grad_out ? grad_out + k * d : nullptr;
        a.loss = loss_out ? loss_out + k : nullptr;
        a.kU = a.kF = k;
        hipLaunchKernelGGL(k_vfit_chain, dim3(1), dim3(CHAIN_THREADS), 0, st, a);
        a.kF = k + 1;
        if (k + 1 < nmb)
            hipLaunchKernelGGL((k_vfit_slice<true, true>), dim3(VH / 16), dim3(SLICE_THREADS), 0, st, a);
        else
            hipLaunchKernelGGL((k_vfit_slice<true, false>), dim3(VH / 16), dim3(SLICE_THREADS), 0, st, a);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
