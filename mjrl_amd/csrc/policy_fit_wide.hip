// policy_fit_wide.hip — policy_fit.hip's minibatch Adam step (phases 1-9 of its header comment)
// for hidden layers up to 256 units wide, sliced over workgroups (fit_backend = "hip_wide";
// mjrl_policy_fit_wide_epoch, mjrl_policy_mse_wide_epoch).  The policy, the masking of rows, the
// heads and every piece these kernels share with k_pfit are policy_step.h's.
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
//       4 - 7 and layer 2's part of 9).
// a0 is double-buffered: a fused k_wide_l0 launch writes step k's a0 while the launches around
// it still read step k - 1's.  An epoch is l0<F> l1<F>, then head l0<U,F> l1<U,F> per step,
// the last pair <U> alone, so a call leaves nothing behind but the loss.
//
// Arithmetic: policy_fit.hip's contract (exact-f32 MFMA, one accumulator per output tile, k
// ascending, every sum in one fixed order, no atomic, fit.h's Adam).  UPDATE and FORWARD are
// run-time flags of one code object, so the same state and arguments give the same bits however
// a run is split into calls.  The rows of gmu, g1 and g0 of a masked row are 0.
#include "policy_step.h"

using namespace mjrl;

namespace {

constexpr int WR = PS_ROWS;            // padded minibatch rows
constexpr int WH = 256;                // largest hidden width
constexpr int WM = PS_NA;              // largest action width
constexpr int WP = WH;                 // row pitch of the tiles in the scratch
constexpr int WTILE = WR * WP;         // floats of one of them
constexpr int TLD = WH + 4;            // LDS row pitch of a [64][256] tile: rows 4 banks apart
constexpr int ZLD = WM + 4;            // of the [64][64] z / gmu tile
constexpr int XCW = PS_XCW;            // columns of the X tile held in LDS at a time (pitch TLD)
constexpr int WT = PS_THREADS;         // threads of every workgroup
constexpr int WW = WT / 64;            // waves
constexpr int A1_OFF = 2 * WTILE, G1_OFF = 3 * WTILE, LOSS_OFF = 4 * WTILE;
constexpr int64_t W_SCRATCH = 4 * (int64_t)WTILE + 64;

// StepArgs: idx is the call's first minibatch, grad / loss and hp those of the step this launch updates
struct WideArgs : StepArgs {
    int64_t kU, kF;                   // minibatch of the update half / of the forward half and the head
    int update, forward;
};

// float offset of step k's a0 in the scratch
__device__ __forceinline__ int a0_off(int64_t k) { return (k & 1) ? WTILE : 0; }

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
            floatx4 acc[1] = {zero4()};
            chain_bwd_prod<TLD, 1>(acc, Ts, w, W1, h1, h0, col, UB1, r, q);
            const float* const a0u = a.scratch + a0_off(a.kU);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = 16 * w + 4 * q + k;
                float gv = 0.f;
                if (col < h0) {
                    MJRL_SLAB_CHECK(a0_off(a.kU) + row * WP + col, a.scap);
                    const float av = a0u[row * WP + col];
                    gv = acc[0][k] * (1.f - av * av);
                }
                gs[row * 16 + r] = gv;
            }
        }
        // dW0 / db0 of the units 16 u .. + 15 and Adam, one 16-column block of [xhat, 1] a job
        const int64_t o_b0 = grad_at(n, a.na, h0, h1, false).b0;
        const int cb0 = n / 16 + 1, nchunk = n / XCW + 1;   // the column of ones (col n) counts
        for (int c = 0; c < nchunk; ++c) {
            __syncthreads();   // the products before have read Ts (and written gs)
            if (n > c * XCW) {   // (a chunk holding only the column of ones needs no tile)
                stage_x<TLD>(a, n, s_ru, Ts, c, tid);
                __syncthreads();
            }
            const int nb0 = cb0 - c * (XCW / 16) < XCW / 16 ? cb0 - c * (XCW / 16) : XCW / 16;
            for (int j = w; j < nb0; j += WW)
                wgrad_job(a, a.hp, a.grad, 0, h0, n, u, c * XCW + 16 * j, gs, 16, 0, Ts, TLD, c * XCW, 0, o_b0, r, q);
        }
    }

    if (a.forward) {
        __syncthreads();   // W0 / b0 as this workgroup's waves have just written them; Ts is free; s_rf
        floatx4 acc[1] = {zero4()};   // rows 16 w .. + 15 by wave w < 4
        chain_fwd_x<TLD, 1>(
            acc, Ts, w < 4, w, W0, h0, n, u, a.vw0, r, q, [&](int c) { stage_x<TLD>(a, n, s_rf, Ts, c, tid); },
            [](int) {});
        if (w < 4) {
            const int col = 16 * u + r;
            const float bias = col < h0 ? b0[col] : 0.f;
            float* const a0f = a.scratch + a0_off(a.kF);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = 16 * w + 4 * q + k;
                MJRL_SLAB_CHECK(a0_off(a.kF) + row * WP + col, a.scap);
                a0f[row * WP + col] = col < h0 ? tanhf(acc[0][k] + bias) : 0.f;
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
        const GradAt o = grad_at(n, a.na, h0, h1, false);
        const int CB1 = h0 / 16 + 1;   // column blocks of [a0, 1]
        for (int j = w; j < CB1; j += WW)
            wgrad_job(a, a.hp, a.grad, 2, h1, h0, u, 16 * j, gs, 16, 0, As, TLD, 0, o.W1, o.b1, r, q);
    }

    if (a.forward) {
        if (a.update) __syncthreads();   // W1 / b1 as this workgroup's waves have just written them; As is free
        stage_tile(a, a0_off(a.kF), 16 * UB0, As, tid);
        __syncthreads();
        if (w < 4) {
            floatx4 acc[1] = {zero4()};
            chain_fwd<TLD, 1>(acc, As, w, W1, h1, h0, u, 0, UB0, a.vw1, r, q);
            const int col = 16 * u + r;
            const float bias = col < h1 ? b1[col] : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = 16 * w + 4 * q + k;
                MJRL_SLAB_CHECK(A1_OFF + row * WP + col, a.scap);
                a.scratch[A1_OFF + row * WP + col] = col < h1 ? tanhf(acc[0][k] + bias) : 0.f;
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
    const int m = a.na, h1 = a.h1;
    const int UB1 = (h1 + 15) / 16, UB2 = (m + 15) / 16, MP = 16 * UB2;
    const bool aliased = a.kind == PF_PPO && a.old_ls != nullptr;
    const float* const W2 = a.p[4];
    const GradAt o = grad_at(a.n, m, a.h0, h1, MSE);
    const int ub = w & 3, rb0 = 2 * (w >> 2);   // mu: wave w owns unit block w & 3, row blocks 2 (w >> 2), + 1

    // ---- 1: the row indices, the per-column constants; a1 into LDS ----
    if (w == 0)
        s_row[lane] = mb_row(a, a.kF, lane);
    else if (w == 1)
        head_consts<MSE>(a, aliased, lane, s_sig, s_gsc, s_q, s_lsum);
    stage_tile(a, A1_OFF, 16 * UB1, a1s, tid);
    __syncthreads();

    // ---- 4: mu = (a1 W2^T + b2) out_scale + out_shift, z = (act - mu) / sigma ----
    if (ub < UB2) {
        floatx4 acc[2] = {zero4(), zero4()};
        chain_fwd<TLD, 2>(acc, a1s, rb0, W2, m, h1, ub, 0, UB1, a.vw2, r, q);
        head_z<MSE, ZLD>(a, acc, ub, rb0, r, q, s_sig, s_row, zs);
    }
    __syncthreads();

    // ---- 5: per row LL, the loss head, dL/dLL ----
    head_rows<MSE, ZLD>(a, aliased, tid, zs, s_q, s_lsum, s_row, s_gll, s_lossd);
    __syncthreads();

    // ---- 6: d log_std (wave 0), the step's loss (wave 1); then gmu in place of z ----
    const float dls = head_sums<MSE, ZLD>(a, w, lane, zs, s_gll, s_lossd, LOSS_OFF, a.loss);
    __syncthreads();
    head_gmu<ZLD>(zs, s_gll, s_gsc, MP, tid);
    __syncthreads();

    // ---- 7: g1 = (gmu W2) o (1 - a1^2) for the next launches: wave w the unit blocks w, w + 8 ----
    for (int ubb = w; ubb < UB1; ubb += WW) {
        floatx4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
        const int col = 16 * ubb + r;
        chain_bwd_prod<ZLD, 4>(acc, zs, 0, W2, m, h1, col, UB2, r, q);
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
    if (!MSE && w == 0 && lane < m) log_std_adam(a, a.hp, dls, lane, a.grad, o.ls);
    const int CB2 = h1 / 16 + 1;   // column blocks of [a1, 1]
    for (int j = w; j < UB2 * CB2; j += WW)
        wgrad_job(a, a.hp, a.grad, 4, m, h1, j / CB2, 16 * (j % CB2), zs, ZLD, 16 * (j / CB2), a1s, TLD, 0, o.W2, o.b2,
                  r, q);
}

// An entry point: policy_step.h's checks and argument filling, then the launches of nmb steps.
template <bool MSE, class Net>
int run_wide(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs, const Net* net,
             const mjrl_adam* hp, float* scratch, float* grad_out, float* loss_out, void* stream) {
    WideArgs a;
    const int rc = step_args<MSE>(a, data, idx, nmb, bs, net, hp, scratch, W_SCRATCH, WH);
    if (rc != MJRL_OK || nmb == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g0((a.h0 + 15) / 16), g1((a.h1 + 15) / 16), blk(WT);
    a.kU = a.kF = 0;
    a.update = 0;
    a.forward = 1;
    hipLaunchKernelGGL(k_wide_l0, g0, blk, 0, st, a);
    hipLaunchKernelGGL(k_wide_l1, g1, blk, 0, st, a);
    for (int64_t k = 0; k < nmb; ++k) {
        adam_bias(hp, k, a.hp.step_size, a.hp.bc2s);
        a.grad = grad_out ? grad_out + k * a.d : nullptr;
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

}  // namespace

extern "C" {

int mjrl_policy_fit_wide_scratch(int32_t n, int32_t m, int32_t h0, int32_t h1, int32_t bs, int64_t* floats) {
    return scratch_query(n, m, h0, h1, bs, WH, W_SCRATCH, floats);
}

int mjrl_policy_fit_wide_epoch(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
                               const mjrl_policy_net* net, const mjrl_adam* hp, float* scratch, float* grad_out,
                               float* loss_out, void* stream) {
    return run_wide<false>(data, idx, nmb, bs, net, hp, scratch, grad_out, loss_out, stream);
}

int mjrl_policy_mse_wide_epoch(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
                               const mjrl_mean_net* net, const mjrl_adam* hp, float* scratch, float* grad_out,
                               float* loss_out, void* stream) {
    return run_wide<true>(data, idx, nmb, bs, net, hp, scratch, grad_out, loss_out, stream);
}

}  // extern "C"
