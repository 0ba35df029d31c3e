// policy_fit.hip — the minibatch Adam steps of PPO and BC on the Gaussian MLP policy
// as one hand-written kernel (mjrl/algos/ppo_clip.py:47-54,
// 89-95, behavior_cloning.py:39-63), for 1 <= h0, h1, m <= 64 (actual sizes: zero-padded in
// the loads, not in memory).  The policy, the masking of rows, the heads (k_pfit<true>: MSE) and
// every piece this kernel shares with policy_fit_wide.hip are policy_step.h's.
//
//   k_pfit   ONE workgroup of 8 waves owns the whole chain of steps: a launch runs up
//       to PF_SPL consecutive steps in a loop.  The steps are serially dependent, so
//       nothing waits across workgroups: no grid barrier, no flag, no spin loop, no
//       atomic, no cooperative launch.  (Measured, DESIGN.md §6: half of a Humanoid
//       step is the weight-gradient jobs with Adam, bound by one CU's instruction
//       rate; spreading them over more CUs means a kernel boundary a step.)
//       The parameters and the Adam moments stay in global memory (the device
//       optimizer's own tensors, L2-resident); __syncthreads() separates a step's
//       stores from the next step's loads (workgroup scope is enough on one CU).
//
// A step, every phase ending in a workgroup barrier (in brackets: policy_step.h's piece):
//   1  row indices (mb_row), per-column constants (head_consts)
//   2  layer 0 over column chunks of the gathered, normalised X tile (stage_x, 256 columns
//      in LDS at a time): a0 = tanh(xhat W0^T + b0)
//   3  a1 = tanh(a0 W1^T + b1)
//   4  mu = (a1 W2^T + b2) out_scale + out_shift, z = (act - mu) / sigma (head_z)
//   5  per row: LL, the loss head, dL/dLL (head_rows)
//   6  d log_std, the step's loss (head_sums); then gmu in place of z (head_gmu)
//   7  g1 = (gmu W2) o (1 - a1^2)
//   8  g0 = (g1 W1) o (1 - a0^2)
//   9  the weight gradients as 16 x 16 jobs (wgrad_job: dW2 = gmu^T [a1, 1], dW1 = g1^T [a0, 1],
//      dW0 = g0^T [xhat, 1] chunk by chunk, the last forward chunk first: it is still
//      in LDS; the bias sums ride along as a column of ones), Adam on exactly the
//      elements of each job, log_std's Adam.  Every use of a step's parameters is
//      behind a barrier before the first of these stores.
//
// Arithmetic: products on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fma chain,
// one accumulator per output tile), every sum in one fixed order, no atomic: the same
// state and arguments give the same bits, however the steps are split over launches
// and calls.  Adam is fit.h's adam_step, the bias corrections of step t formed
// on the host in f64 from t alone.
#include "policy_step.h"

using namespace mjrl;

namespace {

constexpr int PR = PS_ROWS;           // padded minibatch rows
constexpr int PH = 64;                // largest hidden / action width
constexpr int PLD = PH + 4;           // LDS row pitch of the [64][64] tiles: rows 4 banks apart
constexpr int XCW = PS_XCW;           // columns of the X tile held in LDS at a time
constexpr int XLD = XCW + 4;          // its row pitch
constexpr int PF_THREADS = PS_THREADS;
constexpr int PW = PF_THREADS / 64;   // waves
constexpr int PF_SPL = 128;           // steps of one launch at the most (their Adam constants are kernel arguments)
constexpr int64_t PF_SCRATCH = 64;    // floats: [0] the last step's loss

#ifdef MJRL_PFIT_PROF
// phase profile (profiling builds, -DMJRL_PFIT_PROF; tools/policy_fit_prof.py): thread 0 adds the
// s_memtime cycles between stamps into LDS and, at the end of a launch, into the scratch behind
// the loss slot (PF_NPROF 64-bit counters from float 8 on, zeroed by the caller)
constexpr int PF_NPROF = 14;
#define PF_STAMP(i)                                                      \
    do {                                                                 \
        if (tid == 0) {                                                  \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
            s_prof[i] += now_ - pf_last;                                 \
            pf_last = now_;                                              \
        }                                                                \
    } while (0)
#else
#define PF_STAMP(i) \
    do {            \
    } while (0)
#endif

// StepArgs: idx, grad and loss are those of the launch's first step, hp the step-independent part
struct PfitArgs : StepArgs {
    int nsteps;
    float step_size[PF_SPL], bc2s[PF_SPL];   // hp's other two fields for each step of this launch
};

// MSE: a compile-time switch, so that the BC / PPO instantiation stays the code it was
template <bool MSE>
__global__ void __launch_bounds__(PF_THREADS) k_pfit(PfitArgs a) {
    __shared__ __attribute__((aligned(16))) float Xs[PR * XLD];    // xhat, one chunk of columns
    __shared__ __attribute__((aligned(16))) float a0s[PR * PLD];
    __shared__ __attribute__((aligned(16))) float a1s[PR * PLD];
    __shared__ __attribute__((aligned(16))) float g0s[PR * PLD];
    __shared__ __attribute__((aligned(16))) float g1s[PR * PLD];
    __shared__ __attribute__((aligned(16))) float zs[PR * PLD];    // z, then gmu
    __shared__ int64_t s_row[PR];                                  // row index, -1: masked
    __shared__ double s_lossd[PR], s_q[PH], s_lsum[2];             // s_q: 1 - (sigma / sigma_old)^2
    __shared__ float s_gll[PR], s_sig[PH], s_gsc[PH];              // dL/dLL; sigma; out_scale / sigma

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
#ifdef MJRL_PFIT_PROF
    __shared__ unsigned long long s_prof[PF_NPROF];
    if (tid < PF_NPROF) s_prof[tid] = 0;
    __syncthreads();
    unsigned long long pf_last = __builtin_amdgcn_s_memtime();
#endif
    const int n = a.n, m = a.na, h0 = a.h0, h1 = a.h1;
    const int UB0 = (h0 + 15) / 16, UB1 = (h1 + 15) / 16, UB2 = (m + 15) / 16;   // unit blocks
    const int MP = 16 * UB2;
    const bool aliased = a.kind == PF_PPO && a.old_ls != nullptr;
    float *const W0 = a.p[0], *const b0 = a.p[1], *const W1 = a.p[2], *const b1 = a.p[3], *const W2 = a.p[4];
    // flat places of the seven tensors in a step's gradient
    const int64_t o_b0 = (int64_t)h0 * n, o_W1 = o_b0 + h0, o_b1 = o_W1 + (int64_t)h1 * h0, o_W2 = o_b1 + h1,
                  o_b2 = o_W2 + (int64_t)m * h1, o_ls = o_b2 + m;
    // forward / chain products: wave w owns unit block w & 3 and the row blocks 2 (w >> 2), + 1
    const int ub = w & 3, rb0 = 2 * (w >> 2);
    const int nchunk_f = (n + XCW - 1) / XCW;   // forward chunks
    const int nchunk_b = n / XCW + 1;           // backward chunks: the column of ones (col n) counts

    AdamK hp = a.hp;   // step_size / bc2s: the current step's, set below
    // a lambda capturing n: called directly, stage_x costs 69 more SGPR reloads and 0.4 % of Swimmer's epochs
    const auto load_chunk = [&](int c) { stage_x<XLD>(a, n, s_row, Xs, c, tid); };

    for (int step = 0; step < a.nsteps; ++step) {
        hp.step_size = a.step_size[step];
        hp.bc2s = a.bc2s[step];
        float* const grad = a.grad ? a.grad + (int64_t)step * a.d : nullptr;

        // ---- 1: the row indices, the per-column constants ----
        if (w == 0)
            s_row[lane] = mb_row(a, step, lane);
        else if (w == 1)
            head_consts<MSE>(a, aliased, lane, s_sig, s_gsc, s_q, s_lsum);
        __syncthreads();
        PF_STAMP(0);

        // ---- 2: a0 = tanh(xhat W0^T + b0), xhat chunk by chunk ----
        {
            floatx4 acc[2] = {zero4(), zero4()};
            for (int c = 0; c < nchunk_f; ++c) {
                if (c > 0) __syncthreads();   // the previous chunk's products have read Xs
                load_chunk(c);
                __syncthreads();
                PF_STAMP(c == 0 ? 1 : 12);
                if (ub < UB0) {
                    const int c0 = c * XCW, cw = n - c0 < XCW ? n - c0 : XCW, ng = (cw + 15) / 16;
#pragma unroll 4
                    for (int g = 0; g < ng; ++g) {
                        const float4 b = ldw4(W0, h0, n, 16 * ub + r, c0 + 16 * g + 4 * q, a.vw0);
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const float4 av =
                                *reinterpret_cast<const float4*>(Xs + (16 * (rb0 + i) + r) * XLD + 16 * g + 4 * q);
                            acc[i] = mfma_k16(av, b, acc[i]);
                        }
                    }
                }
            }
            if (ub < UB0) {
                const int col = 16 * ub + r;
                const float bias = col < h0 ? b0[col] : 0.f;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        a0s[(16 * (rb0 + i) + 4 * q + k) * PLD + col] = col < h0 ? tanhf(acc[i][k] + bias) : 0.f;
            }
        }
        __syncthreads();
        PF_STAMP(2);

        // ---- 3: a1 = tanh(a0 W1^T + b1) ----
        if (ub < UB1) {
            floatx4 acc[2] = {zero4(), zero4()};
#pragma unroll 4
            for (int g = 0; g < UB0; ++g) {
                const float4 b = ldw4(W1, h1, h0, 16 * ub + r, 16 * g + 4 * q, a.vw1);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float4 av = *reinterpret_cast<const float4*>(a0s + (16 * (rb0 + i) + r) * PLD + 16 * g + 4 * q);
                    acc[i] = mfma_k16(av, b, acc[i]);
                }
            }
            const int col = 16 * ub + r;
            const float bias = col < h1 ? b1[col] : 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    a1s[(16 * (rb0 + i) + 4 * q + k) * PLD + col] = col < h1 ? tanhf(acc[i][k] + bias) : 0.f;
        }
        __syncthreads();
        PF_STAMP(3);

        // ---- 4: mu = (a1 W2^T + b2) out_scale + out_shift, z = (act - mu) / sigma ----
        if (ub < UB2) {
            floatx4 acc[2] = {zero4(), zero4()};
#pragma unroll 4
            for (int g = 0; g < UB1; ++g) {
                const float4 b = ldw4(W2, m, h1, 16 * ub + r, 16 * g + 4 * q, a.vw2);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float4 av = *reinterpret_cast<const float4*>(a1s + (16 * (rb0 + i) + r) * PLD + 16 * g + 4 * q);
                    acc[i] = mfma_k16(av, b, acc[i]);
                }
            }
            head_z<MSE, PLD>(a, acc, ub, rb0, r, q, s_sig, s_row, zs);
        }
        __syncthreads();
        PF_STAMP(4);

        // ---- 5: per row LL, the loss head, dL/dLL ----
        head_rows<MSE, PLD>(a, aliased, tid, zs, s_q, s_lsum, s_row, s_gll, s_lossd);
        __syncthreads();
        PF_STAMP(5);

        // ---- 6: d log_std (wave 0), the step's loss (wave 1); then gmu in place of z ----
        const float dls = head_sums<MSE, PLD>(a, w, lane, zs, s_gll, s_lossd, 0, a.loss ? a.loss + step : nullptr);
        __syncthreads();
        head_gmu<PLD>(zs, s_gll, s_gsc, MP, tid);
        __syncthreads();
        PF_STAMP(6);

        // ---- 7: g1 = (gmu W2) o (1 - a1^2) ----
        if (ub < UB1) {
            floatx4 acc[2] = {zero4(), zero4()};
            const int col = 16 * ub + r;
            for (int g = 0; g < UB2; ++g) {
                const int j = 16 * g + 4 * q;
                const float4 b = ldwt4(W2, m, h1, j, col);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float4 av = *reinterpret_cast<const float4*>(zs + (16 * (rb0 + i) + r) * PLD + j);
                    acc[i] = mfma_k16(av, b, acc[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int row = 16 * (rb0 + i) + 4 * q + k;
                    const float av = a1s[row * PLD + col];
                    g1s[row * PLD + col] = col < h1 ? acc[i][k] * (1.f - av * av) : 0.f;
                }
        }
        __syncthreads();
        PF_STAMP(7);

        // ---- 8: g0 = (g1 W1) o (1 - a0^2) ----
        if (ub < UB0) {
            floatx4 acc[2] = {zero4(), zero4()};
            const int col = 16 * ub + r;
            for (int g = 0; g < UB1; ++g) {
                const int j = 16 * g + 4 * q;
                const float4 b = ldwt4(W1, h1, h0, j, col);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float4 av = *reinterpret_cast<const float4*>(g1s + (16 * (rb0 + i) + r) * PLD + j);
                    acc[i] = mfma_k16(av, b, acc[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int row = 16 * (rb0 + i) + 4 * q + k;
                    const float av = a0s[row * PLD + col];
                    g0s[row * PLD + col] = col < h0 ? acc[i][k] * (1.f - av * av) : 0.f;
                }
        }
        __syncthreads();
        PF_STAMP(8);

        // ---- 9: the weight gradients and Adam; every read of this step's parameters is behind us ----
        if (!MSE && w == 0 && lane < m) log_std_adam(a, hp, dls, lane, grad, o_ls);
        {
            // the units 16 jub .. + 15 of a layer (upstream tile gl, pitch PLD) against 16 columns of [input, 1]
            const auto job = [&](int t, int U, int K, int jub, int col0, const float* gl, const float* bl, int bld,
                                 int boff, int64_t gw, int64_t gb) {
                wgrad_job(a, hp, grad, t, U, K, jub, col0, gl, PLD, 16 * jub, bl, bld, boff, gw, gb, r, q);
            };
            const int CB2 = h1 / 16 + 1, CB1 = h0 / 16 + 1;   // column blocks of [a1, 1], [a0, 1]
            const int nj2 = UB2 * CB2, nj1 = UB1 * CB1;
            int resident = nchunk_f - 1;
            for (int c = nchunk_b - 1; c >= 0; --c) {
                if (c != resident && n > c * XCW) {   // (a chunk holding only the column of ones needs no tile)
                    PF_STAMP(10);
                    __syncthreads();   // the previous chunk's jobs have read Xs
                    PF_STAMP(13);
                    load_chunk(c);
                    __syncthreads();
                    resident = c;
                    PF_STAMP(9);
                }
                const int cb0 = n / 16 + 1 - c * (XCW / 16);          // layer 0's column blocks from this chunk on
                const int nb0 = cb0 < XCW / 16 ? cb0 : XCW / 16;
                const int nj0 = UB0 * nb0;
                const int nj = nj0 + (c == nchunk_b - 1 ? nj2 + nj1 : 0);   // the first chunk visited carries layers 2 and 1
                for (int j = w; j < nj; j += PW) {
                    if (j < nj0)
                        job(0, h0, n, j / nb0, c * XCW + 16 * (j % nb0), g0s, Xs, XLD, c * XCW, 0, o_b0);
                    else if (j < nj0 + nj2)
                        job(4, m, h1, (j - nj0) / CB2, 16 * ((j - nj0) % CB2), zs, a1s, PLD, 0, o_W2, o_b2);
                    else
                        job(2, h1, h0, (j - nj0 - nj2) / CB1, 16 * ((j - nj0 - nj2) % CB1), g1s, a0s, PLD, 0, o_W1, o_b1);
                }
            }
        }
        PF_STAMP(10);      // wave 0's own jobs
        __syncthreads();   // this step's stores before the next step's loads (one CU: workgroup scope)
        PF_STAMP(11);
    }
#ifdef MJRL_PFIT_PROF
    if (tid < PF_NPROF) reinterpret_cast<unsigned long long*>(a.scratch + 8)[tid] += s_prof[tid];
#endif
}

// An entry point: policy_step.h's checks and argument filling, then the launches of nmb steps,
// at most PF_SPL a launch.
template <bool MSE, class Net>
int run_steps(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs, const Net* net,
              const mjrl_adam* hp, float* scratch, int32_t steps_per_launch, float* grad_out, float* loss_out,
              void* stream) {
    if (steps_per_launch < 0) return MJRL_EINVAL;
    PfitArgs a;
    const int rc = step_args<MSE>(a, data, idx, nmb, bs, net, hp, scratch, PF_SCRATCH, PH);
    if (rc != MJRL_OK || nmb == 0) return rc;
    const int spl = steps_per_launch == 0 || steps_per_launch > PF_SPL ? PF_SPL : steps_per_launch;
    for (int64_t k0 = 0; k0 < nmb; k0 += spl) {
        const int ns = (int)(nmb - k0 < spl ? nmb - k0 : spl);
        for (int s = 0; s < ns; ++s) adam_bias(hp, k0 + s, a.step_size[s], a.bc2s[s]);
        for (int s = ns; s < PF_SPL; ++s) a.step_size[s] = a.bc2s[s] = 1.f;
        a.nsteps = ns;
        a.idx = idx + k0 * bs;
        a.grad = grad_out ? grad_out + k0 * a.d : nullptr;
        a.loss = loss_out ? loss_out + k0 : nullptr;
        hipLaunchKernelGGL(k_pfit<MSE>, dim3(1), dim3(PF_THREADS), 0, (hipStream_t)stream, a);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int mjrl_policy_fit_scratch(int32_t n, int32_t m, int32_t h0, int32_t h1, int32_t bs, int64_t* floats) {
    return scratch_query(n, m, h0, h1, bs, PH, PF_SCRATCH, floats);
}

int mjrl_policy_fit_epoch(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
                          const mjrl_policy_net* net, const mjrl_adam* hp, float* scratch, int32_t steps_per_launch,
                          float* grad_out, float* loss_out, void* stream) {
    return run_steps<false>(data, idx, nmb, bs, net, hp, scratch, steps_per_launch, grad_out, loss_out, stream);
}

int mjrl_policy_mse_epoch(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
                          const mjrl_mean_net* net, const mjrl_adam* hp, float* scratch, int32_t steps_per_launch,
                          float* grad_out, float* loss_out, void* stream) {
    return run_steps<true>(data, idx, nmb, bs, net, hp, scratch, steps_per_launch, grad_out, loss_out, stream);
}

}  // extern "C"
