// policy_fit.hip — the minibatch Adam steps of PPO and BC on the Gaussian MLP policy
// as one hand-written kernel (mjrl/algos/ppo_clip.py:47-54,
// 89-95, behavior_cloning.py:39-63), for 1 <= h0, h1, m <= 64 (actual sizes: zero-padded in
// the loads, not in memory).  The policy, the masking of rows, the heads (k_pfit<true>: MSE) and
// every piece this kernel shares with policy_fit_wide.hip and policy_fit_rows.hip are policy_step.h's.
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
// A step, every phase ending in a workgroup barrier (in brackets: policy_step.h's piece; k_pfr_grad
// of policy_fit_rows.hip runs the same pieces on a row tile, the wide kernels those that fit them):
//   1  row indices (mb_row), per-column constants (head_consts)
//   2  layer 0 over column chunks of the gathered, normalised X tile (chain_fwd_x over stage_x,
//      256 columns in LDS at a time): a0 = tanh(xhat W0^T + b0) (chain_tanh)
//   3  a1 = tanh(a0 W1^T + b1) (chain_fwd, chain_tanh)
//   4  mu = (a1 W2^T + b2) out_scale + out_shift, z = (act - mu) / sigma (chain_fwd, head_z)
//   5  per row: LL, the loss head, dL/dLL (head_rows)
//   6  d log_std, the step's loss (head_sums over head_dls); then gmu in place of z (head_gmu)
//   7  g1 = (gmu W2) o (1 - a1^2) (chain_bwd)
//   8  g0 = (g1 W1) o (1 - a0^2) (chain_bwd)
//   9  the weight gradients as 16 x 16 jobs (wgrad_walk over wgrad_job: dW2 = gmu^T [a1, 1],
//      dW1 = g1^T [a0, 1], dW0 = g0^T [xhat, 1] chunk by chunk, the last forward chunk first: it
//      is still in LDS; the bias sums ride along as a column of ones), Adam on exactly the
//      elements of each job, log_std's Adam (log_std_adam).  Every use of a step's parameters is
//      behind a barrier before the first of these stores.  The tensors' places in grad_out: grad_at.
//
// Arithmetic: products on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fma chain,
// one accumulator per output tile), every sum in one fixed order, no atomic: the same
// state and arguments give the same bits, however the steps are split over launches
// and calls.  Adam is fit.h's adam_step, the bias corrections of step t formed
// on the host in f64 from t alone.
#include "policy_step.h"

using namespace mjrl;

namespace {

constexpr int PR = PS_ROWS, PH = PS_H, PLD = PS_LD, XLD = PS_XLD;   // the tiles: policy_step.h
constexpr int PF_THREADS = PS_THREADS;
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
    const GradAt o = grad_at(n, m, h0, h1, MSE);
    const ChainTiles tiles = {Xs, a0s, a1s, g0s, g1s, zs};
    // forward / chain products: wave w owns unit block w & 3 and the row blocks 2 (w >> 2), + 1
    const int ub = w & 3, rb0 = 2 * (w >> 2);

    AdamK hp = a.hp;   // step_size / bc2s: the current step's, set below
    // a lambda capturing n: called directly, stage_x costs 69 more SGPR reloads and 0.4 % of Swimmer's epochs
    const auto load_chunk = [&](int c) { stage_x<XLD>(a, n, s_row, Xs, c, tid); };
    const auto stamp = [&](int i) { PF_STAMP(i); };

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
            chain_fwd_x<XLD, 2>(acc, Xs, ub < UB0, rb0, W0, h0, n, ub, a.vw0, r, q, load_chunk, stamp);
            if (ub < UB0) chain_tanh<PLD>(acc, a0s, rb0, b0, h0, ub, r, q);
        }
        __syncthreads();
        PF_STAMP(2);

        // ---- 3: a1 = tanh(a0 W1^T + b1) ----
        if (ub < UB1) {
            floatx4 acc[2] = {zero4(), zero4()};
            chain_fwd<PLD, 2>(acc, a0s, rb0, W1, h1, h0, ub, 0, UB0, a.vw1, r, q);
            chain_tanh<PLD>(acc, a1s, rb0, b1, h1, ub, r, q);
        }
        __syncthreads();
        PF_STAMP(3);

        // ---- 4: mu = (a1 W2^T + b2) out_scale + out_shift, z = (act - mu) / sigma ----
        if (ub < UB2) {
            floatx4 acc[2] = {zero4(), zero4()};
            chain_fwd<PLD, 2>(acc, a1s, rb0, W2, m, h1, ub, 0, UB1, a.vw2, r, q);
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
        if (ub < UB1) chain_bwd<PLD>(zs, W2, m, h1, UB2, a1s, g1s, ub, rb0, r, q);
        __syncthreads();
        PF_STAMP(7);

        // ---- 8: g0 = (g1 W1) o (1 - a0^2) ----
        if (ub < UB0) chain_bwd<PLD>(g1s, W1, h1, h0, UB1, a0s, g0s, ub, rb0, r, q);
        __syncthreads();
        PF_STAMP(8);

        // ---- 9: the weight gradients and Adam; every read of this step's parameters is behind us ----
        if (!MSE && w == 0 && lane < m) log_std_adam(a, hp, dls, lane, grad, o.ls);
        const auto job = [&](int t, int U, int K, int jub, int col0, const float* gl, const float* bl, int bld,
                             int boff, int64_t gw, int64_t gb) {
            wgrad_job(a, hp, grad, t, U, K, jub, col0, gl, PLD, 16 * jub, bl, bld, boff, gw, gb, r, q);
        };
        wgrad_walk(n, m, h0, h1, w, tiles, o, load_chunk, job, stamp);
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
