// policy_fit_rows.hip — policy_fit.hip's minibatch Adam step (phases 1-9 of its header comment)
// for minibatches of up to 16384 rows, sliced over row tiles (fit_backend = "hip_rows";
// mjrl_policy_fit_rows_epoch), for 1 <= h0, h1, m <= 64 and the BC and PPO heads (the MSE head is
// not built here).  The policy, the masking of rows, the heads, the chain products of phases 2-8
// and phase 9's walk over the weight-gradient jobs are policy_step.h's, as they are k_pfit's.
//
// The forward chain, the loss head and the backward chain of 64 rows are independent of every
// other 64 rows; only the weight-gradient sums and Adam join them.  So one workgroup owns 64 rows
// of the step, and the join is a kernel boundary: no grid barrier, no flag, no spin loop, no
// atomic, no cooperative launch.  Step k is two launches on one stream:
//   k_pfr_grad  grid G = ceil(bs / 64).  Workgroup g runs k_pfit's phases 1-8 on rows 64 g .. + 63
//       of the minibatch (rows past bs and indices outside [0, T) masked, the head dividing by the
//       whole bs), then phase 9's weight-gradient jobs WITHOUT Adam: every accumulator goes to its
//       flat place (torch parameter order, as grad_out has it) in this tile's slice part[g][0 .. d)
//       of a slab in the scratch, the tile's d log_std to part[g][o_ls + j], the tile's loss sum
//       (f64, not yet divided) to a slot of its own.  It reads the parameters and writes nothing
//       but its slice and its slot, all d entries of the slice every step: the slab needs no
//       zero-fill, and a tile whose rows are all masked writes zeros.
//   k_pfr_adam  over the d elements: element e's gradient is the f64 sum of part[0 .. G)[e] in
//       ascending tile order from tile 0's value, rounded once to f32; then weight decay and
//       fit.h's adam_step on (p, m, v) in place, and grad_out[k][e].  One more workgroup folds the
//       loss the same way, divides by bs, rounds once.  The slab is [G][d]: neighbouring threads
//       read neighbouring floats of one slice.
// With bs <= 64 there is one tile and the fold is the identity: the parameters, the moments,
// grad_out and loss_out carry mjrl_policy_fit_epoch's bits.
//
// The scratch (floats): [0] the last step's loss, [4 .. 516) the 256 tiles' loss sums as doubles,
// from 516 on the slab.
//
// Arithmetic: policy_fit.hip's contract (exact-f32 MFMA, one accumulator per output tile, k
// ascending, every sum in one fixed order, no atomic, fit.h's Adam, the bias corrections formed
// on the host): the same state and arguments give the same bits, however the steps are split
// over calls.
#include "policy_step.h"

using namespace mjrl;

namespace {

constexpr int PR = PS_ROWS, PH = PS_H, PLD = PS_LD, XLD = PS_XLD;   // the tiles: policy_step.h
constexpr int RT = PS_THREADS;        // threads of a k_pfr_grad workgroup
constexpr int MAX_TILES = MJRL_POLICY_FIT_ROWS_MAX_BS / PR;
constexpr int AT = 256;               // threads of a k_pfr_adam workgroup
constexpr int LOSS_OFF = 0, LSUM_OFF = 4, SLAB_OFF = LSUM_OFF + 2 * MAX_TILES;   // floats; 16-byte aligned

static_assert(MJRL_POLICY_FIT_ROWS_MAX_BS % PR == 0 && SLAB_OFF % 4 == 0, "scratch layout");

// StepArgs: idx, grad, loss and hp are those of the step the launch belongs to
struct RowsArgs : StepArgs {
    int G;                            // row tiles of a step
};

// floats of scratch for G tiles of d gradients
inline int64_t rows_scratch(int64_t d, int64_t G) { return (SLAB_OFF + G * d + 3) / 4 * 4; }

__global__ void __launch_bounds__(RT) k_pfr_grad(RowsArgs a) {
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
    const int tile = blockIdx.x;
    const int n = a.n, m = a.na, h0 = a.h0, h1 = a.h1;
    const int UB0 = (h0 + 15) / 16, UB1 = (h1 + 15) / 16, UB2 = (m + 15) / 16;   // unit blocks
    const int MP = 16 * UB2;
    const bool aliased = a.kind == PF_PPO && a.old_ls != nullptr;
    const float *const W0 = a.p[0], *const b0 = a.p[1], *const W1 = a.p[2], *const b1 = a.p[3], *const W2 = a.p[4];
    const GradAt o = grad_at(n, m, h0, h1, false);
    const ChainTiles tiles = {Xs, a0s, a1s, g0s, g1s, zs};
    const int64_t off = SLAB_OFF + (int64_t)tile * a.d;   // this tile's slice of the slab
    // forward / chain products: wave w owns unit block w & 3 and the row blocks 2 (w >> 2), + 1
    const int ub = w & 3, rb0 = 2 * (w >> 2);

    const auto load_chunk = [&](int c) { stage_x<XLD>(a, n, s_row, Xs, c, tid); };
    const auto no_stamp = [](int) {};

    // ---- 1: the row indices, the per-column constants ----
    if (w == 0)
        s_row[lane] = mb_row(a, 0, PR * tile + lane);
    else if (w == 1)
        head_consts<false>(a, aliased, lane, s_sig, s_gsc, s_q, s_lsum);
    __syncthreads();

    // ---- 2: a0 = tanh(xhat W0^T + b0), xhat chunk by chunk ----
    {
        floatx4 acc[2] = {zero4(), zero4()};
        chain_fwd_x<XLD, 2>(acc, Xs, ub < UB0, rb0, W0, h0, n, ub, a.vw0, r, q, load_chunk, no_stamp);
        if (ub < UB0) chain_tanh<PLD>(acc, a0s, rb0, b0, h0, ub, r, q);
    }
    __syncthreads();

    // ---- 3: a1 = tanh(a0 W1^T + b1) ----
    if (ub < UB1) {
        floatx4 acc[2] = {zero4(), zero4()};
        chain_fwd<PLD, 2>(acc, a0s, rb0, W1, h1, h0, ub, 0, UB0, a.vw1, r, q);
        chain_tanh<PLD>(acc, a1s, rb0, b1, h1, ub, r, q);
    }
    __syncthreads();

    // ---- 4: mu = (a1 W2^T + b2) out_scale + out_shift, z = (act - mu) / sigma ----
    if (ub < UB2) {
        floatx4 acc[2] = {zero4(), zero4()};
        chain_fwd<PLD, 2>(acc, a1s, rb0, W2, m, h1, ub, 0, UB1, a.vw2, r, q);
        head_z<false, PLD>(a, acc, ub, rb0, r, q, s_sig, s_row, zs);
    }
    __syncthreads();

    // ---- 5: per row LL, the loss head, dL/dLL (the mean divides by the whole bs) ----
    head_rows<false, PLD>(a, aliased, tid, zs, s_q, s_lsum, s_row, s_gll, s_lossd);
    __syncthreads();

    // ---- 6: the tile's d log_std (wave 0) and loss sum (wave 1); then gmu in place of z ----
    float dls = 0.f;
    if (w == 0) {
        dls = head_dls<PLD>(m, lane, zs, s_gll);
    } else if (w == 1) {
        const double tot = wave_sum(s_lossd[lane]);
        if (lane == 0) {
            MJRL_SLAB_CHECK(LSUM_OFF + 2 * tile + 1, a.scap);
            reinterpret_cast<double*>(a.scratch + LSUM_OFF)[tile] = tot;
        }
    }
    __syncthreads();
    head_gmu<PLD>(zs, s_gll, s_gsc, MP, tid);
    __syncthreads();

    // ---- 7: g1 = (gmu W2) o (1 - a1^2) ----
    if (ub < UB1) chain_bwd<PLD>(zs, W2, m, h1, UB2, a1s, g1s, ub, rb0, r, q);
    __syncthreads();

    // ---- 8: g0 = (g1 W1) o (1 - a0^2) ----
    if (ub < UB0) chain_bwd<PLD>(g1s, W1, h1, h0, UB1, a0s, g0s, ub, rb0, r, q);
    __syncthreads();

    // ---- 9: the tile's weight gradients into its slice, k_pfit's jobs in k_pfit's order ----
    if (w == 0 && lane < m) {
        MJRL_SLAB_CHECK(off + o.ls + lane, a.scap);
        a.scratch[off + o.ls + lane] = dls;
    }
    const auto job = [&](int, int U, int K, int jub, int col0, const float* gl, const float* bl, int bld, int boff,
                         int64_t gw, int64_t gb) {
        wgrad_store_job(a, off, U, K, jub, col0, gl, PLD, 16 * jub, bl, bld, boff, gw, gb, r, q);
    };
    wgrad_walk(n, m, h0, h1, w, tiles, o, load_chunk, job, no_stamp);
}

// The fold over the row tiles and Adam: workgroups 0 .. ceil(d / AT) - 1 own AT elements each of
// the flat parameter vector, the last workgroup the loss.
__global__ void __launch_bounds__(AT) k_pfr_adam(RowsArgs a) {
    __shared__ double s_part[MAX_TILES];
    const int G = a.G;
    const int64_t d = a.d;
    if ((int64_t)blockIdx.x * AT >= d) {
        // the loss: the tiles' sums in ascending order from tile 0's, then the mean, rounded once
        for (int g = threadIdx.x; g < G; g += AT) {
            MJRL_SLAB_CHECK(LSUM_OFF + 2 * g + 1, a.scap);
            s_part[g] = reinterpret_cast<const double*>(a.scratch + LSUM_OFF)[g];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = s_part[0];
#pragma unroll 8
            for (int g = 1; g < G; ++g) s += s_part[g];
            const float tot = (float)(s / (double)a.bs);
            MJRL_SLAB_CHECK(LOSS_OFF, a.scap);
            a.scratch[LOSS_OFF] = tot;
            if (a.loss) *a.loss = tot;
        }
        return;
    }
    const int64_t e = (int64_t)blockIdx.x * AT + threadIdx.x;
    if (e >= d) return;
    const float* const part = a.scratch + SLAB_OFF + e;
    MJRL_SLAB_CHECK(SLAB_OFF + (int64_t)(G - 1) * d + e, a.scap);
    double s = (double)part[0];
#pragma unroll 8
    for (int g = 1; g < G; ++g) s += (double)part[(int64_t)g * d];
    const float gr = (float)s;
    // the element's tensor and its place in it (torch parameter order)
    const GradAt o = grad_at(a.n, a.na, a.h0, a.h1, false);
    const int t = (e >= o.b0) + (e >= o.W1) + (e >= o.b1) + (e >= o.W2) + (e >= o.b2) + (e >= o.ls);
    const int64_t i =
        e - (t == 0 ? 0 : t == 1 ? o.b0 : t == 2 ? o.W1 : t == 3 ? o.b1 : t == 4 ? o.W2 : t == 5 ? o.b2 : o.ls);
    const auto pick = [t](float* (&x)[7]) {
        return t == 0 ? x[0] : t == 1 ? x[1] : t == 2 ? x[2] : t == 3 ? x[3] : t == 4 ? x[4] : t == 5 ? x[5] : x[6];
    };
    float *const p = pick(a.p) + i, *const mo = pick(a.m) + i, *const v = pick(a.v) + i;
    float p1, m1, v1;
    adam_step(*p, *mo, *v, gr, a.hp, p1, m1, v1);
    if (a.grad) a.grad[e] = gr;
    *p = p1;
    *mo = m1;
    *v = v1;
}

}  // namespace

extern "C" {

int mjrl_policy_fit_rows_scratch(int32_t n, int32_t m, int32_t h0, int32_t h1, int32_t bs, int64_t* floats) {
    const int64_t G = ((int64_t)bs + PR - 1) / PR;
    return scratch_query(n, m, h0, h1, bs, PH, rows_scratch(grad_at(n, m, h0, h1, false).d, G), floats,
                         MJRL_POLICY_FIT_ROWS_MAX_BS);
}

int mjrl_policy_fit_rows_epoch(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
                               const mjrl_policy_net* net, const mjrl_adam* hp, float* scratch, float* grad_out,
                               float* loss_out, void* stream) {
    RowsArgs a;
    const int rc = step_args<false>(a, data, idx, nmb, bs, net, hp, scratch, 0, PH, MJRL_POLICY_FIT_ROWS_MAX_BS);
    if (rc != MJRL_OK || nmb == 0) return rc;
    a.G = (bs + PR - 1) / PR;
    a.scap = rows_scratch(a.d, a.G);
    hipStream_t st = (hipStream_t)stream;
    const dim3 gadam((unsigned)((a.d + AT - 1) / AT + 1));
    for (int64_t k = 0; k < nmb; ++k) {
        adam_bias(hp, k, a.hp.step_size, a.hp.bc2s);
        a.idx = idx + k * bs;
        a.grad = grad_out ? grad_out + k * a.d : nullptr;
        a.loss = loss_out ? loss_out + k : nullptr;
        hipLaunchKernelGGL(k_pfr_grad, dim3(a.G), dim3(RT), 0, st, a);
        hipLaunchKernelGGL(k_pfr_adam, gadam, dim3(AT), 0, st, a);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
