// policy_fit.hip — the minibatch Adam steps of PPO and BC on the Gaussian MLP policy
// as one hand-written kernel (mjrl/algos/ppo_clip.py:47-54,
// 89-95, behavior_cloning.py:39-63).
//
// The policy is Linear(n, h0) - tanh - Linear(h0, h1) - tanh - Linear(h1, m) plus
// log_std[m], torch's own parameter layouts and order W0 [h0][n], b0, W1 [h1][h0],
// b1, W2 [m][h1], b2, log_std, 1 <= h0, h1, m <= 64 (actual sizes: zero-padded in
// the loads, not in memory).  One step trains on bs <= 64 rows named by a device
// index buffer.
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
// A step, every phase ending in a workgroup barrier:
//   1  row indices, per-column constants (sigma, out_scale / sigma, (sigma / sigma_old)^2)
//   2  layer 0 over column chunks of the gathered, normalised X tile (256 columns in
//      LDS at a time): a0 = tanh(xhat W0^T + b0)
//   3  a1 = tanh(a0 W1^T + b1)
//   4  mu = (a1 W2^T + b2) out_scale + out_shift, z = (act - mu) / sigma
//   5  per row: LL, the loss head, dL/dLL (f64 sums, one order)
//   6  d log_std, the step's loss; then gmu = dL/dLL z out_scale / sigma in place of z
//   7  g1 = (gmu W2) o (1 - a1^2)
//   8  g0 = (g1 W1) o (1 - a0^2)
//   9  the weight gradients as 16 x 16 jobs (dW2 = gmu^T [a1, 1], dW1 = g1^T [a0, 1],
//      dW0 = g0^T [xhat, 1] chunk by chunk, the last forward chunk first: it is still
//      in LDS; the bias sums ride along as a column of ones), Adam on exactly the
//      elements of each job, log_std's Adam.  Every use of a step's parameters is
//      behind a barrier before the first of these stores.
//
// Arithmetic: products on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fma chain,
// one accumulator per output tile), every sum in one fixed order, no atomic: the same
// state and arguments give the same bits, however the steps are split over launches
// and calls.  Adam is fit.h's adam_step, the bias corrections of step t formed
// on the host in f64 from t alone.  Rows bs .. 63 and a row whose index is outside
// [0, T) are masked: nothing of obs / act / adv / ll_old is read for them, their
// dL/dLL is 0, the mean still divides by bs.
//
// k_pfit<true> is the same step under the MSE head of mjrl/algos/behavior_cloning_2.py:46-50
// (mjrl_policy_mse_epoch): L = sum (mu - act)^2 / (bs m) over the unmasked rows, on the six
// tensors of the mean network.  Phase 1 takes sigma = 1 and never reads log_std, phase 4's
// z is act - mu, phase 5's row term is sum z^2 / m with -2 / (bs m) in dL/dLL's place,
// phases 6 and 9 have no log_std.  p[6] / m[6] / v[6] are null there and nothing touches them.
#include "fit.h"

using namespace mjrl;

namespace {

constexpr int PR = 64;                // padded minibatch rows
constexpr int PH = 64;                // largest hidden / action width
constexpr int PLD = PH + 4;           // LDS row pitch of the [64][64] tiles: rows 4 banks apart
constexpr int XCW = 256;              // columns of the X tile held in LDS at a time
constexpr int XLD = XCW + 4;          // its row pitch
constexpr int PF_THREADS = 512;
constexpr int PW = PF_THREADS / 64;   // waves
constexpr int PF_SPL = 128;           // steps of one launch at the most (their Adam constants are kernel arguments)
constexpr int64_t PF_SCRATCH = 64;    // floats: [0] the last step's loss
constexpr int PF_BC = 0, PF_PPO = 1;
constexpr double HALF_LOG_2PI = 0.91893853320467274178;

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

struct PfitArgs {
    const float *obs, *act, *adv, *ll_old, *old_ls;
    const float *in_shift, *in_scale, *out_shift, *out_scale;
    const int64_t* idx;               // this launch's first minibatch
    int64_t T;
    float* p[7];                      // W0, b0, W1, b1, W2, b2, log_std (torch order)
    float* m[7];
    float* v[7];
    float* scratch;
    int64_t scap;                     // floats of scratch (debug build: checked)
    float* grad;                      // null or this launch's first [d] gradient
    float* loss;                      // null or this launch's first loss slot
    int64_t d;
    int n, na, h0, h1, bs, kind, nsteps;   // na: the action width m
    int vx, vw0, vw1, vw2;            // 16-byte loads of obs rows / W0 / W1 / W2 rows allowed
    float clip_lo, clip_hi;           // float(1 - c), float(1 + c)
    AdamK hp;                         // the step-independent part
    float step_size[PF_SPL], bc2s[PF_SPL];   // hp's other two fields for each step of this launch
};

// MSE: the mean-squared-error head (behavior_cloning_2.py:46-50) on the six tensors of the mean
// network, a compile-time switch so that the BC / PPO instantiation stays the code it was.
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
    const int n = a.n, m = a.na, h0 = a.h0, h1 = a.h1, bs = a.bs;
    const int UB0 = (h0 + 15) / 16, UB1 = (h1 + 15) / 16, UB2 = (m + 15) / 16;   // unit blocks
    const int H0P = 16 * UB0, H1P = 16 * UB1, MP = 16 * UB2;
    const bool aliased = a.kind == PF_PPO && a.old_ls != nullptr;
    float *const W0 = a.p[0], *const b0 = a.p[1], *const W1 = a.p[2], *const b1 = a.p[3], *const W2 = a.p[4],
                 *const b2 = a.p[5], *const ls = a.p[6];
    // flat places of the seven tensors in a step's gradient
    const int64_t o_b0 = (int64_t)h0 * n, o_W1 = o_b0 + h0, o_b1 = o_W1 + (int64_t)h1 * h0, o_W2 = o_b1 + h1,
                  o_b2 = o_W2 + (int64_t)m * h1, o_ls = o_b2 + m;
    // forward / chain products: wave w owns unit block w & 3 and the row blocks 2 (w >> 2), + 1
    const int ub = w & 3, rb0 = 2 * (w >> 2);
    const int nchunk_f = (n + XCW - 1) / XCW;   // forward chunks
    const int nchunk_b = n / XCW + 1;           // backward chunks: the column of ones (col n) counts

    AdamK hp = a.hp;   // step_size / bc2s: the current step's, set below

    // the gathered, normalised X tile of chunk c: 8 threads per row, zero-filled to a multiple of 16 columns
    auto load_chunk = [&](int c) {
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
                *reinterpret_cast<float4*>(Xs + xr * XLD + col) = o;
            }
        } else {
#pragma unroll 8
            for (int i = 0; i < XCW / 8; ++i) {
                const int col = xc + 8 * i;
                if (col >= cwp) continue;
                float o = 0.f;
                if (xi >= 0 && col < cw) o = (xrow[col] - a.in_shift[c0 + col]) / (a.in_scale[c0 + col] + 1e-8f);
                Xs[xr * XLD + col] = o;
            }
        }
    };

    // One weight-gradient job and Adam on its elements: the 16 units 16 jub .. + 15 of a layer
    // against the 16 columns col0 .. + 15 of [input, 1].  gl: the layer's upstream tile
    // (pitch PLD), bl / bld / boff: the input tile and the tile column of input column 0.
    // A lane's accumulator register i belongs to the weight [unit 4 q + i][col] (col < K), to
    // that unit's bias (col == K) or to nothing.
    auto wgrad_job = [&](int t, int U, int K, int jub, int col0, const float* gl, const float* bl, int bld, int boff,
                         int64_t gw, int64_t gb, float* grad) {
        float *const pw = a.p[t], *const mw = a.m[t], *const vw = a.v[t];
        float *const pb = a.p[t + 1], *const mb = a.m[t + 1], *const vb = a.v[t + 1];
        const int col = col0 + r;
        const int colc = col < K ? col : K - 1;
        float pm[4][3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int unit = 16 * jub + 4 * q + i, uc = unit < U ? unit : U - 1;
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
            acc = mfma4(gl[row * PLD + 16 * jub + r], col < K ? b : (col == K ? 1.f : 0.f), acc);
        }
        if (col <= K) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int unit = 16 * jub + 4 * q + i;
                if (unit >= U) continue;
                wgrad_tail(pm[i], acc[i], unit, K, col, hp, pw, mw, vw, pb, mb, vb, grad, gw, gb);
            }
        }
    };

    for (int step = 0; step < a.nsteps; ++step) {
        hp.step_size = a.step_size[step];
        hp.bc2s = a.bc2s[step];
        float* const grad = a.grad ? a.grad + (int64_t)step * a.d : nullptr;

        // ---- 1: the row indices, the per-column constants ----
        if (w == 0) {
            int64_t i = -1;
            if (lane < bs) {
                i = a.idx[(int64_t)step * bs + lane];
                i = i >= 0 && i < a.T ? i : -1;
            }
            s_row[lane] = i;
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
                    zs[row * PLD + col] = z;
                }
        }
        __syncthreads();
        PF_STAMP(4);

        // ---- 5: per row LL, the loss head, dL/dLL: 8 lanes per row, 8 columns each ----
        {
            const int row = tid >> 3, part = tid & 7;
            double sz = 0.0, sd = 0.0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int col = 8 * part + j;
                if (col < m) {
                    const double z = (double)zs[row * PLD + col];
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
        PF_STAMP(5);

        // ---- 6: d log_std (wave 0), the step's loss (wave 1); then gmu in place of z ----
        float dls = 0.f;
        if (!MSE && w == 0) {
            if (lane < m) {
                double s = 0.0;
                for (int row = 0; row < PR; ++row) {
                    const double z = (double)zs[row * PLD + lane];
                    s += (double)s_gll[row] * (z * z - 1.0);
                }
                dls = (float)s;
            }
        } else if (w == 1) {
            const double tot = wave_sum(s_lossd[lane]) / (double)bs;
            if (lane == 0) {
                MJRL_SLAB_CHECK(0, a.scap);
                a.scratch[0] = (float)tot;
                if (a.loss) a.loss[step] = (float)tot;
            }
        }
        __syncthreads();
        for (int e = tid; e < PR * MP; e += PF_THREADS) {
            const int row = e / MP, col = e % MP;
            zs[row * PLD + col] = s_gll[row] * (zs[row * PLD + col] * s_gsc[col]);
        }
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
        if (!MSE && w == 0 && lane < m) {
            float p1, m1, v1;
            adam_step(ls[lane], a.m[6][lane], a.v[6][lane], dls, hp, p1, m1, v1);
            if (grad) grad[o_ls + lane] = dls;
            ls[lane] = p1;
            a.m[6][lane] = m1;
            a.v[6][lane] = v1;
        }
        {
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
                        wgrad_job(0, h0, n, j / nb0, c * XCW + 16 * (j % nb0), g0s, Xs, XLD, c * XCW, 0, o_b0, grad);
                    else if (j < nj0 + nj2)
                        wgrad_job(4, m, h1, (j - nj0) / CB2, 16 * ((j - nj0) % CB2), zs, a1s, PLD, 0, o_W2, o_b2, grad);
                    else
                        wgrad_job(2, h1, h0, (j - nj0 - nj2) / CB1, 16 * ((j - nj0 - nj2) % CB1), g1s, a0s, PLD, 0, o_W1,
                                  o_b1, grad);
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

// What both entry points share once their arguments are checked: the sizes, the row and
// transformation pointers, the 16-byte-load flags, then the launches of nmb steps, at most
// PF_SPL a launch.  a.p / m / v, a.adv / ll_old / old_ls, a.kind and the clip range are the caller's.
template <bool MSE>
int run_steps(PfitArgs& a, const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
              const mjrl_adam* hp, float* scratch, int32_t steps_per_launch, float* grad_out, float* loss_out,
              void* stream) {
    const int n = data->n, m = data->m, h0 = data->h0, h1 = data->h1;
    hipStream_t st = (hipStream_t)stream;
    const int spl = steps_per_launch == 0 || steps_per_launch > PF_SPL ? PF_SPL : steps_per_launch;
    a.obs = data->obs;
    a.act = data->act;
    a.in_shift = data->in_shift;
    a.in_scale = data->in_scale;
    a.out_shift = data->out_shift;
    a.out_scale = data->out_scale;
    a.T = data->T;
    a.scratch = scratch;
    a.scap = PF_SCRATCH;
    a.d = (int64_t)h0 * n + h0 + (int64_t)h1 * h0 + h1 + (int64_t)m * h1 + m + (MSE ? 0 : m);
    a.n = n;
    a.na = m;
    a.h0 = h0;
    a.h1 = h1;
    a.bs = bs;
    const auto al16 = [](const void* p) { return (uintptr_t)p % 16 == 0; };
    a.vx = n % 4 == 0 && al16(data->obs) && al16(data->in_shift) && al16(data->in_scale);
    a.vw0 = n % 4 == 0 && al16(a.p[0]);
    a.vw1 = h0 % 4 == 0 && al16(a.p[2]);
    a.vw2 = h1 % 4 == 0 && al16(a.p[4]);
    a.hp = adam_consts(hp);
    for (int64_t k0 = 0; k0 < nmb; k0 += spl) {
        const int ns = (int)(nmb - k0 < spl ? nmb - k0 : spl);
        for (int s = 0; s < ns; ++s) adam_bias(hp, k0 + s, a.step_size[s], a.bc2s[s]);
        for (int s = ns; s < PF_SPL; ++s) a.step_size[s] = a.bc2s[s] = 1.f;
        a.nsteps = ns;
        a.idx = idx + k0 * bs;
        a.grad = grad_out ? grad_out + k0 * a.d : nullptr;
        a.loss = loss_out ? loss_out + k0 : nullptr;
        hipLaunchKernelGGL(k_pfit<MSE>, dim3(1), dim3(PF_THREADS), 0, st, a);
    }
    return (int)hipGetLastError();
}

// the checks both entry points make on what they both read; nmb > 0: the pointers too
bool sizes_ok(const mjrl_policy_fit_data* data, int64_t nmb, int32_t bs, int32_t steps_per_launch) {
    if (!data || bs < 1 || bs > PR || nmb < 0 || steps_per_launch < 0) return false;
    const int n = data->n, m = data->m, h0 = data->h0, h1 = data->h1;
    // n <= 2^24: the kernel indexes a tensor's elements with 32 bits
    return n > 0 && n <= (1 << 24) && m >= 1 && m <= PH && h0 >= 1 && h0 <= PH && h1 >= 1 && h1 <= PH && data->T >= 0;
}

bool pointers_ok(const mjrl_policy_fit_data* data, const int64_t* idx, const void* net, const mjrl_adam* hp,
                 const float* scratch) {
    if (!idx || !net || !hp || !scratch || hp->step0 < 0) return false;
    return data->obs && data->act && data->in_shift && data->in_scale && data->out_shift && data->out_scale;
}

}  // namespace

extern "C" {

int mjrl_policy_fit_scratch(int32_t n, int32_t m, int32_t h0, int32_t h1, int32_t bs, int64_t* floats) {
    if (n <= 0 || m < 1 || m > PH || h0 < 1 || h0 > PH || h1 < 1 || h1 > PH || bs < 1 || bs > PR || !floats)
        return MJRL_EINVAL;
    *floats = PF_SCRATCH;
    return MJRL_OK;
}

int mjrl_policy_fit_epoch(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
                          const mjrl_policy_net* net, const mjrl_adam* hp, float* scratch, int32_t steps_per_launch,
                          float* grad_out, float* loss_out, void* stream) {
    if (!sizes_ok(data, nmb, bs, steps_per_launch)) return MJRL_EINVAL;
    if (data->kind != MJRL_POLICY_FIT_BC && data->kind != MJRL_POLICY_FIT_PPO) return MJRL_EINVAL;
    if (data->kind == MJRL_POLICY_FIT_PPO && (!data->ll_old == !data->old_log_std)) return MJRL_EINVAL;
    if (nmb == 0) return MJRL_OK;
    if (!pointers_ok(data, idx, net, hp, scratch)) return MJRL_EINVAL;
    if (data->kind == MJRL_POLICY_FIT_PPO && !data->adv) return MJRL_EINVAL;
    PfitArgs a;
    if (!net_ptrs(net, a.p, a.m, a.v)) return MJRL_EINVAL;
    a.adv = data->adv;
    a.ll_old = data->kind == MJRL_POLICY_FIT_PPO ? data->ll_old : nullptr;
    a.old_ls = data->kind == MJRL_POLICY_FIT_PPO ? data->old_log_std : nullptr;
    a.kind = data->kind == MJRL_POLICY_FIT_PPO ? PF_PPO : PF_BC;
    a.clip_lo = (float)(1.0 - data->clip);
    a.clip_hi = (float)(1.0 + data->clip);
    return run_steps<false>(a, data, idx, nmb, bs, hp, scratch, steps_per_launch, grad_out, loss_out, stream);
}

int mjrl_policy_mse_epoch(const mjrl_policy_fit_data* data, const int64_t* idx, int64_t nmb, int32_t bs,
                          const mjrl_mean_net* net, const mjrl_adam* hp, float* scratch, int32_t steps_per_launch,
                          float* grad_out, float* loss_out, void* stream) {
    if (!sizes_ok(data, nmb, bs, steps_per_launch)) return MJRL_EINVAL;
    if (nmb == 0) return MJRL_OK;
    if (!pointers_ok(data, idx, net, hp, scratch)) return MJRL_EINVAL;
    PfitArgs a;
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
    return run_steps<true>(a, data, idx, nmb, bs, hp, scratch, steps_per_launch, grad_out, loss_out, stream);
}

}  // extern "C"
