// rows.h — the row-pass argument block and helpers every policy-pass kernel shares,
// and k_rows, the general row kernel (included first by policy.hip).
//
//   k_rows<H0,H1,MP,MODE>  persistent, one 64-row (32 for 128- and 256-wide layers)
//                          tile of timesteps at a time; the whole per-row chain runs
//                          out of LDS on v_mfma_f32_16x16x4_f32:
//                            FWD  forward + LL + VPG upstream + backprop to every layer
//                            FVP  JVP of the tangent + Gauss-Newton weight + backprop
//                            EVAL forward at new params + likelihood ratio + KL
// Its upstreams go through HBM to k_wgrad / k_wgrad_all (wgrad.h); the slabs those
// write are folded by k_gather / k_gather_flat (gather.h).  DESIGN.md §4.
//
// Reference math: mjrl/policies/gaussian_mlp.py:100-182, gaussian_linear.py:98-175,
// mjrl/algos/batch_reinforce.py:37-55, mjrl/algos/npg_cg.py:55-74.
#pragma once

namespace {

enum { FWD = 0, FVP = 1, EVAL = 2 };

struct RowArgs {
    int64_t T;            // rows processed by this call
    int np, m;
    const float* xhat;
    const float* act;
    const float* adv;     // EVAL: surrogate advantages
    const float* adv_vpg; // FWD: advantages driving the gradient
    float* a0;
    float* a1;
    float* mu0;
    float* ll0;
    float* gu0;
    float* gu1;
    float* gp;
    const float* P;       // packed theta (new)
    const float* V;       // FVP: packed tangent;  EVAL: packed old theta (log_std)
    const float* out_shift;
    const float* out_scale;
    double* rpart;        // per-workgroup partials
    const int32_t* done;
    float llc;            // -0.5 * m * log(2 pi) rounded to f32
    const void* xs;       // split-f16 xhat rows [T][hi NP | lo NP] (k_kx), or null
    const float* xu;      // [T] power-of-two row scales of xs
    const float* xc;      // [NP] power-of-two column scales of xs
    // FWD with the batch assembly fused in (k_kx<.., FWD, true>): the staged f32
    // observations [T][n_obs] (identity input normalisation), converted to the split
    // rows in the tile publish, which also writes them to xs_w / xu_w
    const float* obs32;
    _Float16* xs_w;
    float* xu_w;
    int n_obs;
};

// rows per k_rows tile for a hidden width.  128-wide layers: 32 rows keep the f32
// activation buffers (4 x BT x (H + 4) floats) at 70 KB, two workgroups per CU —
// the HalfCheetah FVP 388 -> 298 us against 64 rows and one workgroup; 256-wide
// layers: 32 rows (16 rows, two workgroups per CU, measured 1 % slower)
__host__ __device__ constexpr int rows_bt(int hmax) { return hmax >= 128 ? 32 : 64; }
// threads per k_rows workgroup.  256-wide layers: one 138 KB workgroup per CU of
// 16 waves (four per SIMD, 128 VGPRs each); 128-wide: two 70 KB workgroups of 8
// waves.  Measured against 4 waves: door DAPG FVP 415 -> 369 us (8 waves) -> 353
// us (16); HalfCheetah TRPO FVP 298 -> 251 us (8).  The phase-1 staging and the
// row pass leave threads beyond the tile's elements idle.
__host__ __device__ constexpr int rows_nt(int hmax) { return hmax >= 256 ? 1024 : (hmax >= 128 ? 512 : NTHREADS); }

template <int H0, int H1, int MP>
struct Layout {
    static constexpr bool LIN = (H0 == 0);
    static constexpr int HMAX = H0 > H1 ? H0 : H1;
    static constexpr int BT = rows_bt(HMAX);
    static constexpr int RB = BT / 16;
    static constexpr int LD0 = LIN ? 0 : H0 + 4;
    static constexpr int LD1 = LIN ? 0 : H1 + 4;
    static constexpr int LDP = MP + 4;
    static constexpr int KC = 64;
    static constexpr int LDX = KC + 4;
    static constexpr int oD0 = 0;
    static constexpr int oA0 = oD0 + BT * LD0;
    static constexpr int oD1 = oA0 + BT * LD0;
    static constexpr int oA1 = oD1 + BT * LD1;
    static constexpr int oGP = oA1 + BT * LD1;
    static constexpr int XS = 2 * BT * LDX;
    static constexpr bool XS_ALIAS = !LIN && 2 * BT * LD1 >= XS;
    static constexpr int oXS = XS_ALIAS ? oD1 : oGP + BT * LDP;
    static constexpr int end1 = XS_ALIAS ? oGP + BT * LDP : oXS + XS;
    static constexpr int NT = rows_nt(HMAX);
    static constexpr int total = end1 > 2 * NT ? end1 : 2 * NT;   // >= row_pass_final's doubles
    static constexpr int bytes = total * 4;
};

__device__ __forceinline__ float tanh_f(float x) { return tanhf(x); }

// sum_j log_std_j in action order (the -sum(log_std) term of log_likelihood)
__device__ __forceinline__ float ls_sum(const float* __restrict__ P_ls, int m) {
    // sum(log_std) front to back; the loads of a 16-chunk are issued together
    // (adding the zero padding is exact)
    float s = 0.f;
    for (int j0 = 0; j0 < m; j0 += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = j0 + u < m ? P_ls[j0 + u] : 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u) s += v[u];
    }
    return s;
}

// Per-row pass of FWD / EVAL over a tile of BT rows whose output-layer values
// sit in GPs[BT][ldp] (gaussian_mlp.py:100-140 log_likelihood, mean_LL,
// likelihood_ratio, kl_old_new; batch_reinforce.py:37-55).
// Element-parallel over (row, action): thread tid owns action j = tid % MP of
// rows (tid + u NT) / MP, so the MP lanes of a row sit in one wave and the sums
// over actions are a fixed shuffle tree inside the row's lanes (no barrier).
//   FWD : mu0 <- mean; GPs <- adv z / sigma * out_scale (zero for j >= m and rows
//         past T); ll0 <- log-likelihood; acc0 += adv (z^2 - 1) (log-std VPG, action j).
//   EVAL: acc0 += exp(LL_new - LL_old) adv, acc1 += KL(old || new) (lanes j = 0).
// The per-thread partials are folded once per launch by row_pass_final.
// The per-row inputs of row_pass (actions, old means, old log-likelihoods,
// advantages) for this thread's elements, loaded ahead of the pass by a caller
// with registers to spare (the EVAL pass of k_kx loads them at the top of the
// tile, so the row pass no longer waits on them).
template <int BT, int MP, int NT>
struct RowPre {
    static constexpr int NE = BT * MP;
    static constexpr int PER = NE >= NT ? NE / NT : 1;
    float av[PER], mo[PER], l0[PER], ad[PER];
};

template <int MODE, int BT, int MP, int NT>
__device__ __forceinline__ void row_pre_load(const RowArgs& a, int64_t row_base, int tid, RowPre<BT, MP, NT>& pre) {
    using R = RowPre<BT, MP, NT>;
    const int m = a.m;
    const int64_t T = a.T;
    const int j = tid % MP;
    // unconditional loads from clamped indices, no selects: row_pass reads an element
    // only where it is valid (gr < T, j < m; j == 0 for the per-row values), and a
    // load under a branch would make every later vmcnt wait conservative (it waited
    // for the next tile's xhat loads)
    const int jc = j < m ? j : 0;
#pragma unroll
    for (int u = 0; u < R::PER; ++u) {
        const bool in = R::NE >= NT || tid + u * NT < R::NE;
        const int row = in ? (tid + u * NT) / MP : 0;
        const int64_t gr = in ? row_base + row : T;
        const int64_t gc = gr < T ? gr : T - 1;
        pre.av[u] = a.act[gc * m + jc];
        pre.mo[u] = MODE == EVAL ? a.mu0[gc * m + jc] : 0.f;
        pre.l0[u] = MODE == EVAL ? a.ll0[gc] : 0.f;
        pre.ad[u] = MODE == FWD ? a.adv_vpg[gc] : a.adv[gc];
    }
}

// The row pass's per-launch constants of this thread's action j (log-stds, out_scale),
// loaded once before the tile loop by callers that keep them in registers: a
// per-tile load would make the row pass wait (in-order vmcnt) on every global load
// issued before it, the next tile's xhat prefetch included.
struct RowConst {
    float lsn, sn, os, lso, so;
};

template <int MODE, int MP>
__device__ __forceinline__ RowConst row_const(const RowArgs& a, const float* __restrict__ P_ls, int tid) {
    const int j = tid % MP;
    const bool act_j = j < a.m;
    RowConst c;
    c.lsn = act_j ? P_ls[j] : 0.f;
    c.sn = expf(c.lsn);
    c.os = 1.f;
    c.lso = 0.f;
    c.so = 1.f;
    if (MODE == FWD) {
        if (a.out_scale && act_j) c.os = a.out_scale[j];
    } else {
        c.lso = act_j ? a.V[(P_ls - a.P) + j] : 0.f;
        c.so = expf(c.lso);
    }
    return c;
}

template <int MODE, int BT, int MP, int NT, bool STORE_GP, bool PRE = false>
__device__ __forceinline__ void row_pass(const RowArgs& a, const float* __restrict__ P_ls, float sls,
                                         int64_t row_base, float* GPs, int ldp, double& acc0, double& acc1,
                                         int tid, const RowPre<BT, MP, NT>* pre = nullptr,
                                         const RowConst* rc = nullptr) {
    constexpr int NE = BT * MP;                        // (row, action) elements of the tile
    constexpr int PER = NE >= NT ? NE / NT : 1;        // more threads than elements: the rest idle
    static_assert(NT % MP == 0 && (NE >= NT ? PER * NT == NE : NT % NE == 0) && MP <= 64, "row lanes in one wave");
    const int m = a.m;
    const int64_t T = a.T;
    const int j = tid % MP;
    const bool act_j = j < m;
    const RowConst c = rc ? *rc : row_const<MODE, MP>(a, P_ls, tid);
    const float lsn = c.lsn, sn = c.sn, os = c.os, lso = c.lso, so = c.so;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const bool in = NE >= NT || tid + u * NT < NE;
        const int row = in ? (tid + u * NT) / MP : 0;
        const int64_t gr = in ? row_base + row : T;        // an idle thread acts as a row past T
        const bool valid = gr < T && act_j;
        float* g = GPs + row * ldp + j;
        const float mu = in ? *g : 0.f;
        const float av = PRE ? pre->av[u] : (valid ? a.act[gr * m + j] : 0.f);
        float mo = 0.f, adv = 0.f;
        if (MODE == EVAL) mo = PRE ? pre->mo[u] : (valid ? a.mu0[gr * m + j] : 0.f);
        if (MODE == FWD) adv = PRE ? pre->ad[u] : (gr < T ? a.adv_vpg[gr] : 0.f);
        const float zs = valid ? (av - mu) / sn : 0.f;
        float z2 = zs * zs;
        float kl = 0.f;
        if (MODE == FWD) {
            if (valid) {
                a.mu0[gr * m + j] = mu;
                acc0 += (double)(adv * (z2 - 1.f));
            }
            const float gv = valid ? adv * (zs / sn) * os : 0.f;
            if (in) *g = gv;
            if (STORE_GP && gr < T) a.gp[gr * MP + j] = gv;
        } else if (valid) {
            const float dm = mo - mu;
            const float nr = (dm * dm + so * so) - sn * sn;
            const float dr = 2.f * sn * sn + 1e-8f;
            kl = (nr / dr + lsn) - lso;
        }
#pragma unroll
        for (int o = MP / 2; o > 0; o >>= 1) {
            z2 += __shfl_xor(z2, o, 64);
            if (MODE == EVAL) kl += __shfl_xor(kl, o, 64);
        }
        if (j == 0 && gr < T) {
            const float ll = ((-0.5f * z2) + (-sls)) + a.llc;
            if (MODE == FWD) {
                a.ll0[gr] = ll;
            } else {
                const float lr = expf(ll - (PRE ? pre->l0[u] : a.ll0[gr]));
                acc0 += (double)(lr * (PRE ? pre->ad[u] : a.adv[gr]));
                acc1 += (double)kl;
            }
        }
    }
}

// Fold the launch's row-pass partials (fixed order): FWD -> rpart[blk][MP]
// (log-std VPG sums), EVAL -> rpart[blk][2] (surrogate and KL sums).
// red: LDS scratch of NT doubles; the caller has synchronised the block.
template <int MODE, int MP, int NT>
__device__ __forceinline__ void row_pass_final(double acc0, double acc1, double* red, double* __restrict__ rpart,
                                               int64_t blk, int tid) {
    if (MODE == FWD) {
        red[tid] = acc0;
        __syncthreads();
        if (tid < MP) {
            double s = 0.0;
            for (int k = 0; k < NT / MP; ++k) s += red[k * MP + tid];
            rpart[blk * MP + tid] = s;
        }
    } else {
        if (tid % MP == 0) {
            red[tid / MP] = acc0;
            red[NT / MP + tid / MP] = acc1;
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0, k = 0.0;
            for (int i = 0; i < NT / MP; ++i) {
                s += red[i];
                k += red[NT / MP + i];
            }
            rpart[blk * 2 + 0] = s;
            rpart[blk * 2 + 1] = k;
        }
    }
}

template <int H0, int H1, int MP, int MODE>
__global__ void __launch_bounds__((Layout<H0, H1, MP>::NT), (Layout<H0, H1, MP>::bytes > 81920 ? 1 : 2))
    k_rows(RowArgs a) {
    using L = Layout<H0, H1, MP>;
    constexpr int BT = L::BT, RB = L::RB, NT = L::NT, NW = NT / 64;
    constexpr int N1 = L::LIN ? MP : H0;
    using S1 = Split<RB, N1 / 16, NW>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* D0 = smem + L::oD0;
    float* A0s = smem + L::oA0;
    float* D1 = smem + L::oD1;
    float* A1s = smem + L::oA1;
    float* GPs = smem + L::oGP;
    float* XS = smem + L::oXS;

    // FVP: a converged CG loop (cg_solve.py:19-20); EVAL: a TRPO trial the device line
    // search no longer needs (mjrl_policy_eval_if)
    if ((MODE == FVP || MODE == EVAL) && a.done && *a.done) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    const int np = a.np, m = a.m;
    const int64_t T = a.T;
    const int64_t ntiles = (T + BT - 1) / BT;

    const float* P = a.P;
    const Packed pk(H0, H1, np, MP);
    // per-lane output-column constants for the output layer
    // FWD / EVAL row-pass partials (row_pass), folded at the end of the launch
    double racc0 = 0.0, racc1 = 0.0;
    const float sls = MODE == FVP ? 0.f : ls_sum(P + pk.ls, m);

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row_base = tile * BT;

        // ---------------- phase 1: [BT x N1] = xhat[BT x np] * W^T, K = np ----------------
        floatx4 acc1[S1::NRW][S1::NCW];
        zero_acc(acc1);
        {
            const float* W = (MODE == FVP ? a.V : P) + pk.W0;
            constexpr int NQ = BT * (L::KC / 4);              // float4 pieces of a staged chunk
            constexpr int PER = NQ >= NT ? NQ / NT : 1;
            static_assert(NQ < NT ? NT % NQ == 0 : PER * NT == NQ, "phase-1 staging");
            float4 st[PER];
            const int nch = (np + L::KC - 1) / L::KC;
            auto gload = [&](int c) {
#pragma unroll
                for (int u = 0; u < PER; ++u) {
                    const int idx = tid + u * NT;
                    const int row = idx / (L::KC / 4), c4 = idx % (L::KC / 4);
                    const int col = c * L::KC + c4 * 4;
                    const int64_t gr = row_base + row;
                    st[u] = (idx < NQ && gr < T && col < np) ? *reinterpret_cast<const float4*>(a.xhat + gr * np + col)
                                                 : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            };
            gload(0);
            for (int c = 0; c < nch; ++c) {
                float* xs = XS + (c & 1) * BT * L::LDX;
#pragma unroll
                for (int u = 0; u < PER; ++u) {
                    const int idx = tid + u * NT;
                    const int row = idx / (L::KC / 4), c4 = idx % (L::KC / 4);
                    if (idx < NQ) *reinterpret_cast<float4*>(xs + row * L::LDX + c4 * 4) = st[u];
                }
                __syncthreads();
                if (c + 1 < nch) gload(c + 1);
                const int kb = c * L::KC;
                const int ke = kb + L::KC < np ? kb + L::KC : np;
                gemm_tile(acc1, xs, L::LDX, kb, S1::rb0(w), S1::RBS, RB, W, np, S1::cb0(w), S1::CBS, kb, ke, lane);
            }
            __syncthreads();
        }

        if constexpr (L::LIN) {
            // ---------------- linear policy: phase 1 is the output layer -----------
#pragma unroll
            for (int i = 0; i < S1::NRW; ++i) {
                const int rb = S1::rb0(w) + i * S1::RBS;
                if (rb >= RB) continue;
#pragma unroll
                for (int j = 0; j < S1::NCW; ++j) {
                    const int col = (S1::cb0(w) + j * S1::CBS) * 16 + r16;
                    const float ls = P[pk.ls + col];
                    const float os = a.out_scale ? (col < m ? a.out_scale[col] : 1.f) : 1.f;
                    const float osh = a.out_shift ? (col < m ? a.out_shift[col] : 0.f) : 0.f;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int row = rb * 16 + 4 * q + rr;
                        const float v = acc1[i][j][rr];
                        if (MODE == FVP) {
                            const float sg = expf(ls);
                            const float wq = os * os * (2.f / (2.f * sg * sg + 1e-8f));
                            const float g = col < m ? wq * v : 0.f;
                            const int64_t gr = row_base + row;
                            if (gr < T) a.gp[gr * MP + col] = g;
                        } else {
                            GPs[row * L::LDP + col] = col < m ? v * os + osh : 0.f;
                        }
                    }
                }
            }
        } else {
            // ---------------- epilogue 1 ----------------
#pragma unroll
            for (int i = 0; i < S1::NRW; ++i) {
                const int rb = S1::rb0(w) + i * S1::RBS;
                if (rb >= RB) continue;
#pragma unroll
                for (int j = 0; j < S1::NCW; ++j) {
                    const int col = (S1::cb0(w) + j * S1::CBS) * 16 + r16;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int row = rb * 16 + 4 * q + rr;
                        const int64_t gr = row_base + row;
                        const float v = acc1[i][j][rr];
                        if (MODE == FVP) {
                            const float av = gr < T ? a.a0[gr * H0 + col] : 0.f;
                            D0[row * L::LD0 + col] = (1.f - av * av) * v;
                            A0s[row * L::LD0 + col] = av;
                        } else {
                            const float av = tanh_f(v);
                            A0s[row * L::LD0 + col] = av;
                            if (MODE == FWD && gr < T) a.a0[gr * H0 + col] = av;
                        }
                    }
                }
            }
            __syncthreads();

            // ---------------- phase 2: [BT x H1], K = H0 ----------------
            using S2 = Split<RB, H1 / 16, NW>;
            floatx4 acc2[S2::NRW][S2::NCW];
            zero_acc(acc2);
            if (MODE == FVP) {
                gemm_tile(acc2, D0, L::LD0, 0, S2::rb0(w), S2::RBS, RB, P + pk.W1, H0, S2::cb0(w), S2::CBS, 0, H0,
                          lane);
                gemm_tile(acc2, A0s, L::LD0, 0, S2::rb0(w), S2::RBS, RB, a.V + pk.W1, H0, S2::cb0(w), S2::CBS, 0,
                          H0, lane);
            } else {
                gemm_tile(acc2, A0s, L::LD0, 0, S2::rb0(w), S2::RBS, RB, P + pk.W1, H0, S2::cb0(w), S2::CBS, 0, H0,
                          lane);
            }
            // epilogue 2
#pragma unroll
            for (int i = 0; i < S2::NRW; ++i) {
                const int rb = S2::rb0(w) + i * S2::RBS;
                if (rb >= RB) continue;
#pragma unroll
                for (int j = 0; j < S2::NCW; ++j) {
                    const int col = (S2::cb0(w) + j * S2::CBS) * 16 + r16;
                    const float bias = (MODE == FVP ? a.V : P)[pk.b1 + col];
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int row = rb * 16 + 4 * q + rr;
                        const int64_t gr = row_base + row;
                        const float v = acc2[i][j][rr] + bias;
                        if (MODE == FVP) {
                            const float av = gr < T ? a.a1[gr * H1 + col] : 0.f;
                            D1[row * L::LD1 + col] = (1.f - av * av) * v;
                            A1s[row * L::LD1 + col] = av;
                        } else {
                            const float av = tanh_f(v);
                            A1s[row * L::LD1 + col] = av;
                            if (MODE == FWD && gr < T) a.a1[gr * H1 + col] = av;
                        }
                    }
                }
            }
            __syncthreads();

            // ---------------- phase 3: [BT x MP], K = H1 ----------------
            using S3 = Split<RB, MP / 16, NW>;
            floatx4 acc3[S3::NRW][S3::NCW];
            zero_acc(acc3);
            if (MODE == FVP) {
                gemm_tile(acc3, D1, L::LD1, 0, S3::rb0(w), S3::RBS, RB, P + pk.W2, H1, S3::cb0(w), S3::CBS, 0, H1,
                          lane);
                gemm_tile(acc3, A1s, L::LD1, 0, S3::rb0(w), S3::RBS, RB, a.V + pk.W2, H1, S3::cb0(w), S3::CBS, 0,
                          H1, lane);
            } else {
                gemm_tile(acc3, A1s, L::LD1, 0, S3::rb0(w), S3::RBS, RB, P + pk.W2, H1, S3::cb0(w), S3::CBS, 0, H1,
                          lane);
            }
#pragma unroll
            for (int i = 0; i < S3::NRW; ++i) {
                const int rb = S3::rb0(w) + i * S3::RBS;
                if (rb >= RB) continue;
#pragma unroll
                for (int j = 0; j < S3::NCW; ++j) {
                    const int col = (S3::cb0(w) + j * S3::CBS) * 16 + r16;
                    const float bias = (MODE == FVP ? a.V : P)[pk.b2 + col];
                    const float os = a.out_scale ? (col < m ? a.out_scale[col] : 1.f) : 1.f;
                    const float osh = a.out_shift ? (col < m ? a.out_shift[col] : 0.f) : 0.f;
                    float wq = 0.f;
                    if (MODE == FVP) {
                        const float sg = expf(P[pk.ls + col]);
                        wq = os * os * (2.f / (2.f * sg * sg + 1e-8f));
                    }
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int row = rb * 16 + 4 * q + rr;
                        const float v = acc3[i][j][rr] + bias;
                        if (MODE == FVP) {
                            const float g = col < m ? wq * v : 0.f;
                            GPs[row * L::LDP + col] = g;
                            const int64_t gr = row_base + row;
                            if (gr < T) a.gp[gr * MP + col] = g;
                        } else {
                            GPs[row * L::LDP + col] = col < m ? v * os + osh : 0.f;
                        }
                    }
                }
            }
        }
        __syncthreads();

        // ---------------- per-row pass: log-likelihood, VPG upstream, LR, KL -------------
        if (MODE != FVP) {
            row_pass<MODE, BT, MP, NT, true>(a, P + pk.ls, sls, row_base, GPs, L::LDP, racc0, racc1, tid);
            __syncthreads();
        }

        if constexpr (!L::LIN) {
            if (MODE != EVAL) {
                // ---------------- phase 4: ga1 = g * W2, K = MP ----------------
                using S2 = Split<RB, H1 / 16, NW>;
                floatx4 acc4[S2::NRW][S2::NCW];
                zero_acc(acc4);
                gemm_tile(acc4, GPs, L::LDP, 0, S2::rb0(w), S2::RBS, RB, P + pk.W2T, MP, S2::cb0(w), S2::CBS, 0, MP,
                          lane);
#pragma unroll
                for (int i = 0; i < S2::NRW; ++i) {
                    const int rb = S2::rb0(w) + i * S2::RBS;
                    if (rb >= RB) continue;
#pragma unroll
                    for (int j = 0; j < S2::NCW; ++j) {
                        const int col = (S2::cb0(w) + j * S2::CBS) * 16 + r16;
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) {
                            const int row = rb * 16 + 4 * q + rr;
                            const float av = A1s[row * L::LD1 + col];
                            const float g = (1.f - av * av) * acc4[i][j][rr];
                            D1[row * L::LD1 + col] = g;
                            const int64_t gr = row_base + row;
                            if (gr < T) a.gu1[gr * H1 + col] = g;
                        }
                    }
                }
                __syncthreads();
                // ---------------- phase 5: ga0 = gu1 * W1, K = H1 ----------------
                floatx4 acc5[S1::NRW][S1::NCW];
                zero_acc(acc5);
                gemm_tile(acc5, D1, L::LD1, 0, S1::rb0(w), S1::RBS, RB, P + pk.W1T, H1, S1::cb0(w), S1::CBS, 0, H1,
                          lane);
#pragma unroll
                for (int i = 0; i < S1::NRW; ++i) {
                    const int rb = S1::rb0(w) + i * S1::RBS;
                    if (rb >= RB) continue;
#pragma unroll
                    for (int j = 0; j < S1::NCW; ++j) {
                        const int col = (S1::cb0(w) + j * S1::CBS) * 16 + r16;
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) {
                            const int row = rb * 16 + 4 * q + rr;
                            const float av = A0s[row * L::LD0 + col];
                            const int64_t gr = row_base + row;
                            if (gr < T) a.gu0[gr * H0 + col] = (1.f - av * av) * acc5[i][j][rr];
                        }
                    }
                }
                __syncthreads();
            }
        }
    }

    if (MODE != FVP) {
        static_assert(L::total >= 2 * NT, "row_pass_final scratch");
        __syncthreads();
        row_pass_final<MODE, MP, NT>(racc0, racc1, reinterpret_cast<double*>(smem), a.rpart, blockIdx.x, tid);
    }
}

}  // namespace
