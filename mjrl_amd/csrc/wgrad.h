// wgrad.h — the weight gradients of the k_rows path, split-K over timesteps
// (included by policy.hip after rows.h):
//   k_wgrad       G^T A per layer, one workgroup per 64 x 64 output block and row
//                 slice (bias gradients ride along: the obs bias column / column
//                 sums); slabs in the per-job layout of make_jobs (k_gather)
//   k_wgrad_all   all three products of a row slice in one workgroup; slabs in the
//                 flat chunk-major layout (k_gather_flat)
#pragma once

namespace {

// ---------------------------------------------------------------------------
// Weight gradients: C[N][K] = sum_t G[t][n] * A[t][k], split over T into S slices.
// ---------------------------------------------------------------------------
struct WJob {
    const float* G;
    const float* A;
    int ldg, lda, N, K;
    int nbN, nbK, bias;
    int64_t off;    // float offset of slice 0's [N][K] slab in wpart
    int64_t boff;   // float offset of slice 0's [N] bias slab
};

struct WArgs {
    WJob job[3];
    int njobs;
    int start[4];   // prefix sums of blocks per slice per job
    int S;
    int64_t T;
    int64_t rows_per_slice;
    float* wpart;
    const int32_t* done;
    int64_t wcap;   // floats of the scratch's slabs (MJRL_SLAB_CHECK)
};

constexpr int WB = 64;        // output block edge
constexpr int WT = 64;        // rows per staged tile
constexpr int WLD = WB + 16;  // LDS row stride (floats): rows 4 apart land 16 banks apart

// (A split-f16 version — transposed LDS tiles, per-(32-row step, column) scales —
// measured slower: HalfCheetah 87 -> 126 us, door 94 -> 134 us per launch, from
// the transposing LDS writes and the per-step splits; profiles/r03g/rejected/.)
__global__ void __launch_bounds__(NTHREADS, 2) k_wgrad(WArgs a) {
    if (a.done && *a.done) return;
    __shared__ __attribute__((aligned(16))) float Gs[WT * WLD];
    __shared__ __attribute__((aligned(16))) float As[WT * WLD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    const int jb = blockIdx.x / a.S, s = blockIdx.x % a.S;
    int ji = 0;
    while (ji + 1 < a.njobs && jb >= a.start[ji + 1]) ++ji;
    const WJob& J = a.job[ji];
    const int local = jb - a.start[ji];
    const int nb = local / J.nbK, kb = local % J.nbK;
    const int n0 = nb * WB, k0 = kb * WB;
    const int64_t r0 = (int64_t)s * a.rows_per_slice;
    int64_t r1 = r0 + a.rows_per_slice;
    if (r1 > a.T) r1 = a.T;

    floatx4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = zero4();
    double bsum = 0.0;
    const bool do_bias = J.bias && kb == 0;

    // staging: 64 rows x 64 cols of G and of A = 1024 float4 each, 4 per thread
    float4 g4[4], a4[4];
    auto gload = [&](int64_t t0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + u * NTHREADS;
            const int row = idx >> 4, c4 = (idx & 15) * 4;
            const int64_t t = t0 + row;
            const bool rv = t < r1;
            g4[u] = (rv && n0 + c4 < J.N) ? *reinterpret_cast<const float4*>(J.G + t * J.ldg + n0 + c4)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
            a4[u] = (rv && k0 + c4 < J.K) ? *reinterpret_cast<const float4*>(J.A + t * J.lda + k0 + c4)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    if (r0 < r1) gload(r0);
    for (int64_t t0 = r0; t0 < r1; t0 += WT) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + u * NTHREADS;
            const int row = idx >> 4, c4 = (idx & 15) * 4;
            *reinterpret_cast<float4*>(Gs + row * WLD + c4) = g4[u];
            *reinterpret_cast<float4*>(As + row * WLD + c4) = a4[u];
        }
        __syncthreads();
        if (t0 + WT < r1) gload(t0 + WT);
        if (n0 + 16 * w < J.N) {
#pragma unroll 4
            for (int tt = 0; tt < WT; tt += 4) {
                const float ga = Gs[(tt + q) * WLD + 16 * w + r16];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float ab = As[(tt + q) * WLD + 16 * i + r16];
                    acc[i] = mfma4(ga, ab, acc[i]);
                }
            }
        }
        if (do_bias && tid < WB) {
            double cs = 0.0;
            for (int row = 0; row < WT; ++row) cs += (double)Gs[row * WLD + tid];
            bsum += cs;
        }
    }
    // write this slice's partial block
    float* out = a.wpart + J.off + (int64_t)s * J.N * J.K;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + 16 * i + r16;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int n = n0 + 16 * w + 4 * q + rr;
            if (n < J.N && k < J.K) {
                MJRL_SLAB_CHECK(J.off + (int64_t)s * J.N * J.K + (int64_t)n * J.K + k, a.wcap);
                out[(int64_t)n * J.K + k] = acc[i][rr];
            }
        }
    }
    if (do_bias && tid < WB && n0 + tid < J.N) {
        MJRL_SLAB_CHECK(J.boff + (int64_t)s * J.N + n0 + tid, a.wcap);
        a.wpart[J.boff + (int64_t)s * J.N + n0 + tid] = (float)bsum;
    }
}

// ---------------------------------------------------------------------------
// All three weight gradients of one row slice in ONE workgroup (MLP, H0 = H1 = H):
//   gW0[H][NP] += gu0^T xhat,  gW1[H][H] += gu1^T a0 (+ gb1),  gW2[MP][H] += gp^T a1 (+ gb2)
// k_wgrad gives each 64 x 64 output block its own workgroup, so every row tile of
// gu1 / a0 / ... is fetched once per block that reads it (HalfCheetah: 2x the
// bytes it needs, and half the CUs at its 128 slices).  Here a workgroup stages
// each row tile of the six inputs into LDS once (register prefetch of the next
// tile under this tile's MFMAs) and every output block of all three products is
// an accumulator in some wave: wave w owns the 16-row strips w + NW t of gW1 and
// gW0 (a strip's gu fragment feeds all its column blocks) and BW2 blocks of gW2.
// Slabs in the flat chunk-major layout of k_kx (k_gather_flat), fixed order.
// ---------------------------------------------------------------------------
__host__ __device__ constexpr int wall_ld(int w) {   // LDS row stride: w <= ld, ld % 64 in {16, 48}
    return (w % 64 == 0) ? w + 16 : (w % 64 <= 16 ? w - w % 64 + 16 : (w % 64 <= 48 ? w - w % 64 + 48 : w - w % 64 + 80));
}

// v where c holds, else zero, component by component (a select of the whole float4
// made the compiler select between two stack addresses and reload through scratch)
__device__ __forceinline__ float4 sel4(bool c, float4 v) {
    return make_float4(c ? v.x : 0.f, c ? v.y : 0.f, c ? v.z : 0.f, c ? v.w : 0.f);
}

template <int H, int MP, int NPBM>
struct WallCfg {
    static constexpr int NW = H / 16 < 8 ? H / 16 : 8;   // waves
    static constexpr int NT = 64 * NW;
    static constexpr int SPW = (H / 16) / NW;            // gW1 / gW0 strips per wave
    static constexpr int BW2 = (MP / 16) * (H / 16) / NW;   // gW2 blocks per wave
    static constexpr int BT = 32;                        // rows per staged tile
    static constexpr int LDH = wall_ld(H), LDP = wall_ld(MP), LDX = wall_ld(16 * NPBM);
    static constexpr int oG0 = 0, oG1 = oG0 + BT * LDH, oGP = oG1 + BT * LDH, oX = oGP + BT * LDP,
                         oA0 = oX + BT * LDX, oA1 = oA0 + BT * LDH, total = oA1 + BT * LDH;
    static constexpr int bytes = total * 4;
};

struct WallArgs {
    const float *gu0, *gu1, *gp, *x, *a0, *a1;
    int n, m, np, S;
    int64_t T, rows_per_slice;
    float* wpart;   // flat slab layout (k_gather_flat)
    const int32_t* done;
    int64_t wcap;   // floats of the scratch's slabs (MJRL_SLAB_CHECK)
};

// PART 0: all three products (the kernel below); 1: gW1 + gb1 only, 2: gW0, gW2 + gb2
// only (the two-workgroups-per-slice split measured for 256-wide layers, not used)
template <int H, int MP, int NPBM, int PART>
__device__ __forceinline__ void wall_body(const WallArgs& a, int s, float* sm) {
    using C = WallCfg<H, MP, NPBM>;
    constexpr int BT = C::BT, NW = C::NW, SPW = C::SPW, BW2 = C::BW2, HB = H / 16;
    constexpr bool J1 = PART != 2, J02 = PART != 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    const int np = a.np, npb = np / 16;
    const int64_t r0 = (int64_t)s * a.rows_per_slice;
    const int64_t r1 = r0 + a.rows_per_slice < a.T ? r0 + a.rows_per_slice : a.T;

    // Staging of a tile: every load unconditional (rows past the slice clamped to its
    // last row, masked to zero when stored to LDS; surplus threads of the narrow gp /
    // x pieces re-read a valid piece and store nothing), so no load sits under a
    // branch and none waits for another (in-order vmcnt; a branchy per-piece decode
    // measured 114 vs 87 us for k_wgrad).  H-wide inputs: PH float4 per thread, a
    // compile-time row / column decode.
    constexpr int PH = BT * H / 4 / C::NT;   // float4 per thread of one H-wide input
    static_assert(PH * C::NT == BT * H / 4, "H-wide staging");
    constexpr int QP = BT * MP / 4, PP = (QP + C::NT - 1) / C::NT;                // gp pieces
    constexpr int PX = (BT * 16 * NPBM / 4 + C::NT - 1) / C::NT;               // x pieces (np <= 16 NPBM)
    const int qx = BT * np / 4;
    int prow[PP], pc4[PP], xrow[PX], xc4[PX];
#pragma unroll
    for (int u = 0; u < PP; ++u) {
        const int i = tid + u * C::NT, ic = i < QP ? i : QP - 1;
        prow[u] = ic / (MP / 4);
        pc4[u] = ic % (MP / 4);
    }
#pragma unroll
    for (int u = 0; u < PX; ++u) {
        const int i = tid + u * C::NT, ic = i < qx ? i : qx - 1;
        xrow[u] = ic / (np / 4);
        xc4[u] = ic % (np / 4);
    }
    struct Stage {
        float4 g0[PH], g1[PH], a0[PH], a1[PH], p[PP], x[PX];
    };
    Stage stA;
    auto hload = [&](float4 (&dst)[PH], const float* src, int64_t t0) __attribute__((always_inline)) {
        const int64_t tl = r1 - 1;
#pragma unroll
        for (int u = 0; u < PH; ++u) {
            const int i = tid + u * C::NT, row = i / (H / 4), c4 = i % (H / 4);
            const int64_t t = t0 + row < tl ? t0 + row : tl;
            dst[u] = *reinterpret_cast<const float4*>(src + t * H + 4 * c4);
        }
    };
    auto hstore = [&](const float4 (&v)[PH], int off, int64_t t0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PH; ++u) {
            const int i = tid + u * C::NT, row = i / (H / 4), c4 = i % (H / 4);
            *reinterpret_cast<float4*>(sm + off + row * C::LDH + 4 * c4) = sel4(t0 + row < r1, v[u]);
        }
    };
    auto gload = [&](Stage& st, int64_t t0) __attribute__((always_inline)) {
        const int64_t tl = r1 - 1;
        if constexpr (J02) hload(st.g0, a.gu0, t0);
        if constexpr (J1) hload(st.g1, a.gu1, t0);
        if constexpr (J1) hload(st.a0, a.a0, t0);
        if constexpr (J02) hload(st.a1, a.a1, t0);
        if constexpr (J02) {
#pragma unroll
            for (int u = 0; u < PP; ++u) {
                const int64_t tp = t0 + prow[u] < tl ? t0 + prow[u] : tl;
                st.p[u] = *reinterpret_cast<const float4*>(a.gp + tp * MP + 4 * pc4[u]);
            }
#pragma unroll
            for (int u = 0; u < PX; ++u) {
                const int64_t tx = t0 + xrow[u] < tl ? t0 + xrow[u] : tl;
                st.x[u] = *reinterpret_cast<const float4*>(a.x + tx * np + 4 * xc4[u]);
            }
        }
    };
    auto sstore = [&](const Stage& st, int64_t t0) __attribute__((always_inline)) {
        if constexpr (J02) hstore(st.g0, C::oG0, t0);
        if constexpr (J1) hstore(st.g1, C::oG1, t0);
        if constexpr (J1) hstore(st.a0, C::oA0, t0);
        if constexpr (J02) hstore(st.a1, C::oA1, t0);
        if constexpr (J02) {
#pragma unroll
            for (int u = 0; u < PP; ++u)
                if (tid + u * C::NT < QP)
                    *reinterpret_cast<float4*>(sm + C::oGP + prow[u] * C::LDP + 4 * pc4[u]) = sel4(t0 + prow[u] < r1, st.p[u]);
#pragma unroll
            for (int u = 0; u < PX; ++u)
                if (tid + u * C::NT < qx)
                    *reinterpret_cast<float4*>(sm + C::oX + xrow[u] * C::LDX + 4 * xc4[u]) = sel4(t0 + xrow[u] < r1, st.x[u]);
        }
    };

    constexpr int S1 = J1 ? SPW : 0, S0 = J02 ? SPW : 0, B2 = J02 ? BW2 : 0;
    floatx4 acc1[S1 ? S1 : 1][HB], acc0[S0 ? S0 : 1][NPBM], acc2[B2 ? B2 : 1];
#pragma unroll
    for (int t = 0; t < SPW; ++t) {
#pragma unroll
        for (int kb = 0; kb < HB; ++kb) acc1[t < S1 ? t : 0][kb] = zero4();
#pragma unroll
        for (int kb = 0; kb < NPBM; ++kb) acc0[t < S0 ? t : 0][kb] = zero4();
    }
#pragma unroll
    for (int b = 0; b < BW2; ++b) acc2[b < B2 ? b : 0] = zero4();
    double bsum = 0.0;   // thread c < H: gb1[c]; H <= c < H + MP: gb2[c - H]
    const bool bias_thr = (J1 && tid < H) || (J02 && tid >= H && tid < H + MP);

    // One k-step's operands (4 rows): read from LDS one k-step ahead of the MFMAs that
    // use them (the scheduler otherwise waited on each read right before its MFMA).
    struct Ops {
        float av[J1 ? HB : 1], g1[S1 ? S1 : 1], xv[NPBM], g0[S0 ? S0 : 1], gp[B2 ? B2 : 1], a1[B2 ? B2 : 1];
    };
    auto rd = [&](Ops& o, int kk) __attribute__((always_inline)) {
        const int row = 4 * kk + q;
        if constexpr (J1) {
#pragma unroll
            for (int kb = 0; kb < HB; ++kb) o.av[kb] = sm[C::oA0 + row * C::LDH + 16 * kb + r16];
#pragma unroll
            for (int t = 0; t < S1; ++t) o.g1[t] = sm[C::oG1 + row * C::LDH + 16 * (w + NW * t) + r16];
        }
        if constexpr (J02) {
#pragma unroll
            for (int kb = 0; kb < NPBM; ++kb) o.xv[kb] = kb < npb ? sm[C::oX + row * C::LDX + 16 * kb + r16] : 0.f;
#pragma unroll
            for (int t = 0; t < S0; ++t) o.g0[t] = sm[C::oG0 + row * C::LDH + 16 * (w + NW * t) + r16];
#pragma unroll
            for (int b = 0; b < B2; ++b) {
                const int blk = w * BW2 + b, sb = blk / HB, kb = blk % HB;
                o.gp[b] = sm[C::oGP + row * C::LDP + 16 * sb + r16];
                o.a1[b] = sm[C::oA1 + row * C::LDH + 16 * kb + r16];
            }
        }
    };
    auto mm = [&](const Ops& o) __attribute__((always_inline)) {
        if constexpr (J1) {
#pragma unroll
            for (int t = 0; t < S1; ++t)
#pragma unroll
                for (int kb = 0; kb < HB; ++kb) acc1[t][kb] = mfma4(o.g1[t], o.av[kb], acc1[t][kb]);
        }
        if constexpr (J02) {
#pragma unroll
            for (int t = 0; t < S0; ++t)
#pragma unroll
                for (int kb = 0; kb < NPBM; ++kb)
                    if (kb < npb) acc0[t][kb] = mfma4(o.g0[t], o.xv[kb], acc0[t][kb]);
#pragma unroll
            for (int b = 0; b < B2; ++b) acc2[b] = mfma4(o.gp[b], o.a1[b], acc2[b]);
        }
    };
    constexpr bool PIPE = SPW * (HB + NPBM) + BW2 <= 11;   // a second operand set fits the registers
    auto tile = [&]() __attribute__((always_inline)) {
        Ops o0, o1;
        if constexpr (PIPE) {
            rd(o0, 0);
#pragma unroll   // fully: a rolled loop's induction registers took prefetch registers (copies waiting on HBM)
            for (int kk = 0; kk < BT / 4; kk += 2) {
                rd(o1, kk + 1);
                __builtin_amdgcn_sched_barrier(0);
                mm(o0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 2 < BT / 4) rd(o0, kk + 2);
                __builtin_amdgcn_sched_barrier(0);
                mm(o1);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < BT / 4; ++kk) {
                rd(o0, kk);
                mm(o0);
            }
        }
        if (bias_thr) {   // bias sums: rows in order, fp64 (the LDS reads batched ahead of the adds)
            const float* col = tid < H ? sm + C::oG1 + tid : sm + C::oGP + (tid - H);
            const int ld = tid < H ? C::LDH : C::LDP;
            double cs = 0.0;
#pragma unroll
            for (int rb = 0; rb < BT; rb += 8) {   // eight reads in flight at a time
                float v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = col[(rb + r) * ld];
#pragma unroll
                for (int r = 0; r < 8; ++r) cs += (double)v[r];
            }
            bsum += cs;
        }
    };
    // one tile of register prefetch under the current tile's MFMAs (a second stage
    // measured no faster: 71.6 vs 71.3 us; its registers hold the next k-step's
    // operands instead)
    if (r0 < r1) gload(stA, r0);
    for (int64_t t0 = r0; t0 < r1; t0 += BT) {
        __syncthreads();
        sstore(stA, t0);
        __syncthreads();
        gload(stA, t0 + BT);   // unconditional (rows clamped): a branch made the compiler copy prefetch registers at the join, waiting on HBM
        tile();
    }
    // this slice's slab in the flat, parameter-chunk-major layout of k_kx:
    // wpart[f / 64][S][64] for flat parameter f (reference order W0, b0, W1, b1, W2, b2,
    // gaussian_mlp.py:61-64), so k_gather_flat folds each 64-parameter chunk from one
    // contiguous run; padded columns / rows are not stored
    const int n = a.n, m = a.m;
    const int fb0 = H * n, fW1 = fb0 + H, fb1 = fW1 + H * H, fW2 = fb1 + H, fb2 = fW2 + m * H;
    float* wp = a.wpart + (int64_t)s * 64;
    const int64_t cs = (int64_t)a.S * 64;
    auto put = [&](int f, float v) {
        MJRL_SLAB_CHECK((int64_t)s * 64 + (int64_t)(f >> 6) * cs + (f & 63), a.wcap);
        wp[(int64_t)(f >> 6) * cs + (f & 63)] = v;
    };
    if constexpr (J1) {
#pragma unroll
        for (int t = 0; t < S1; ++t) {
            const int n0 = 16 * (w + NW * t) + 4 * q;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int j = n0 + rr;
                if constexpr (H % 64 == 0) {
                    // fW1 = H (n + 1) is a multiple of 64: row j of gW1 is H / 64 whole chunks,
                    // so column k lands in chunk fW1 / 64 + j H / 64 + k / 64 at k % 64 (one
                    // address per row, immediate offsets for the 16-column steps)
                    float* rowp = wp + (int64_t)((fW1 >> 6) + j * (H / 64)) * cs + r16;
#pragma unroll
                    for (int kb = 0; kb < HB; ++kb) {
                        MJRL_SLAB_CHECK((rowp - a.wpart) + (kb >> 2) * cs + 16 * (kb & 3), a.wcap);
                        rowp[(kb >> 2) * cs + 16 * (kb & 3)] = acc1[t][kb][rr];
                    }
                } else {
#pragma unroll
                    for (int kb = 0; kb < HB; ++kb) put(fW1 + j * H + 16 * kb + r16, acc1[t][kb][rr]);
                }
            }
        }
        if (tid < H) put(fb1 + tid, (float)bsum);
    }
    if constexpr (J02) {
#pragma unroll
        for (int t = 0; t < S0; ++t) {
            const int n0 = 16 * (w + NW * t) + 4 * q;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                for (int kb = 0; kb < NPBM; ++kb) {
                    const int k = 16 * kb + r16, h = n0 + rr;
                    if (k < n) put(h * n + k, acc0[t][kb][rr]);
                    else if (k == n) put(fb0 + h, acc0[t][kb][rr]);   // the bias column: b0
                }
        }
#pragma unroll
        for (int b = 0; b < B2; ++b) {
            const int blk = w * BW2 + b, sb = blk / HB, kb = blk % HB;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int j = 16 * sb + 4 * q + rr;
                if (j < m) put(fW2 + j * H + 16 * kb + r16, acc2[b][rr]);
            }
        }
        if (tid >= H && tid < H + m) put(fb2 + (tid - H), (float)bsum);
    }
}

template <int H, int MP, int NPBM>
__global__ void __launch_bounds__((WallCfg<H, MP, NPBM>::NT)) k_wgrad_all(WallArgs a) {
    if (a.done && *a.done) return;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    wall_body<H, MP, NPBM, 0>(a, blockIdx.x, sm);
}

}  // namespace
