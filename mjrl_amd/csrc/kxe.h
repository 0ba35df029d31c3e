// kxe.h — the EVAL pass of k_kx (kx.h) with the first layer of the next tile run
// under this tile's chain, included by policy.hip after kx.h.
//
// The serial EVAL tile is publish -> P1 -> fold -> P2 -> P3 -> row pass: the part
// that streams and multiplies the 48 KB xhat tile (publish + P1, LDS bandwidth and
// MFMA issue) and a barrier-separated latency chain with 9 MFMAs per wave, one
// after the other.  EVAL keeps no weight-gradient accumulators and needs none of
// the backward buffers, so it has the registers and the LDS for a second tile in
// flight.  Here, while tile t runs its chain, the same waves
//   - store tile t+1's register-staged xhat pieces into the other of two image
//     buffers (before the fold barrier), then issue tile t+2's HBM loads in two
//     halves under the two tanh intervals;
//   - run tile t+1's P1 products in groups of k32 steps, one group per barrier
//     interval of the chain (tanh / P2 / P3 / row pass; MJRL_KXE_SPLIT: most of them
//     under the row pass, whose shuffle and divide chains leave the most room), into
//     acc1 of tile t+1, which stays in registers until its own fold at the top of the
//     next iteration.
// P1 keeps the serial order of k-steps into the same accumulators and every other
// expression is the serial kernel's, so every output is bit-identical to
// k_kx<MP, KG, EVAL>.  The two image buffers let the last P1 group sit in the row
// pass interval while faster waves already publish the tile after it, so the
// barrier after the row pass is gone: four barriers per tile instead of six.
// A workgroup's last iteration multiplies an all-zero image (its tile t+1 does
// not exist: xload returns zeros): no branch around the products, whose loads
// would make the compiler's waits conservative (kx.h, comment at xload).
#pragma once

namespace {

// P1 k-steps per chain interval (tanh, P2, P3, row pass), in sixths of the KS steps
// (1M-row Humanoid eval pass: 1,2,1,2 512 us, 2,1,1,2 506 us, 1,1,1,3 490 us; serial 547 us)
#ifndef MJRL_KXE_SPLIT
#define MJRL_KXE_SPLIT 1, 1, 1, 3
#endif
template <int MP, int KG>
struct XELayout {
    static constexpr int H = 64, BT = 32;
    static constexpr int NP = 32 * KG, KH = NP / 2;
    static constexpr int RBYTES = NP * 2;          // one f16 row of an xhat hi / lo image
    static constexpr int XIMG = BT * RBYTES;       // one xhat image (hi or lo)
    static constexpr int LD = H + 4;               // f32 [row][LD] buffers
    static constexpr int LDG = 32 + 4;             // GPf [row][LDG]
    static constexpr int WIMG = 64 * 128;
    static constexpr int WIMG2 = 32 * 128;
    static constexpr int AIMG = AIMG_BYTES;
    // byte offsets
    static constexpr int oX = 0;                       // two buffers of (hi, lo)
    static constexpr int oS1 = oX + 4 * XIMG;          // W1r: hi, lo
    static constexpr int oS3 = oS1 + 2 * WIMG;         // W2r: hi, lo
    static constexpr int oSC = oS3 + 2 * WIMG2;        // f32 inverse scales: s1[64] s3[32]
    static constexpr int oU = oSC + (64 + 32) * 4;     // two xhat row-scale arrays [BT]
    static constexpr int oD0 = oU + 2 * BT * 4;        // f32 [BT][LD]: the fold's partner halves
    static constexpr int oGP = oD0 + BT * LD * 4;      // f32 [BT][LDG]
    static constexpr int oA0 = oGP + BT * LDG * 4;     // a0 image hi, lo
    static constexpr int oA1 = oA0 + 2 * AIMG;         // a1 image hi, lo
    static constexpr int bytes = oA1 + 2 * AIMG;
    static_assert(bytes <= 160 * 1024, "LDS");
    static_assert(bytes >= 2 * KT * 8, "row_pass_final scratch");
    static constexpr int XPER = BT * NP / 4 / KT;
    static constexpr int KS = KH / 32;                 // k32 steps per observation half
    static_assert(NP % 128 == 0, "chunk swizzle of the xhat images");
    static_assert(MP == 16 || MP == 32, "output layer: one k32 step");
    // first k-step of interval i (0 .. 3), KS for i = 4
    static constexpr int step0(int i) {
        constexpr int c[4] = {MJRL_KXE_SPLIT};
        static_assert(c[0] + c[1] + c[2] + c[3] == 6, "MJRL_KXE_SPLIT: sixths");
        int cum = 0;
        for (int k = 0; k < i; ++k) cum += c[k];
        return (KS * cum + 3) / 6;
    }
    // the most k-steps in one interval
    static constexpr int gmax() {
        int g = 1;
        for (int i = 0; i < 4; ++i) g = step0(i + 1) - step0(i) > g ? step0(i + 1) - step0(i) : g;
        return g;
    }
};

template <int MP, int KG>
__global__ void __launch_bounds__(KT, 1) k_kx_eval_pipe(RowArgs a) {
    // as k_kx: multiply-add chains contract to FMA (the same expressions, the same bits)
#pragma clang fp contract(fast)
    using L = XELayout<MP, KG>;
    constexpr int H = 64, BT = L::BT, NP = L::NP, KH = L::KH, KS = L::KS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* sb = reinterpret_cast<char*>(smem);
    char* S1 = sb + L::oS1;
    char* S3 = sb + L::oS3;
    float* sc1 = reinterpret_cast<float*>(sb + L::oSC);
    float* sc3 = sc1 + 64;
    float* Us2 = reinterpret_cast<float*>(sb + L::oU);
    float* D0 = reinterpret_cast<float*>(sb + L::oD0);
    float* GPf = reinterpret_cast<float*>(sb + L::oGP);
    char* A0i = sb + L::oA0;
    char* A1i = sb + L::oA1;

#ifdef MJRL_KX_PROF
    const unsigned long long kx_t0_ = __builtin_amdgcn_s_memtime();
    unsigned long long kx_pre_[6];
#endif
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    const int cb = w & 3, kh = w >> 2;
    const int m = a.m;
    const int64_t T = a.T;
    const int64_t ntiles = (T + BT - 1) / BT;
    const int64_t G = gridDim.x;
    const float* P = a.P;
    const Packed pk(H, H, NP, MP);

    // ---- launch preamble (k_kx's, EVAL): W1r / W2r images, this wave's W0 slice ----
    static_assert(KT == 512 && MP <= 32, "preamble layout: 8 waves, output-layer images of 32 rows");
    const float8v rv1 = wload_rows<64>(P + pk.W1, H, tid);
    const float8v rv2 = wload_rows<32>(P + pk.W2, MP, tid);
    const float bias1 = P[pk.b1 + cb * 16 + r16];
    const int cbo3 = w & (MP / 16 - 1), rb3 = w / (MP / 16);   // P3: waves < 2 * MP/16
    const int col3 = cbo3 * 16 + r16;
    const float bias3 = P[pk.b2 + col3];
    const float os3 = a.out_scale ? (col3 < m ? a.out_scale[col3] : 1.f) : 1.f;
    const float osh3 = a.out_shift ? (col3 < m ? a.out_shift[col3] : 0.f) : 0.f;
    const float sls = ls_sum(P + pk.ls, m);
    const RowConst rconst = row_const<EVAL, MP>(a, P + pk.ls, tid);
    KX_PRE(0);
    half8 wh[KS], wl[KS];
    float wsc;
    {
        float8v v[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k0 = kh * KH + 32 * s + 8 * q;
            v[s] = load8(P + pk.W0 + (cb * 16 + r16) * NP + k0) * load8(a.xc + k0);
        }
        float mx = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) mx = fmaxf(mx, absmax8(v[s]));
        const float sc = pow2_scale(max_over_groups(mx), wsc);
#pragma unroll
        for (int s = 0; s < KS; ++s) split8(v[s], sc, wh[s], wl[s]);
    }
    KX_PRE(1);
    wrows_store<64>(rv1, S1, L::WIMG, sc1, tid);
    wrows_store<32>(rv2, S3, L::WIMG2, sc3, tid);
    KX_PRE(2);
    KX_PRE(3);
    KX_PRE(4);
    // a TRPO trial the device line search no longer needs (mjrl_policy_eval_if)
    if (a.done && *a.done) return;

    double racc0 = 0.0, racc1 = 0.0;
    float touch[2] = {0.f, 0.f};
    // the xhat pieces of one tile in registers (kx.h xload: conditional loads, zeros
    // for a tile or rows that do not exist)
    float4 xn[L::XPER];
    float un = 1.f;
    // pieces u0 .. u1 - 1 (the tile loop issues the 48 KB of a tile in two parts, under
    // the two tanh intervals, whose VALU work leaves the vector-memory path idle: issued
    // in one go they held the publish interval for ~700 cycles)
    auto xload = [&](int64_t t_, int u0 = 0, int u1 = L::XPER) {
        const int64_t rb_ = t_ * BT;
        const int row = tid >> 4, c16 = tid & 15;
        const bool ok = t_ < ntiles && rb_ + row < T;
        const char* src = reinterpret_cast<const char*>(a.xs) + (ok ? (rb_ + row) * (4 * NP) : 0);
#pragma unroll
        for (int u = 0; u < L::XPER; ++u)
            if (u >= u0 && u < u1)
                xn[u] = ok ? *reinterpret_cast<const float4*>(src + 16 * (c16 + 16 * u)) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (u0 == 0) {
            const bool uok = tid < BT && t_ < ntiles && rb_ + tid < T;
            un = a.xu[uok ? rb_ + tid : 0];
        }
    };
    // the pieces in registers -> image buffer b (hi, lo) and its row scales
    auto publish = [&](int b) {
        const int row = tid >> 4, c16 = tid & 15;
        char* dst = sb + L::oX + b * (2 * L::XIMG) + row * L::RBYTES + 16 * (c16 ^ chunk_swz(row));
#pragma unroll
        for (int u = 0; u < L::XPER; ++u) {
            constexpr int UH = NP / 128;
            *reinterpret_cast<float4*>(dst + (u / UH) * L::XIMG + 256 * (u % UH)) = xn[u];
        }
        if (tid < BT) Us2[b * BT + tid] = un;
    };
    // P1's image offsets as in k_kx: (row r16, chunk kh*KH/8 + 4s + q, swizzled)
    const int p1A = 16 * (kh * (KH / 8) + q), p1B = 16 * chunk_swz(r16), p1C = r16 * L::RBYTES;
    // k-steps s0 .. s1 - 1 of the first layer over image buffer b, this wave's
    // observation half, in two parts: the operand reads into registers (issued at the
    // start of a chain interval, right after the chain's own reads, so their LDS
    // latency and bandwidth run under the chain) and the products (the serial order
    // of k-steps into the same accumulators)
    constexpr int GMAX = L::gmax();
    auto p1_load = [&](int b, int s0, int s1, half8 (&xh)[GMAX][2], half8 (&xl)[GMAX][2]) __attribute__((always_inline)) {
        const char* XH = sb + L::oX + b * (2 * L::XIMG);
#pragma unroll
        for (int s = 0; s < KS; ++s)
            if (s >= s0 && s < s1) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int off = ((p1A + 64 * s) ^ p1B) + p1C + i * 16 * L::RBYTES;
                    xh[s - s0][i] = *reinterpret_cast<const half8*>(XH + off);
                    xl[s - s0][i] = *reinterpret_cast<const half8*>(XH + L::XIMG + off);
                }
            }
    };
    auto p1_mma = [&](int s0, int s1, const half8 (&xh)[GMAX][2], const half8 (&xl)[GMAX][2], floatx4 (&acc)[2])
        __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
            if (s >= s0 && s < s1) {
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i] = mfma_x3(xh[s - s0][i], xl[s - s0][i], wh[s], wl[s], acc[i]);
            }
    };
    auto p1_steps = [&](int b, int s0, int s1, floatx4 (&acc)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int g0 = 0; g0 < KS; g0 += GMAX) {
            half8 xh[GMAX][2], xl[GMAX][2];
            const int lo = g0 > s0 ? g0 : s0, hi = g0 + GMAX < s1 ? g0 + GMAX : s1;
            p1_load(b, lo, hi, xh, xl);
            p1_mma(lo, hi, xh, xl, acc);
        }
    };
    auto p1_scale = [&](int b, floatx4 (&acc)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) acc[i][rr] *= Us2[b * BT + i * 16 + 4 * q + rr] * wsc;
    };

    // ---- prologue: the first tile's publish and whole first layer ----
    xload(blockIdx.x);
    __syncthreads();   // images and scales ready
    publish(0);
    xload(blockIdx.x + G);
    __syncthreads();
    floatx4 acc1[2] = {zero4(), zero4()};   // the current tile's first-layer partials
    p1_steps(0, 0, KS, acc1);
    p1_scale(0, acc1);
#ifdef MJRL_KX_PROF
    unsigned long long kx_acc_[KX_NPROF] = {0};
    unsigned long long kx_last_ = __builtin_amdgcn_s_memtime();
    kx_acc_[15] = kx_last_ - kx_t0_;
    kx_acc_[17] = 1;
    kx_acc_[18] = kx_pre_[0] - kx_t0_;
    for (int i = 1; i < 5; ++i) kx_acc_[18 + i] = kx_pre_[i] - kx_pre_[i - 1];
    kx_acc_[23] = kx_last_ - kx_pre_[4];
#endif

    int nb = 1;   // the image buffer tile t+1 goes to (wave-uniform)
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += G) {
        KX_STAMP(9);   // loop top
        const int64_t row_base = tile * BT;

        // ---- fold store of tile t; publish of tile t+1; loads ----
        // No barrier since the previous row pass: D0 was last read two barriers back,
        // image buffer nb and its scales by the P1 groups of the iteration before the
        // previous one (the previous one read the other buffer).
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            D0[((1 - kh) * 16 + 4 * q + rr) * L::LD + cb * 16 + r16] = kh ? acc1[0][rr] : acc1[1][rr];
        asm volatile("" ::"v"(touch[0]), "v"(touch[1]));
        publish(nb);
        {
            // pull tile t+1's per-row inputs into L2, one dword per 128-byte line
            const int64_t nt = tile + G;
            if (nt < ntiles) {
                const int64_t nbase = nt * BT;
                const int nr = (int)(T - nbase < BT ? T - nbase : BT);
                const int mline = (BT * m * 4 + 127) / 128;
                const int idx = tid;
                const float* p = nullptr;
                const int ne = nr * m;
                if (idx < mline) {
                    if (32 * idx < ne) p = a.act + nbase * m + 32 * idx;
                } else if (idx < 2 * mline) {
                    if (32 * (idx - mline) < ne) p = a.mu0 + nbase * m + 32 * (idx - mline);
                } else if (idx == 2 * mline) {
                    p = a.adv + nbase;
                } else if (idx == 2 * mline + 1) {
                    p = a.ll0 + nbase;
                }
                touch[0] = *(p ? p : reinterpret_cast<const float*>(a.xs));
            } else {
                touch[0] = *reinterpret_cast<const float*>(a.xs);
            }
        }
        __syncthreads();
        KX_STAMP(0);

        // Every chain interval below: the chain's LDS reads, the P1 group's operand reads
        // behind them (so their latency runs under the chain), the chain's arithmetic,
        // then the group's products.  (tanhf and the row pass branch, so the compiler
        // cannot interleave products into them; the two waves of a SIMD taking the two
        // in opposite orders measured slower, profiles/r07a/variants.txt.)
        half8 ph[GMAX][2], pl[GMAX][2];

        // ---- fold: a0 of row block kh; first P1 group of tile t+1 ----
        floatx4 accn[2] = {zero4(), zero4()};
        {
            const int col = cb * 16 + r16;
            float dv[4];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) dv[rr] = D0[(kh * 16 + 4 * q + rr) * L::LD + col];
            p1_load(nb, L::step0(0), L::step0(1), ph, pl);
            __builtin_amdgcn_sched_barrier(0);
            float av[4];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) av[rr] = tanhf((kh ? acc1[1][rr] : acc1[0][rr]) + dv[rr]);
            astore4(A0i, col, kh * 16 + 4 * q, av);
            p1_mma(L::step0(0), L::step0(1), ph, pl, accn);
        }
        // tile t+2's xhat loads (conditional), first half: after the publish has emptied
        // the registers, before this tile's unconditional row-pass loads (kx.h, comment
        // at xload)
        xload(tile + 2 * G, 0, L::XPER / 2);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        KX_STAMP(2);

        // ---- P2: layer 1, wave -> (rb = kh, cb); second P1 group ----
        {
            const int j = cb * 16 + r16;
            half8 bh[2], bl[2], xh[2], xl[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                arow(A0i, kh, s, q, r16, xh[s], xl[s]);
                wrow(S1, L::WIMG, j, s, q, bh[s], bl[s]);
            }
            const float rsc = sc1[j] * AHR_INV;
            p1_load(nb, L::step0(1), L::step0(2), ph, pl);
            __builtin_amdgcn_sched_barrier(0);
            floatx4 acc = zero4();
#pragma unroll
            for (int s = 0; s < 2; ++s) acc = mfma_x3(xh[s], xl[s], bh[s], bl[s], acc);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) acc[rr] *= rsc;
            float av[4];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float v = acc[rr] + bias1;
                av[rr] = tanhf(v);
            }
            astore4(A1i, j, kh * 16 + 4 * q, av);
            p1_mma(L::step0(1), L::step0(2), ph, pl, accn);
        }
        xload(tile + 2 * G, L::XPER / 2, L::XPER);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        KX_STAMP(3);

        // ---- P3: output layer [32 x MP], waves < 2 * MP/16 -> (rb3, cbo3); third P1 group ----
        // this tile's row-pass inputs (L2 hits since the previous tile's touch): loaded
        // here, after the conditional xhat loads, and consumed after the next barrier
        RowPre<BT, MP, KT> rpre;
        row_pre_load<EVAL, BT, MP, KT>(a, row_base, tid, rpre);
        {
            const bool p3 = w < 2 * (MP / 16);
            half8 bh[2], bl[2], xh[2], xl[2];
            float rsc = 0.f;
            if (p3) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    arow(A1i, rb3, s, q, r16, xh[s], xl[s]);
                    wrow(S3, L::WIMG2, col3, s, q, bh[s], bl[s]);
                }
                rsc = sc3[col3] * AHR_INV;
            }
            p1_load(nb, L::step0(2), L::step0(3), ph, pl);
            __builtin_amdgcn_sched_barrier(0);
            if (p3) {
                floatx4 acc = zero4();
#pragma unroll
                for (int s = 0; s < 2; ++s) acc = mfma_x3(xh[s], xl[s], bh[s], bl[s], acc);
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) acc[rr] *= rsc;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int row = rb3 * 16 + 4 * q + rr;
                    const float v = acc[rr] + bias3;
                    GPf[row * L::LDG + col3] = col3 < m ? v * os3 + osh3 : 0.f;
                }
            }
            p1_mma(L::step0(2), L::step0(3), ph, pl, accn);
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        KX_STAMP(4);

        // ---- row pass (LR and KL); the last P1 group and tile t+1's row scales ----
        p1_load(nb, L::step0(3), KS, ph, pl);
        __builtin_amdgcn_sched_barrier(0);
        row_pass<EVAL, BT, MP, KT, false, true>(a, P + pk.ls, sls, row_base, GPf, L::LDG, racc0, racc1, tid, &rpre,
                                                &rconst);
        p1_mma(L::step0(3), KS, ph, pl, accn);
        p1_scale(nb, accn);
        acc1[0] = accn[0];
        acc1[1] = accn[1];
        nb ^= 1;
        KX_STAMP(5);
    }

    __syncthreads();
    row_pass_final<EVAL, MP, KT>(racc0, racc1, reinterpret_cast<double*>(smem), a.rpart, blockIdx.x, tid);
#ifdef MJRL_KX_PROF
    kx_acc_[16] = __builtin_amdgcn_s_memtime() - kx_last_;
    if (blockIdx.x == 0 && tid == 0)
        for (int i = 0; i < KX_NPROF; ++i) g_kx_prof[i] += kx_acc_[i];
#endif
}

}  // namespace
