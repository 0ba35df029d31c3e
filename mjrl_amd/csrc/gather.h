// gather.h — the fixed-order folds that end a pass (included by policy.hip after
// wgrad.h):
//   k_gather       per-job slabs (k_wgrad) -> the flat d-vector
//   k_gather_flat  flat chunk-major slabs (k_kx / k_ks / k_fused / k_wgrad_all)
//   k_eval_final   the EVAL pass's per-workgroup partials -> surrogate and KL sums
#pragma once

namespace {

// ---------------------------------------------------------------------------
// Gather: gsum[f] = sum over slices (fixed order) of the slab element feeding
// flat parameter f (reference order, gaussian_mlp.py:61-64).
// ---------------------------------------------------------------------------
struct GArgs {
    int n, m, h0, h1, np, mp, d, S;
    int64_t off0, off1, off2, boff1, boff2;
    const float* wpart;
    int64_t wcap;           // floats of the scratch's slabs (MJRL_SLAB_CHECK)
    const double* lspart;   // FWD: per-row-kernel-WG log-std partials [G][mp]; null for FVP
    int G;
    float* gsum;
    const int32_t* done;
    CgZ cz;   // fused CG z step (cz.p == nullptr: plain gather)
};

// Block = 16 waves over 64 consecutive flat parameters: lane -> parameter, wave w
// loads its contiguous share of the slices (all loads in flight at once) and sums
// them in slice order; wave 0 adds the sixteen wave partials in order
// (deterministic, fp64).
constexpr int GATHER_WAVES = 16;
constexpr int GATHER_PER = 16;   // slices per wave per batch (S <= 256: one batch)

__global__ void __launch_bounds__(64 * GATHER_WAVES) k_gather(GArgs a) {
    if (a.done && *a.done) return;
    __shared__ double part[GATHER_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + lane;
    int64_t src = -1, stride = 0;
    int lsj = -1;
    int g = f;
    if (f >= a.d) {
    } else if (a.h0 == 0) {
        if (g < a.m * a.n) {
            src = a.off0 + (int64_t)(g / a.n) * a.np + g % a.n;
            stride = (int64_t)a.mp * a.np;
        } else if ((g -= a.m * a.n) < a.m) {
            src = a.off0 + (int64_t)g * a.np + a.n;
            stride = (int64_t)a.mp * a.np;
        } else {
            lsj = g - a.m;
        }
    } else {
        const int s0 = a.h0 * a.n, s1 = a.h0, s2 = a.h1 * a.h0, s3 = a.h1, s4 = a.m * a.h1, s5 = a.m;
        if (g < s0) {
            src = a.off0 + (int64_t)(g / a.n) * a.np + g % a.n;
            stride = (int64_t)a.h0 * a.np;
        } else if ((g -= s0) < s1) {
            src = a.off0 + (int64_t)g * a.np + a.n;
            stride = (int64_t)a.h0 * a.np;
        } else if ((g -= s1) < s2) {
            src = a.off1 + g;
            stride = (int64_t)a.h1 * a.h0;
        } else if ((g -= s2) < s3) {
            src = a.boff1 + g;
            stride = a.h1;
        } else if ((g -= s3) < s4) {
            src = a.off2 + g;   // [mp][h1] with rows < m contiguous as [m][h1]
            stride = (int64_t)a.mp * a.h1;
        } else if ((g -= s4) < s5) {
            src = a.boff2 + g;
            stride = a.mp;
        } else {
            lsj = g - s5;
        }
    }
    double acc = 0.0;
    if (src >= 0) {
        const int per = (a.S + GATHER_WAVES - 1) / GATHER_WAVES;
        const int s0 = w * per, s1 = min(a.S, s0 + per);
        const float* p = a.wpart + src;
        if (s1 > s0) MJRL_SLAB_CHECK(src + (int64_t)(s1 - 1) * stride, a.wcap);
        for (int sb = s0; sb < s1; sb += GATHER_PER) {
            float v[GATHER_PER];
#pragma unroll
            for (int j = 0; j < GATHER_PER; ++j) v[j] = sb + j < s1 ? p[(int64_t)(sb + j) * stride] : 0.f;
#pragma unroll
            for (int j = 0; j < GATHER_PER; ++j) acc += (double)v[j];
        }
    } else if (lsj >= 0 && a.lspart) {
        const int per = (a.G + GATHER_WAVES - 1) / GATHER_WAVES;
        const int b0 = w * per, b1 = min(a.G, b0 + per);
        for (int b = b0; b < b1; ++b) acc += a.lspart[(int64_t)b * a.mp + lsj];
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0) {
        float gs = 0.f;
        if (f < a.d) {
            double t = part[0][lane];
#pragma unroll
            for (int j = 1; j < GATHER_WAVES; ++j) t += part[j][lane];
            gs = (float)t;
            a.gsum[f] = gs;
        }
        if (a.cz.p) cgz_epilogue(a.cz, f, a.d, gs);
    }
}

// Gather of the flat slab layout of k_kx: block c folds wpart[c][0..S)[64] — one
// contiguous run — for flat parameters 64c..64c+63 (waves take 16 slices each,
// loads all in flight, fixed-order fp64 sums); log-std entries (FWD) from lspart.
__global__ void __launch_bounds__(64 * GATHER_WAVES) k_gather_flat(const float* __restrict__ wpart, int S, int d_mu,
                                                                   int d, const double* __restrict__ lspart, int G,
                                                                   int mp, float* __restrict__ gsum,
                                                                   const int32_t* __restrict__ done, CgZ cz,
                                                                   int64_t wcap) {
    __shared__ double part[GATHER_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + lane;
    float pf = 0.f, lsv = 0.f;   // the CG z step's operands, in flight with the slab loads
    if (w == 0 && cz.p) cgz_load(cz, f, d, pf, lsv);
    double acc = 0.0;
    if (f < d_mu) {
        const int per = (S + GATHER_WAVES - 1) / GATHER_WAVES;
        const int s0 = w * per, s1 = min(S, s0 + per);
        const float* p = wpart + (int64_t)blockIdx.x * S * 64 + lane;
        if (s1 > s0) MJRL_SLAB_CHECK((int64_t)blockIdx.x * S * 64 + lane + (int64_t)(s1 - 1) * 64, wcap);
        for (int sb = s0; sb < s1; sb += GATHER_PER) {
            float v[GATHER_PER];
#pragma unroll
            for (int j = 0; j < GATHER_PER; ++j) v[j] = sb + j < s1 ? p[(int64_t)(sb + j) * 64] : 0.f;
#pragma unroll
            for (int j = 0; j < GATHER_PER; ++j) acc += (double)v[j];
        }
    } else if (f < d && lspart) {
        const int lsj = f - d_mu;
        const int per = (G + GATHER_WAVES - 1) / GATHER_WAVES;
        const int b0 = w * per, b1 = min(G, b0 + per);
        for (int b = b0; b < b1; ++b) acc += lspart[(int64_t)b * mp + lsj];
    }
    part[w][lane] = acc;
    // a converged CG loop: nothing is stored (checked after the slab loads, whose
    // results the store above consumed, so the flag's load overlaps them)
    if (done && *done) return;
    __syncthreads();
    if (w == 0) {
        float gs = 0.f;
        if (f < d) {
            double t = part[0][lane];
#pragma unroll
            for (int j = 1; j < GATHER_WAVES; ++j) t += part[j][lane];
            gs = (float)t;
            gsum[f] = gs;
        }
        if (cz.p) cgz_epilogue(cz, f, d, gs, pf, lsv);
    }
}

__global__ void __launch_bounds__(64) k_eval_final(const double* __restrict__ rpart, int G, double* __restrict__ sums,
                                                   const int32_t* __restrict__ skip) {
    if (skip && *skip) return;
    // one wave: lane l folds partials l, l+64, ... in order, then a fixed shuffle tree
    double s = 0.0, k = 0.0;
    for (int b = threadIdx.x; b < G; b += 64) {
        s += rpart[2 * b];
        k += rpart[2 * b + 1];
    }
    s = wave_sum(s);
    k = wave_sum(k);
    if (threadIdx.x == 0) {
        sums[0] = s;
        sums[1] = k;
    }
}

}  // namespace
