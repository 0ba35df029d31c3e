// fit.h — what the fused minibatch Adam fits (value_fit.hip, policy_fit.hip) share: the Adam
// step and its host-side constants, the zero-padded operand loaders, the tail of a
// weight-gradient job and the check of a net's pointers.
#pragma once

#include <math.h>

#include "common.h"

namespace mjrl {

// Adam (torch's single-tensor formula): g' = g + wd p, m += (g' - m)(1 - beta1),
// v = beta2 v + (1 - beta2) g'^2 evaluated in f64 and rounded once on the store
// (an f32 evaluation cancels in m for g' near -9 m), then
// p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps) in f32 on the stored moments,
// the bias corrections bc1 = 1 - beta1^t, bc2 = 1 - beta2^t formed on the host
// in f64 for every step.
struct AdamK {
    double omb1, beta2, omb2, wd;     // 1 - beta1, beta2, 1 - beta2, weight decay
    float step_size, bc2s, eps;       // lr / bc1, sqrt(bc2), eps
};

// the step-independent part of AdamK (step_size = bc2s = 1 until adam_bias sets them)
inline AdamK adam_consts(const mjrl_adam* hp) {
    return AdamK{1.0 - hp->beta1, hp->beta2, 1.0 - hp->beta2, hp->weight_decay, 1.f, 1.f, (float)hp->eps};
}

// step_size and bc2s of step k of a call (k = 0 the first): a function of the absolute
// step number alone, whatever the split into launches and calls
inline void adam_bias(const mjrl_adam* hp, int64_t k, float& step_size, float& bc2s) {
    const double t = (double)(hp->step0 + k + 1);
    step_size = (float)(hp->lr / (1.0 - pow(hp->beta1, t)));
    bc2s = (float)sqrt(1.0 - pow(hp->beta2, t));
}

// one element's Adam step from its loaded parameter and moments; g is the minibatch
// gradient before weight decay
__device__ __forceinline__ void adam_step(float p0, float m0, float v0, float g, const AdamK& h, float& p1, float& m1,
                                          float& v1) {
    const double gd = (double)g + h.wd * (double)p0;
    m1 = (float)((double)m0 + (gd - (double)m0) * h.omb1);
    v1 = (float)(h.beta2 * (double)v0 + h.omb2 * (gd * gd));
    const float denom = sqrtf(v1) / h.bc2s + h.eps;
    p1 = p0 - h.step_size * (m1 / denom);
}

// The loaders: branch-free (clamped addresses, then selects) so that a run of them issues
// as one burst; vec (16-byte loads) needs K % 4 == 0, k % 4 == 0 and an aligned row: all
// four elements inside or all four outside.  ldw4 is ld4 with a row guard; it keeps a body
// of its own because k_pfit allocates other registers (and spills more of them) when the
// guard is a select behind ld4 or a flag passed into it.
//
// row[k .. k + 3], zero past K
__device__ __forceinline__ float4 ld4(const float* row, int k, int K, bool vec) {
    float4 r;
    if (vec) {
        r = *reinterpret_cast<const float4*>(row + (k < K ? k : K - 4));
        if (k >= K) r = float4{0.f, 0.f, 0.f, 0.f};
        return r;
    }
    const int l = K - 1;
    r.x = row[k < l ? k : l];
    r.y = row[k + 1 < l ? k + 1 : l];
    r.z = row[k + 2 < l ? k + 2 : l];
    r.w = row[k + 3 < l ? k + 3 : l];
    r.x = k < K ? r.x : 0.f;
    r.y = k + 1 < K ? r.y : 0.f;
    r.z = k + 2 < K ? r.z : 0.f;
    r.w = k + 3 < K ? r.w : 0.f;
    return r;
}

// W[row][k .. k + 3] of a [rows][K] matrix, zero for row >= rows and past K
__device__ __forceinline__ float4 ldw4(const float* W, int rows, int K, int row, int k, bool vec) {
    const float* const p = W + (size_t)(row < rows ? row : rows - 1) * K;
    float4 r;
    if (vec) {
        r = *reinterpret_cast<const float4*>(p + (k < K ? k : K - 4));
        if (k >= K || row >= rows) r = float4{0.f, 0.f, 0.f, 0.f};
        return r;
    }
    const int l = K - 1;
    r.x = p[k < l ? k : l];
    r.y = p[k + 1 < l ? k + 1 : l];
    r.z = p[k + 2 < l ? k + 2 : l];
    r.w = p[k + 3 < l ? k + 3 : l];
    const bool in = row < rows;
    r.x = in && k < K ? r.x : 0.f;
    r.y = in && k + 1 < K ? r.y : 0.f;
    r.z = in && k + 2 < K ? r.z : 0.f;
    r.w = in && k + 3 < K ? r.w : 0.f;
    return r;
}

// W[j .. j + 3][col] of a [rows][K] matrix (the transposed operand), zero outside
__device__ __forceinline__ float4 ldwt4(const float* W, int rows, int K, int j, int col) {
    const int c = col < K ? col : K - 1, l = rows - 1;
    float4 r;
    r.x = W[(size_t)(j < l ? j : l) * K + c];
    r.y = W[(size_t)(j + 1 < l ? j + 1 : l) * K + c];
    r.z = W[(size_t)(j + 2 < l ? j + 2 : l) * K + c];
    r.w = W[(size_t)(j + 3 < l ? j + 3 : l) * K + c];
    const bool in = col < K;
    r.x = in && j < rows ? r.x : 0.f;
    r.y = in && j + 1 < rows ? r.y : 0.f;
    r.z = in && j + 2 < rows ? r.z : 0.f;
    r.w = in && j + 3 < rows ? r.w : 0.f;
    return r;
}

// The tail of a weight-gradient job for one accumulator register: its gradient g belongs
// to the weight [unit][col] of a layer with K inputs (col < K) or to that unit's bias
// (col == K, the column of ones); the caller has excluded col > K and a unit the layer has
// not.  Adam on the preloaded (p, m, v) triple pm, the gradient into its place of the flat
// gradient (grad may be null), the parameter and its moments back.  The tensors are
// wave-uniform and the element offsets 32-bit, so every access is a scalar base plus a
// lane offset.  Unit is the caller's own index type, int or unsigned: how the bias index
// is extended to 64 bits decides the register allocation of both kernels, which are at
// their limits, so each keeps the extension it was tuned with.
template <class Unit>
__device__ __forceinline__ void wgrad_tail(const float (&pm)[3], float g, Unit unit, int K, int col, const AdamK& hp,
                                           float* pw, float* mw, float* vw, float* pb, float* mb, float* vb,
                                           float* grad, int64_t gw, int64_t gb) {
    const unsigned e = (unsigned)unit * K + col;
    float p1, m1, v1;
    adam_step(pm[0], pm[1], pm[2], g, hp, p1, m1, v1);
    if (col < K) {
        if (grad) (grad + gw)[e] = g;
        pw[e] = p1;
        mw[e] = m1;
        vw[e] = v1;
    } else {
        if (grad) (grad + gb)[unit] = g;
        pb[unit] = p1;
        mb[unit] = m1;
        vb[unit] = v1;
    }
}

// a net's N tensors and their moments into p / m / v; false when one is null
template <int N, class Net>
inline bool net_ptrs(const Net* net, float* (&p)[N], float* (&m)[N], float* (&v)[N]) {
    for (int i = 0; i < N; ++i) {
        if (!net->p[i] || !net->exp_avg[i] || !net->exp_avg_sq[i]) return false;
        p[i] = net->p[i];
        m[i] = net->exp_avg[i];
        v[i] = net->exp_avg_sq[i];
    }
    return true;
}

}  // namespace mjrl
