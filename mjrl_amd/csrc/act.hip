// act.hip — the device actor: the action of the Gaussian
// policy for the current observation of every environment of a device-resident
// batch, noise included, one launch per environment step.
//
// Reference: mjrl/policies/gaussian_mlp.py:91-98 (get_action: mean = MuNet.forward,
// :168-182; action = mean + exp(log_std) * randn(m); evaluation = mean) and
// gaussian_linear.py.  Where k_policy_mean (rollout.hip) serves a few hundred host
// environments with one wave per row, this kernel serves the thousands of rows of a
// batched GPU simulator: one workgroup per tile of ACT_BT rows, the three layers as
// exact-f32 MFMA products (mfma_k16), the weights read from the packed set once per
// tile, and an epilogue that owns the output tile: counter-based noise (Philox4x32-10
// keyed by (seed; step, env, column block), so a row's noise does not depend on how
// the environments or the steps are split over calls), the action, and the optional
// mean / noise / observation-copy stores, straight into the step-major slabs that
// train_from_rollout takes.
//
// Rows do not interact: every output row is a function of its own observation row,
// the parameters and (seed, step, env0 + e) alone.  Output element (row, j) is one
// accumulator lane's k-ordered fma chain over that row's activations, whichever tile
// and tile row the row falls on, so a sub-batch [a, b) launched with env0 = a gives
// the bits of rows a..b-1 of the full launch for any a (tests/test_gpu_device_actor.py).
//
// No grid barrier, no atomics, no spin loops: plain vector stores only.
#include "common.h"
#include "philox.h"

using namespace mjrl;

namespace {

constexpr int ACT_BT = 16;    // rows per workgroup: 256 tiles at E = 4096, one per CU
constexpr int ACT_KC = 128;   // observation columns staged per chunk (a multiple of 16)
constexpr int ACT_LDX = ACT_KC + 4;
constexpr int ACT_NCB = 4;    // first-layer column blocks per wave: widths up to 16 * 4 * ACT_NCB = 256

// The standard normal of column j (element j & 3 of its block of four) from the
// block's four words: Box-Muller on the pair (x0, x1) or (x2, x3), u1 = ((x >> 8) + 1)
// 2^-24 in (0, 1], u2 = (x' >> 8) 2^-24 in [0, 1) (both exact in f32), r = sqrt(-2 log
// u1), th = f32(2 pi) u2, (r cos th, r sin th): samplers/device_actor.py states the
// same in NumPy.
__device__ __forceinline__ float normal_of(const uint32_t (&x)[4], int e) {
    const uint32_t xa = e & 2 ? x[2] : x[0], xb = e & 2 ? x[3] : x[1];
    const float u1 = __fmul_rn((float)((xa >> 8) + 1u), 5.9604644775390625e-8f);
    const float u2 = __fmul_rn((float)(xb >> 8), 5.9604644775390625e-8f);
    const float r = sqrtf(__fmul_rn(-2.f, logf(u1)));
    const float th = __fmul_rn(6.283185307179586f, u2);
    return __fmul_rn(r, e & 1 ? sinf(th) : cosf(th));
}

struct ActArgs {
    const float* P;
    const float *in_shift, *in_scale, *out_shift, *out_scale;
    const float* sigma;
    uint64_t seed;
    int64_t step, env0, E;
    float* mean;
    float* eps;
};

// acc += A[16 rows][k] * W[cols 16 cb .. 16 cb + 15][k] over k in [kb, ke) (multiples of
// 16): gemm_tile's product for one 16 x 16 block with run-time k bounds, ACT_U k-groups
// of operands in flight (A: LDS row-major, lda floats, columns offset by a_col0; W:
// global row-major [.][ldw], 16-byte loads).  The k order of every output element is
// ascending, as gemm_tile's.
constexpr int ACT_U = 4;
__device__ __forceinline__ floatx4 act_gemm(floatx4 acc, const float* As, int lda, int a_col0,
                                            const float* __restrict__ W, int ldw, int cb, int kb, int ke, int lane) {
    const int r = lane & 15, q = lane >> 4;
    const float* __restrict__ wp = W + (size_t)(cb * 16 + r) * ldw + 4 * q;
    const float* ap = As + r * lda - a_col0 + 4 * q;
    int k = kb;
    for (; k + 16 * ACT_U <= ke; k += 16 * ACT_U) {
        float4 a[ACT_U], b[ACT_U];
#pragma unroll
        for (int u = 0; u < ACT_U; ++u) b[u] = *reinterpret_cast<const float4*>(wp + k + 16 * u);
#pragma unroll
        for (int u = 0; u < ACT_U; ++u) a[u] = *reinterpret_cast<const float4*>(ap + k + 16 * u);
#pragma unroll
        for (int u = 0; u < ACT_U; ++u) acc = mfma_k16(a[u], b[u], acc);
    }
    const int rem = (ke - k) >> 4;   // 0 .. ACT_U - 1 k-groups left (wave-uniform)
    if (rem) {
        float4 a[ACT_U - 1], b[ACT_U - 1];
#pragma unroll
        for (int u = 0; u < ACT_U - 1; ++u)
            if (u < rem) b[u] = *reinterpret_cast<const float4*>(wp + k + 16 * u);
#pragma unroll
        for (int u = 0; u < ACT_U - 1; ++u)
            if (u < rem) a[u] = *reinterpret_cast<const float4*>(ap + k + 16 * u);
#pragma unroll
        for (int u = 0; u < ACT_U - 1; ++u)
            if (u < rem) acc = mfma_k16(a[u], b[u], acc);
    }
    return acc;
}

// tanh(As [16][K] W^T + bias) -> out [16][16 CB] (LDS), W [16 CB][ldw] global; wave w
// takes column blocks w, w + 4, ...
__device__ __forceinline__ void hidden_layer(const float* As, int lda, int K, const float* __restrict__ W, int ldw,
                                             const float* __restrict__ bias, int CB, float* out, int ldo, int w,
                                             int lane) {
    const int col = lane & 15, q = lane >> 4;
    for (int cb = w; cb < CB; cb += 4) {
        const floatx4 acc = act_gemm(zero4(), As, lda, 0, W, ldw, cb, 0, K, lane);
        const float b = bias[cb * 16 + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(4 * q + r) * ldo + cb * 16 + col] = tanhf(acc[r] + b);
    }
}

// The epilogue of one 16 x 16 block of the output layer: lane (q, col) holds rows
// 4q .. 4q + 3 of column j = 16 cb + col.
template <typename ObsT>
__device__ __forceinline__ void act_epilogue(const ActArgs& a, int m, int64_t row0, int cb, const floatx4& acc,
                                             float bias, ObsT* __restrict__ act, int lane) {
    const int j = cb * 16 + (lane & 15), q = lane >> 4;
    if (j >= m) return;
    const float osc = a.out_scale ? a.out_scale[j] : 1.f, osh = a.out_scale ? a.out_shift[j] : 0.f;
    const float sg = a.sigma ? a.sigma[j] : 0.f;
    const bool noise = a.sigma || a.eps;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + 4 * q + r;
        if (row >= a.E) continue;
        float mu = acc[r] + bias;
        if (a.out_scale) mu = mu * osc + osh;
        float e = 0.f;
        if (noise) {
            const uint64_t env = (uint64_t)(a.env0 + row);
            uint32_t c[4] = {(uint32_t)a.step, (uint32_t)((uint64_t)a.step >> 32), (uint32_t)env, (uint32_t)(j >> 2)};
            philox4x32_10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
            e = normal_of(c, j & 3);
        }
        const float v = a.sigma ? __fadd_rn(mu, __fmul_rn(sg, e)) : mu;
        act[row * m + j] = (ObsT)v;
        if (a.mean) a.mean[row * m + j] = mu;
        if (a.eps) a.eps[row * m + j] = e;
    }
}

// One workgroup (4 waves) per tile of ACT_BT rows.  LDS: xs [16][ACT_LDX] (the
// normalised observation chunk, bias column n = 1, zeros after), a0 [16][h0 + 4],
// a1 [16][h1 + 4].  Rows at or beyond E are computed on zeros and store nothing.
template <typename ObsT>
__global__ void __launch_bounds__(NTHREADS) k_policy_act(mjrl_shape s, const ObsT* __restrict__ obs, ActArgs a,
                                                         ObsT* __restrict__ act, ObsT* __restrict__ obs_copy) {
    extern __shared__ __attribute__((aligned(16))) float act_sm[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = s.n, m = s.m, np = s.np, mp = s.mp, h0 = s.h0, h1 = s.h1;
    const Packed pk(h0, h1, np, mp);
    const int ld0 = h0 + 4, ld1 = h1 + 4;
    float* xs = act_sm;
    float* a0 = xs + ACT_BT * ACT_LDX;
    float* a1 = a0 + ACT_BT * ld0;
    const int64_t row0 = (int64_t)blockIdx.x * ACT_BT;
    const int nlive = (int)(a.E - row0 < ACT_BT ? a.E - row0 : ACT_BT);
    const int CB0 = (h0 ? h0 : mp) >> 4;   // column blocks of the first product (the only one of the linear policy)

    // first product over the observation columns, chunk by chunk: x [16][np] W0^T,
    // W0 [h0][np] (linear: Wp [mp][np]) with the bias in column n
    floatx4 acc0[ACT_NCB];
#pragma unroll
    for (int i = 0; i < ACT_NCB; ++i) acc0[i] = zero4();
    for (int c0 = 0; c0 < np; c0 += ACT_KC) {
        const int kc = np - c0 < ACT_KC ? np - c0 : ACT_KC;
        if (c0) __syncthreads();   // the previous chunk has been read
        for (int i = threadIdx.x; i < ACT_BT * kc; i += NTHREADS) {
            const int r = i / kc, c = c0 + i % kc;
            float x = 0.f;
            if (r < nlive && c < n) {
                const ObsT raw = obs[(row0 + r) * n + c];
                if (obs_copy) obs_copy[(row0 + r) * n + c] = raw;
                x = (float)raw;
                if (a.in_shift) x = (x - a.in_shift[c]) / (a.in_scale[c] + 1e-8f);
            } else if (c == n) {
                x = 1.f;
            }
            xs[r * ACT_LDX + (c - c0)] = x;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ACT_NCB; ++i) {
            const int cb = w + 4 * i;
            if (cb < CB0) acc0[i] = act_gemm(acc0[i], xs, ACT_LDX, c0, a.P + pk.W0, np, cb, c0, c0 + kc, lane);
        }
    }

    if (h0 == 0) {   // linear policy
#pragma unroll
        for (int i = 0; i < ACT_NCB; ++i) {
            const int cb = w + 4 * i;
            if (cb < CB0) act_epilogue<ObsT>(a, m, row0, cb, acc0[i], 0.f, act, lane);
        }
        return;
    }
    {   // a0 = tanh(fc0)
        const int col = lane & 15, q = lane >> 4;
#pragma unroll
        for (int i = 0; i < ACT_NCB; ++i) {
            const int cb = w + 4 * i;
            if (cb < CB0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) a0[(4 * q + r) * ld0 + cb * 16 + col] = tanhf(acc0[i][r]);
            }
        }
    }
    __syncthreads();
    hidden_layer(a0, ld0, h0, a.P + pk.W1, h0, a.P + pk.b1, h1 >> 4, a1, ld1, w, lane);   // a1 = tanh(fc1)
    __syncthreads();
    for (int cb = w; cb < (mp >> 4); cb += 4) {   // fc2, de-normalised, and the action
        const floatx4 acc = act_gemm(zero4(), a1, ld1, 0, a.P + pk.W2, h1, cb, 0, h1, lane);
        act_epilogue<ObsT>(a, m, row0, cb, acc, a.P[pk.b2 + cb * 16 + (lane & 15)], act, lane);
    }
}

}  // namespace

extern "C" {

int mjrl_policy_act(const mjrl_shape* s, const void* obs, int32_t obs_f64, int64_t E, const float* packed_theta,
                    const float* in_shift, const float* in_scale, const float* out_shift, const float* out_scale,
                    const float* sigma, uint64_t seed, int64_t step, int64_t env0, void* act, float* mean, float* eps,
                    void* obs_copy, void* stream) {
    if (!s || !packed_theta || E < 0 || step < 0 || (obs_f64 != 0 && obs_f64 != 1) || (E > 0 && (!obs || !act)))
        return MJRL_EINVAL;
    if ((in_shift == nullptr) != (in_scale == nullptr) || (out_shift == nullptr) != (out_scale == nullptr))
        return MJRL_EINVAL;
    if (s->h0 > 64 * ACT_NCB || s->mp > 64 * ACT_NCB || s->np % 16 || s->mp % 16 || s->h0 % 16 || s->h1 % 16 ||
        (s->h0 == 0) != (s->h1 == 0))
        return MJRL_ESHAPE;
    if (E == 0) return MJRL_OK;
    const int64_t g = (E + ACT_BT - 1) / ACT_BT;
    if (g > 0x7fffffff) return MJRL_EINVAL;
    const size_t lds = (size_t)ACT_BT * (ACT_LDX + (s->h0 + 4) + (s->h1 + 4)) * sizeof(float);
    ActArgs a{packed_theta, in_shift, in_scale, out_shift, out_scale, sigma, seed, step, env0, E, mean, eps};
    if (obs_f64)
        hipLaunchKernelGGL(k_policy_act<double>, dim3((unsigned)g), dim3(NTHREADS), lds, (hipStream_t)stream, *s,
                           (const double*)obs, a, (double*)act, (double*)obs_copy);
    else
        hipLaunchKernelGGL(k_policy_act<float>, dim3((unsigned)g), dim3(NTHREADS), lds, (hipStream_t)stream, *s,
                           (const float*)obs, a, (float*)act, (float*)obs_copy);
    return (int)hipGetLastError();
}

}  // extern "C"
