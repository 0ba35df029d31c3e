// rollout.hip — the batched policy forward of vectorised sampling (SURVEY.md §8f
// row f3): the mean action of the Gaussian policy for the current observation of
// every environment of a lock-stepped batch, one launch per environment step.
//
// Reference: mjrl/policies/gaussian_mlp.py:92-98 (get_action: the mean of
// MuNet.forward, :168-182, plus host noise) and gaussian_linear.py; the loop it
// serves is mjrl/samplers/base_sampler.py:64-74.  Latency-bound (a few hundred
// rows): one 64-lane wave per row, 4 rows per workgroup, the row's activations in
// LDS, weights from the packed parameter set (L2-resident across steps).  fp32
// dot products per output unit in index order.  Below it, what else reads the
// lock step's observations on the device: the MLPBaseline value features
// (mlp_baseline.py:37-56), formed row by row while sampling and assembled into
// the value network's input after it.
#include "common.h"

using namespace mjrl;

namespace {

constexpr int ACT_ROWS = 4;   // rows (waves) per workgroup

// The forward of one row by one wave (all 64 * ACT_ROWS threads of the workgroup
// call it: it holds the barriers).  ObsT: float, or double rounded to float here
// ((float)x: round to nearest even, numpy's astype(float32)) before anything else,
// so both entry points run the same f32 arithmetic.  `row` indexes obs [.][n] and
// mean [.][m]; a wave with live == false computes on zeros and writes nothing.
template <typename ObsT>
__device__ __forceinline__ void policy_mean_row(const mjrl_shape& s, const ObsT* __restrict__ obs, int64_t row,
                                                bool live, const float* __restrict__ P,
                                                const float* __restrict__ in_shift,
                                                const float* __restrict__ in_scale,
                                                const float* __restrict__ out_shift,
                                                const float* __restrict__ out_scale, float* __restrict__ mean,
                                                float* sm) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = s.n, m = s.m, np = s.np, h0 = s.h0, h1 = s.h1;
    const Packed pk(h0, h1, np, s.mp);
    float* xs = sm + w * (np + h0 + h1);
    float* a0 = xs + np;
    float* a1 = a0 + h0;
    // xhat = (obs - in_shift) / (in_scale + 1e-8), bias column n = 1 (MuNet.forward:177)
    for (int c = lane; c < np; c += 64) {
        float x = 0.f;
        if (live && c < n) {
            x = (float)obs[row * n + c];
            if (in_shift) x = (x - in_shift[c]) / (in_scale[c] + 1e-8f);
        } else if (c == n) {
            x = 1.f;
        }
        xs[c] = x;
    }
    __syncthreads();
    if (h0 == 0) {   // linear policy: Wp [MP][NP] with the bias in column n
        for (int j = lane; j < m; j += 64) {
            float acc = 0.f;
            for (int k = 0; k < np; ++k) acc += P[pk.W0 + j * np + k] * xs[k];
            if (live) mean[row * m + j] = out_scale ? acc * out_scale[j] + out_shift[j] : acc;
        }
        return;
    }
    for (int j = lane; j < h0; j += 64) {   // tanh(fc0): W0 [h0][np], b0 in column n
        float acc = 0.f;
        for (int k = 0; k < np; ++k) acc += P[pk.W0 + j * np + k] * xs[k];
        a0[j] = tanhf(acc);
    }
    __syncthreads();
    for (int j = lane; j < h1; j += 64) {   // tanh(fc1): W1T [h0][h1] (coalesced over j)
        float acc = 0.f;
        for (int k = 0; k < h0; ++k) acc += P[pk.W1T + k * h1 + j] * a0[k];
        a1[j] = tanhf(acc + P[pk.b1 + j]);
    }
    __syncthreads();
    for (int j = lane; j < m; j += 64) {    // fc2, de-normalised: W2T [h1][mp]
        float acc = 0.f;
        for (int k = 0; k < h1; ++k) acc += P[pk.W2T + k * s.mp + j] * a1[k];
        acc += P[pk.b2 + j];
        if (live) mean[row * m + j] = out_scale ? acc * out_scale[j] + out_shift[j] : acc;
    }
}

__global__ void __launch_bounds__(64 * ACT_ROWS) k_policy_mean(mjrl_shape s, const float* __restrict__ obs, int64_t N,
                                                              const float* __restrict__ P,
                                                              const float* __restrict__ in_shift,
                                                              const float* __restrict__ in_scale,
                                                              const float* __restrict__ out_shift,
                                                              const float* __restrict__ out_scale,
                                                              float* __restrict__ mean) {
    extern __shared__ float sm[];
    const int64_t row = (int64_t)blockIdx.x * ACT_ROWS + (threadIdx.x >> 6);
    policy_mean_row<float>(s, obs, row, row < N, P, in_shift, in_scale, out_shift, out_scale, mean, sm);
}

// The same forward for the E slots live[0..E) of an observation board obs64 [S][n]
// (f64, one row per environment slot): wave i reads row live[i] and writes row
// live[i] of mean [S][m].  An index outside [0, S) is skipped, never dereferenced.
__global__ void __launch_bounds__(64 * ACT_ROWS) k_policy_mean_slots(mjrl_shape s, const double* __restrict__ obs64,
                                                                    const int32_t* __restrict__ live, int64_t E,
                                                                    int64_t S, const float* __restrict__ P,
                                                                    const float* __restrict__ in_shift,
                                                                    const float* __restrict__ in_scale,
                                                                    const float* __restrict__ out_shift,
                                                                    const float* __restrict__ out_scale,
                                                                    float* __restrict__ mean) {
    extern __shared__ float sm[];
    const int64_t i = (int64_t)blockIdx.x * ACT_ROWS + (threadIdx.x >> 6);
    const int64_t slot = i < E ? (int64_t)live[i] : -1;
    const bool ok = slot >= 0 && slot < S;
    policy_mean_row<double>(s, obs64, ok ? slot : 0, ok, P, in_shift, in_scale, out_shift, out_scale, mean, sm);
}

// ---- MLPBaseline value features formed while sampling (mlp_baseline.py:37-56) ----
// float32(clip(x, +-10) / 10) of the f64 observation, the first n feature columns.
// The clip is written as comparisons (a NaN fails both and stays, -0.0 stays -0.0,
// as np.clip leaves them), the division is an f64 division (x * 0.1 rounds
// differently) and (float) rounds to nearest even: numpy's .astype('float32').
__device__ __forceinline__ float value_feature(double x) {
    const double c = x < -10.0 ? -10.0 : (x > 10.0 ? 10.0 : x);
    return (float)(c / 10.0);
}

// Row live[i] of the observation board obs64 [S][n] to row dest[i] of feat
// [rows_cap][n], one wave per row (elementwise, a few hundred rows: latency-bound).
// A live index outside [0, S) or a dest index outside [0, rows_cap) skips the row.
__global__ void __launch_bounds__(64 * ACT_ROWS) k_value_features_slots(const double* __restrict__ obs64,
                                                                       const int32_t* __restrict__ live,
                                                                       const int64_t* __restrict__ dest, int64_t E,
                                                                       int64_t S, int n, int64_t rows_cap,
                                                                       float* __restrict__ feat) {
    const int64_t i = (int64_t)blockIdx.x * ACT_ROWS + (threadIdx.x >> 6);
    if (i >= E) return;
    const int64_t slot = (int64_t)live[i], row = dest[i];
    if (slot < 0 || slot >= S || row < 0 || row >= rows_cap) return;
    const double* __restrict__ x = obs64 + slot * n;
    float* __restrict__ f = feat + row * n;
    for (int c = threadIdx.x & 63; c < n; c += 64) f[c] = value_feature(x[c]);
}

// out [T][n + 4]: row i = [feat_pad[r][0..n), time_tab[r % H][0..4)], r = src_row[i]
// (i itself when src_row is null).  One wave per row per grid stride, V = float4 /
// float2 / float words: n is a multiple of V's width, so are both row pitches (n and
// n + 4 floats) and no word straddles the two sources; the host picks the widest V
// that n and the base addresses allow.  A row index outside [0, rows_cap) skips the
// row.  HBM-bound: T (2 n + 4) floats moved.
template <typename V>
__global__ void __launch_bounds__(256) k_value_features_finish(const V* __restrict__ feat_pad,
                                                               const int64_t* __restrict__ src_row, int64_t T,
                                                               int nv, int64_t rows_cap, int64_t H,
                                                               const V* __restrict__ time_tab, V* __restrict__ out) {
    constexpr int TV = 16 / (int)sizeof(V);   // words of V per time_tab row (4 floats)
    const int lane = threadIdx.x & 63;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < T; i += nw) {
        const int64_t r = src_row ? src_row[i] : i;
        if (r < 0 || r >= rows_cap) continue;
        const V* __restrict__ s = feat_pad + r * nv;
        const V* __restrict__ tt = time_tab + (r % H) * TV;
        V* __restrict__ d = out + i * (nv + TV);
        for (int c = lane; c < nv + TV; c += 64) d[c] = c < nv ? s[c] : tt[c - nv];
    }
}

}  // namespace

extern "C" {

int mjrl_policy_mean(const mjrl_shape* s, const float* obs, int64_t N, const float* packed_theta,
                     const float* in_shift, const float* in_scale, const float* out_shift, const float* out_scale,
                     float* mean, void* stream) {
    if (!s || !packed_theta || !mean || N < 0 || (N > 0 && !obs)) return MJRL_EINVAL;
    if ((in_shift == nullptr) != (in_scale == nullptr) || (out_shift == nullptr) != (out_scale == nullptr))
        return MJRL_EINVAL;
    if (N == 0) return MJRL_OK;
    const size_t lds = (size_t)ACT_ROWS * (s->np + s->h0 + s->h1) * sizeof(float);
    const int64_t g = (N + ACT_ROWS - 1) / ACT_ROWS;
    hipLaunchKernelGGL(k_policy_mean, dim3((unsigned)g), dim3(64 * ACT_ROWS), lds, (hipStream_t)stream, *s, obs, N,
                       packed_theta, in_shift, in_scale, out_shift, out_scale, mean);
    return (int)hipGetLastError();
}

int mjrl_policy_mean_slots(const mjrl_shape* s, const double* obs64, const int32_t* live, int64_t E, int64_t S,
                           const float* packed_theta, const float* in_shift, const float* in_scale,
                           const float* out_shift, const float* out_scale, float* mean, void* stream) {
    if (!s || !packed_theta || !mean || E < 0 || S < 0 || E > S || (E > 0 && (!obs64 || !live))) return MJRL_EINVAL;
    if ((in_shift == nullptr) != (in_scale == nullptr) || (out_shift == nullptr) != (out_scale == nullptr))
        return MJRL_EINVAL;
    if (E == 0) return MJRL_OK;
    const size_t lds = (size_t)ACT_ROWS * (s->np + s->h0 + s->h1) * sizeof(float);
    const int64_t g = (E + ACT_ROWS - 1) / ACT_ROWS;
    hipLaunchKernelGGL(k_policy_mean_slots, dim3((unsigned)g), dim3(64 * ACT_ROWS), lds, (hipStream_t)stream, *s, obs64,
                       live, E, S, packed_theta, in_shift, in_scale, out_shift, out_scale, mean);
    return (int)hipGetLastError();
}

int mjrl_value_features_slots(const double* obs64, const int32_t* live, const int64_t* dest, int64_t E, int64_t S,
                              int32_t n, int64_t rows_cap, float* feat, void* stream) {
    if (E < 0 || S < 0 || E > S || n <= 0 || rows_cap < 0 || (E > 0 && (!obs64 || !live || !dest || !feat)))
        return MJRL_EINVAL;
    if (E == 0) return MJRL_OK;
    const int64_t g = (E + ACT_ROWS - 1) / ACT_ROWS;
    hipLaunchKernelGGL(k_value_features_slots, dim3((unsigned)g), dim3(64 * ACT_ROWS), 0, (hipStream_t)stream, obs64,
                       live, dest, E, S, (int)n, rows_cap, feat);
    return (int)hipGetLastError();
}

int mjrl_value_features_finish(const float* feat_pad, const int64_t* src_row, int64_t T, int32_t n, int64_t rows_cap,
                               int64_t H, const float* time_tab, float* out, void* stream) {
    if (T < 0 || n <= 0 || rows_cap < 0 || H <= 0 || (T > 0 && (!feat_pad || !time_tab || !out))) return MJRL_EINVAL;
    if (!src_row && T > rows_cap) return MJRL_EINVAL;   // identity rows: i < T must be rows of feat_pad
    if (T == 0) return MJRL_OK;
    const int64_t waves = (T + 3) / 4;   // 4 waves per workgroup, grid-stride past 2^16 workgroups
    const unsigned g = (unsigned)(waves < 65536 ? waves : 65536);
    const uintptr_t a = (uintptr_t)feat_pad | (uintptr_t)time_tab | (uintptr_t)out;
    hipStream_t st = (hipStream_t)stream;
    if (n % 4 == 0 && a % 16 == 0)
        hipLaunchKernelGGL(k_value_features_finish<float4>, dim3(g), dim3(256), 0, st, (const float4*)feat_pad, src_row,
                           T, n / 4, rows_cap, H, (const float4*)time_tab, (float4*)out);
    else if (n % 2 == 0 && a % 8 == 0)
        hipLaunchKernelGGL(k_value_features_finish<float2>, dim3(g), dim3(256), 0, st, (const float2*)feat_pad, src_row,
                           T, n / 2, rows_cap, H, (const float2*)time_tab, (float2*)out);
    else
        hipLaunchKernelGGL(k_value_features_finish<float>, dim3(g), dim3(256), 0, st, feat_pad, src_row, T, (int)n,
                           rows_cap, H, time_tab, out);
    return (int)hipGetLastError();
}

}  // extern "C"
