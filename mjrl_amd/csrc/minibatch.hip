// minibatch.hip — the minibatch row indices of PPO's epochs, drawn on the device
// (DESIGN.md §1 row f7): what np.random.choice(T, mb) gives the reference per
// minibatch (mjrl/algos/ppo_clip.py:90-91), uniform on [0, T) with replacement, as a
// counter-based stream so that no host RNG and no upload stand between two epochs.
//
// Draw g of the stream of `seed` is a function of (seed, g, T) alone: block b = g >> 1
// of Philox4x32-10 on the counter (b lo, b hi, 0, 0) under the key (seed lo, seed hi ^
// "MBXI"), the 64-bit word u = x0 | x1 << 32 (g even) or x2 | x3 << 32 (g odd), and the
// index the high 64 bits of u T (bias at most T / 2^64).  algos/_device_sgd.py:
// minibatch_indices_reference states the same in NumPy.  The key's constant keeps the
// stream apart from the actor's noise (act.hip) under the same seed.
//
// One thread per Philox block; it stores whichever of its two draws lie in the
// requested range, so an odd first draw and an odd end need no second kernel.  Plain
// vector stores, no atomics, nothing outside idx[0 .. count).
#include "common.h"
#include "philox.h"

using namespace mjrl;

namespace {

constexpr uint32_t DRAW_KEY_TAG = 0x4D425849u;   // "MBXI"

__global__ void __launch_bounds__(NTHREADS) k_minibatch_indices(uint64_t seed, int64_t first, int64_t count,
                                                                uint64_t T, int64_t b0, int64_t nblocks,
                                                                int64_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
    if (i >= nblocks) return;
    const uint64_t b = (uint64_t)(b0 + i);
    uint32_t c[4] = {(uint32_t)b, (uint32_t)(b >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32) ^ DRAW_KEY_TAG);
    const int64_t at = (int64_t)(b << 1) - first;   // where draw 2b goes: -1 for the block of an odd first
    if (at >= 0 && at < count) idx[at] = (int64_t)__umul64hi((uint64_t)c[0] | (uint64_t)c[1] << 32, T);
    if (at + 1 >= 0 && at + 1 < count) idx[at + 1] = (int64_t)__umul64hi((uint64_t)c[2] | (uint64_t)c[3] << 32, T);
}

}  // namespace

extern "C" {

int mjrl_minibatch_indices(uint64_t seed, int64_t first, int64_t count, int64_t T, int64_t* idx, void* stream) {
    if (T < 1 || first < 0 || count < 0 || (count > 0 && !idx)) return MJRL_EINVAL;
    if (count == 0) return MJRL_OK;
    if (count > INT64_MAX - first) return MJRL_EINVAL;   // draw numbers stay below 2^63
    const int64_t b0 = first >> 1;
    const int64_t nblocks = ((first + count - 1) >> 1) - b0 + 1;
    const int64_t grid = (nblocks + NTHREADS - 1) / NTHREADS;
    if (grid > 0x7fffffff) return MJRL_EINVAL;
    hipLaunchKernelGGL(k_minibatch_indices, dim3((unsigned)grid), dim3(NTHREADS), 0, (hipStream_t)stream, seed, first,
                       count, (uint64_t)T, b0, nblocks, idx);
    return (int)hipGetLastError();
}

}  // extern "C"
