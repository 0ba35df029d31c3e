// philox.h — the counter-based generator under the device actor's noise (act.hip)
// and the minibatch draws (minibatch.hip); samplers/device_actor.py:philox4x32 states
// the same in NumPy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mjrl {

// Philox4x32-10 (Salmon et al., SC'11; Random123's philox4x32_R(10, ...)).
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c[0]), l0 = 0xD2511F53u * c[0];
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c[2]), l1 = 0xCD9E8D57u * c[2];
        c[0] = h1 ^ c[1] ^ k0;
        c[1] = l1;
        c[2] = h0 ^ c[3] ^ k1;
        c[3] = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

}  // namespace mjrl
