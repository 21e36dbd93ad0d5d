// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants): a counter-based
// generator -- four 32-bit words out of a 128-bit counter and a 64-bit key, no state.  The batch sampler keys every draw by what it
// is FOR (batch_sampler.hip), so results do not depend on the launch shape.  Host-callable so a CPU build can check the known answers.
#pragma once
#include <stdint.h>

namespace dispu {

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DISPU_HD __host__ __device__ __forceinline__
#else
#define DISPU_HD inline
#endif

DISPU_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 24-bit uniform in [0, 1): (w >> 8) * 2^-24, exact in fp32 (and so is 1 - u, in (0, 1])
DISPU_HD float philox_u01(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }

}  // namespace dispu
