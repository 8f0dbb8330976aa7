// philox.h — Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based
// generator behind the seeded control draws (control_kernels.hip).  One block of four words is a pure function of (counter, key):
// nothing is kept between calls, so a draw's words do not depend on thread, wave or launch shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cd {

struct Philox4 { uint32_t w[4]; };

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;  // the Weyl sequence of the key
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}
// the block of control draw k: key = the 64-bit seed, counter = (k low, k high, attempt, stream)
__host__ __device__ inline Philox4 control_draw_words(uint64_t seed, uint64_t k, uint32_t attempt, uint32_t stream) {
    return philox4x32_10((uint32_t)k, (uint32_t)(k >> 32), attempt, stream, (uint32_t)seed, (uint32_t)(seed >> 32));
}
// 52 random bits and a half: exact in double, inside [2^-53, 1 - 2^-53] — never 0 or 1, which qnorm could not take
__host__ __device__ inline double control_uniform(uint32_t r0, uint32_t r1) {
    return ((double)(r0 >> 6) * 67108864.0 + (double)(r1 >> 6) + 0.5) * 2.220446049250313e-16;  // 2^-52
}

}  // namespace cd
