// Philox4x32-10 (Salmon et al., SC 2011; the Random123 constants) and the counter layout of the engine's draws: what
// rng.hip and the kernels that draw inside a launch of their own (nway.hip, diffaug.hip, voxaug.hip) share.
#pragma once
#include "kernels.h"

namespace fmri {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct u32x4 {
    uint32_t w[4];
};

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return u32x4{{c0, c1, c2, c3}};
}

// Philox block `blk` of stream `sid` at the state's seed and offset
__device__ __forceinline__ u32x4 rng_block(const int64_t* __restrict__ state, uint64_t blk, uint32_t sid) {
    const uint64_t seed = (uint64_t)state[0];
    const uint64_t ctr = (uint64_t)state[1] + blk;
    return philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), sid, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ---- the normal draw: what rng_normal_kernel and the kernels that draw normals inside a launch of their own share ----
// u = (k + 0.5) * 2^-24 with k = w >> 8 is no fp32 number for k >= 2^23 (25 significant bits), and near u = 1 the half
// step it would be rounded by moves sqrt(-2 ln u) by far more than an ulp.  1 - u = ((2^24 - 1 - k) + 0.5) * 2^-24 IS one
// there, so the upper half of the interval goes through its complement: ln u = log1p(-(1 - u)), and the angle 2 pi u is
// taken as -2 pi (1 - u) (cos is even, sin odd).  Both halves evaluate the same real-valued map.
__device__ __forceinline__ float neg2_log_u(uint32_t w) {
    const uint32_t k = w >> 8;
    if (k < (1u << 23)) return -2.f * logf(((float)k + 0.5f) * 0x1p-24f);
    return -2.f * log1pf(-(((float)(0xFFFFFFu - k) + 0.5f) * 0x1p-24f));
}

__device__ __forceinline__ void sincos_2pi_u(uint32_t w, float& s, float& c) {
    const uint32_t k = w >> 8;
    const float two_pi = 6.28318530717958647692f;
    if (k < (1u << 23)) {
        sincosf(two_pi * (((float)k + 0.5f) * 0x1p-24f), &s, &c);
    } else {
        sincosf(two_pi * (((float)(0xFFFFFFu - k) + 0.5f) * 0x1p-24f), &s, &c);
        s = -s;
    }
}

__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float scale, float& z0, float& z1) {
    const float r = scale * sqrtf(neg2_log_u(wa));
    float s, c;
    sincos_2pi_u(wb, s, c);
    z0 = r * c;
    z1 = r * s;
}

}  // namespace fmri
