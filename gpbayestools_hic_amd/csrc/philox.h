// philox.h — the counter-based generator of the device samplers (gpb_stretch.hip: the stretch move; gpb_ptlmc.hip: PTLMC).
// Philox4x32-10 (Salmon et al., SC'11) keyed by a 64-bit seed; oracle/stretch_oracle.py restates it.  The fourth counter
// word is a tag that keeps the draws of different purposes apart: 0, 1, 7 stretch move; 2, 3, 4 PTLMC; 8, 9, 10 SMC
// (gpb_smc.hip); 11 the swap proposals of the MaxPro design generator (gpb_maxpro.hip, MP_TAG of maxpro_index.h); 12, 13, 14
// HMC's momenta, step-size jitter and accept draws (gpb_hmc.hip); 15 the simulated measurements of the expected information gain
// (gpb_eig.hip); 16 the candidate rows of history matching (gpb_hm.hip, keyed by the absolute row).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace gpb {
struct U4 { uint32_t x, y, z, w; };
__device__ __forceinline__ U4 philox(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    U4 c = {c0, c1, c2, c3};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        U4 n;
        n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
        n.y = (uint32_t)p1;
        n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
        n.w = (uint32_t)p0;
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
__device__ __forceinline__ double u01(uint32_t hi, uint32_t lo) {   // 53-bit uniform in [0,1)
    const uint64_t b = (((uint64_t)hi << 32) | lo) >> 11;
    return (double)b * (1.0 / 9007199254740992.0);
}

// two N(0, 1) draws from the counter (c, k, j, tag): Box-Muller on two 53-bit uniforms, contraction off so that the host
// restatements (tests/ptlmc_reference.py, tests/smc_reference.py) follow it operation for operation
__device__ __forceinline__ void normal_pair(uint64_t seed, uint32_t c, uint32_t k, uint32_t j, uint32_t tag, double& n0,
                                            double& n1) {
#pragma clang fp contract(off)
    const U4 r = philox(seed, c, k, j, tag);
    const double u1 = u01(r.x, r.y), u2 = u01(r.z, r.w);
    const double rad = sqrt(-2.0 * log(1.0 - u1));
    const double a = 6.283185307179586 * u2;                  // 2 pi
    n0 = rad * cos(a);
    n1 = rad * sin(a);
}

}  // namespace gpb
