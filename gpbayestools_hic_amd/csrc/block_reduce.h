// block_reduce.h — the fixed-order sums of the reduction kernels (gpb_ppd.hip, gpb_diag.hip): a compensated partial sum per thread,
// a wave butterfly, then the four waves of a 256-thread workgroup in order.  The tree's shape depends on nothing but the
// number of terms and the workgroup size: equal inputs give equal bits, no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace gpb {

constexpr int REDUCE_THREADS = 256;
constexpr int REDUCE_WAVES = REDUCE_THREADS / 64;

// compensated (Kahan) accumulation: the error of a thread's partial sum does not grow with the number of its terms
struct Kahan {
    double s = 0.0, c = 0.0;
    __device__ __forceinline__ void add(double x) {
        const double y = x - c, t = s + y;
        c = isinf(t) ? 0.0 : (t - s) - y;         // (a sum that overflows stays +-inf instead of turning into NaN)
        s = t;
    }
};

__device__ __forceinline__ double wave_sum(double v) {            // butterfly: every lane ends with the same bits
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum of v over the workgroup (REDUCE_THREADS threads), the same bits in every thread; sw: REDUCE_WAVES doubles of LDS (free again
// after the call)
static_assert(REDUCE_WAVES == 4, "block_sum adds four wave partials");
__device__ __forceinline__ double block_sum(double v, double* sw) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (sw[0] + sw[1]) + (sw[2] + sw[3]);
    __syncthreads();
    return r;
}

}  // namespace gpb
