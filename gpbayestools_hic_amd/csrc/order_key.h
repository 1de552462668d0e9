// order_key.h — the order-preserving 64-bit key of a double that the exact radix selects count digits of (gpb_ppd.hip's rows,
// gpb_curves.hip's re-evaluated curve values): unsigned keys in the order of the doubles, -0.0 in front of +0.0.
#pragma once
#include <hip/hip_runtime.h>

namespace gpb {

__device__ __forceinline__ unsigned long long ppd_key(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ppd_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

}  // namespace gpb
