// maxpro_index.h — the definitions of the MaxPro Latin-hypercube generator (gpb_maxpro.hip) that a host program can include and
// tests/maxpro_reference.py restates: the scale of a pair term, ln psi from the objective, the decoding of a proposal from the
// four Philox words, and the strided row loop of a wave.  Plain integer and fp64 arithmetic, free of HIP
// (tests/host/maxpro_index_check.cpp runs it on the host).
//
// Levels l[i][c] in {0 .. n-1}, every column a permutation; the design is x = (l + 0.5) / n.  A pair term is
//     t_ij = prod_c (s (l_ic - l_jc))^-2,   s = e^1.5 / n     (= prod_c (e^1.5 (x_ic - x_jc))^-2 for a real design),
// the objective f = ln sum_{i<j} t_ij, and the MaxPro criterion (Joseph, Gul, Ba 2015)
//     psi = (mean_{i<j} prod_c (x_ic - x_jc)^-2)^(1/d):    ln psi = (f + 3 d - ln(n (n - 1) / 2)) / d.
// With this s a typical factor averages 1 in the log: neither the close pairs nor the far ones leave the fp64 range at d = 64.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MP_HD __host__ __device__
#else
#define MP_HD
#endif

namespace gpb {

constexpr int MP_MIN_N = 4, MP_MAX_N = 4096, MP_MIN_D = 2, MP_MAX_D = 64, MP_MAX_R = 16, MP_MAX_BLOCK = 64;
constexpr uint32_t MP_TAG = 11;                         // the fourth Philox counter word of a proposal (philox.h lists the tags)
constexpr double MP_E15 = 4.4816890703380645;           // e^1.5
constexpr int MP_WAVE = 64;
// An accepted state becomes the best so far when its sum lies below the best's by more than this fraction of it.  Hypercubes that
// mirror one another have sums that are equal up to rounding; which of them is kept must not hang on the order of a sum.
constexpr double MP_BEST_EPS = 1e-10;

MP_HD inline double mp_scale(int n) { return MP_E15 / (double)n; }

MP_HD inline double mp_lnpsi(double f, int n, int d) {
#pragma clang fp contract(off)
    const double pairs = 0.5 * (double)n * (double)(n - 1);
    return (f + 3.0 * (double)d - log(pairs)) / (double)d;
}

// A proposal: swap column c between the rows a != b; u in (0, 1) drives the acceptance.  From the Philox words (x, y, z, w) of
// the counter (global block index, restart, slot, MP_TAG): c = floor(x d / 2^32), a = floor(y n / 2^32), b one of the n - 1
// other rows (floor(z (n - 1) / 2^32), stepped over a), u = (w + 0.5) / 2^32.
struct MpProposal {
    int c, a, b;
    double u;
};
MP_HD inline MpProposal mp_decode(uint32_t x, uint32_t y, uint32_t z, uint32_t w, int n, int d) {
    MpProposal p;
    p.c = (int)(((uint64_t)x * (uint64_t)d) >> 32);
    p.a = (int)(((uint64_t)y * (uint64_t)n) >> 32);
    const int b0 = (int)(((uint64_t)z * (uint64_t)(n - 1)) >> 32);
    p.b = b0 + (b0 >= p.a ? 1 : 0);
    p.u = ((double)w + 0.5) * (1.0 / 4294967296.0);
    return p;
}

// the strided row loop: lane `lane` of a group of `width` serves the rows lane, lane + width, ... below n
MP_HD inline int mp_rows_of(int lane, int width, int n) { return lane < n ? (n - lane + width - 1) / width : 0; }
MP_HD inline int mp_row(int lane, int width, int k) { return lane + k * width; }

}  // namespace gpb
