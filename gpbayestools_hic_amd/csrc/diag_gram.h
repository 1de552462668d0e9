// diag_gram.h — the banded fp64 Gram product whose diagonal sums are lag sums: k_diag_gram, shared by gpb_diag.hip (the walkers'
// normalised series) and gpb_rank.hip (the split chains' centred series, section 32).  Y [parameter or
// series][nsp][nwp]: time t padded to 64, the series' index padded to 16, the padding exactly zero.  Every translation unit that
// includes this gets its own copy of the kernel.
#pragma once
#include "gemm_tile.h"

namespace gpb {

namespace {

// blockIdx.x = D * nb + I: block row I of block diagonal D (J = I + D); blockIdx.y: the parameter of the group.
// part[(jj * pstride + D * nb + I) * 128 + 63 + delta] = sum over the tile's diagonal col - row = delta, rows ascending; that
// diagonal is lag 64 D + delta.  Diagonal blocks (D = 0) hold each pair twice: only delta >= 0 is summed.
// The grid is the rectangle nd x nb: the workgroups with I + D >= nb (about half of them for the full band, few for a short one)
// leave at once — the price of an index that needs no square root; a triangular index would not launch them.
__global__ __launch_bounds__(GEMM_THREADS) void k_diag_gram(const double* __restrict__ Y, int64_t nsp, int64_t nwp, int64_t nb,
                                                            int64_t pstride, double* __restrict__ part) {
    __shared__ TileLds<64> lds;
    __shared__ double G[64][65];
    const int64_t D = (int64_t)blockIdx.x / nb, I = (int64_t)blockIdx.x % nb, J = I + D;
    if (J >= nb) return;                                   // (uniform: the whole workgroup leaves)
    const double* Yj = Y + (int64_t)blockIdx.y * nsp * nwp;
    Acc<64> acc;
    acc_zero<64>(acc);
    gemm_tile_loop<64, false, true, 4, 64, BK, true>(Yj, nwp, Yj, nwp, I * 64, J * 64, 64, 64, 0, nwp, lds, acc);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = (wave >> 1) * 32, n0 = (wave & 1) * 32, lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jn = 0; jn < 2; ++jn)
#pragma unroll
            for (int r = 0; r < 4; ++r) G[m0 + 16 * i + lk + 4 * r][n0 + 16 * jn + lr] = acc.v[i][jn][r];
    __syncthreads();
    if (tid < 127) {
        const int delta = tid - 63;
        double s = 0.0;
        if (D > 0 || delta >= 0) {
            const int r0 = delta < 0 ? -delta : 0, r1 = delta < 0 ? 64 : 64 - delta;
            for (int r = r0; r < r1; ++r) s += G[r][r + delta];
        }
        part[((int64_t)blockIdx.y * pstride + blockIdx.x) * 128 + tid] = s;
    }
}

}  // namespace

}  // namespace gpb
