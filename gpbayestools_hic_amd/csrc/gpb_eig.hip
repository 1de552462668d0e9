// gpb_eig.hip — expected information gain of planned measurements (gpb_eig_simulate, gpb_eig_lse): the nested Monte Carlo
// estimator needs, for every simulated data vector y_i and every group of observables g, ln sum_{j != o_i} exp l_ij(g) over all
// inner samples j — S_out S_in M Gaussian terms whose S_out x S_in matrix is never formed.  The rule is in include/gpbayes.h and
// restated by tests/eig_reference.py.  Built with -ffp-contract=off (build.py): y = mu + sqrt(s) z is two roundings, which numpy
// reproduces from the returned z.
//   k_eig_check    counts the outer indices outside [0, S_in): the entry points refuse the call before anything reads through one.
//   k_eig_simulate a lane per (outer position, pair of observables): normal_pair of philox.h, tag 15.
//   k_eig_centre   a workgroup per observable: c_m = mean_j mu_jm, block_reduce.h's fixed tree.
//   k_eig_pack     a lane per (observable, sample): the k-major operand panels, row 2m and 2m + 1 of observable m — (t, u) of the
//                  inner set, (q, l) of the outer set — so that a group of observables is ONE contiguous K range; the columns
//                  behind S up to the next whole tile are zeros, the loads of the main kernel need no column edge.
//   k_eig_bias     a lane per (group, inner sample): b_gj.
//   k_eig_main     a workgroup per (tile of 64 outer rows, range of the inner axis, group), 4 waves (2 x 2) of 32 x 32 on
//                  v_mfma_f64_16x16x4_f64 through gemm_tile.h's fragments, LDS tiles and tile_mma; the K loop is this file's (the
//                  rows at and behind the group's end read as zeros).  After the K loop of an inner tile a lane holds 8 outer rows
//                  x 2 inner samples of the C fragment; it keeps a running maximum and a running sum of exponentials PER LANE AND
//                  ROW over the columns it sees — nothing crosses lanes inside the walk.  At the end the 16 lanes of a row are
//                  merged by a butterfly (both partners add the same two numbers: equal bits), the two wave columns through LDS.
//   k_eig_merge    a lane per (group, outer row): the ranges' (max, sum) pairs in range order, the logarithm, and self[g, i] from
//                  the raw inputs term by term.
// No floating-point atomics; the same call gives the same bits.  DESIGN.md section 31.
#include <algorithm>
#include "gpb_internal.h"
#include "block_reduce.h"
#include "eig_plan.h"
#include "gemm_tile.h"
#include "philox.h"

namespace gpb {

namespace {

constexpr int EIG_THREADS = 256;
constexpr uint32_t EIG_TAG = 15;
static_assert(EIG_TILE_OUT == 64 && EIG_TILE_IN == 64 && EIG_KB == 16 && EIG_THREADS == GEMM_THREADS, "k_eig_main's tile");

__global__ __launch_bounds__(EIG_THREADS) void k_eig_check(const int* __restrict__ oidx, int S_out, int S_in, int* __restrict__ bad) {
    const int i = blockIdx.x * EIG_THREADS + threadIdx.x;
    const int b = i < S_out && (oidx[i] < 0 || oidx[i] >= S_in);
    const int nb = __popcll(__ballot(b));
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(bad, nb);
}

// blockIdx.y: the pair of observables (2p, 2p + 1).  s = var + vadd, each 0 where its pointer is NULL.
__global__ __launch_bounds__(EIG_THREADS) void k_eig_simulate(const double* __restrict__ mu, const double* __restrict__ var,
                                                              const double* __restrict__ vadd, int M, int S_in, int64_t ld_in,
                                                              const int* __restrict__ oidx, int S_out, uint64_t seed,
                                                              double* __restrict__ y, double* __restrict__ z, int64_t ld_out) {
    const int i = blockIdx.x * EIG_THREADS + threadIdx.x, p = blockIdx.y;
    if (i >= S_out) return;
    const int o = oidx[i];
    if (o < 0 || o >= S_in) return;
    double n[2];
    normal_pair(seed, (uint32_t)i, (uint32_t)p, 0u, EIG_TAG, n[0], n[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int m = 2 * p + h;
        if (m >= M) break;
        const double s = (var ? var[m * ld_in + o] : 0.0) + (vadd ? vadd[m] : 0.0);
        const double r = sqrt(s) * n[h];
        y[m * ld_out + i] = mu[m * ld_in + o] + r;
        if (z) z[m * ld_out + i] = n[h];
    }
}

__global__ __launch_bounds__(REDUCE_THREADS) void k_eig_centre(const double* __restrict__ mu, int S_in, int64_t ld_in,
                                                               double* __restrict__ cen) {
    __shared__ double sw[REDUCE_WAVES];
    const int m = blockIdx.x;
    Kahan k;
    for (int j = threadIdx.x; j < S_in; j += REDUCE_THREADS) k.add(mu[m * ld_in + j]);
    const double tot = block_sum(k.s, sw);
    if (threadIdx.x == 0) cen[m] = tot / (double)S_in;
}

// INNER: rows (t, u) = (1 / s, (mu - c) / s) from mu, var, vadd;  else rows (q, l) = (-(y - c)^2 / 2, y - c) from y (in `mu`).
// blockIdx.y = m; columns x < S from the input, S <= x < sp zeros.
template <bool INNER>
__global__ __launch_bounds__(EIG_THREADS) void k_eig_pack(const double* __restrict__ mu, const double* __restrict__ var,
                                                          const double* __restrict__ vadd, const double* __restrict__ cen, int S,
                                                          int64_t ld, double* __restrict__ op, int64_t sp) {
    const int64_t x = (int64_t)blockIdx.x * EIG_THREADS + threadIdx.x;
    const int m = blockIdx.y;
    if (x >= sp) return;
    double r0 = 0.0, r1 = 0.0;
    if (x < S) {
        const double d = mu[m * ld + x] - cen[m];
        if (INNER) {
            const double s = (var ? var[m * ld + x] : 0.0) + (vadd ? vadd[m] : 0.0);
            r0 = 1.0 / s;
            r1 = d * r0;
        } else {
            r0 = -0.5 * (d * d);
            r1 = d;
        }
    }
    op[(int64_t)(2 * m) * sp + x] = r0;
    op[(int64_t)(2 * m + 1) * sp + x] = r1;
}

// ranges [G][4]: (first K row, end K row, the group's number in the caller's order, unused), heaviest group first.
// bias [gi][j] = ln w_j - sum_{m in g} [(mu_jm - c_m)^2 t_jm + ln s_jm] / 2
__global__ __launch_bounds__(EIG_THREADS) void k_eig_bias(const double* __restrict__ mu, const double* __restrict__ var,
                                                          const double* __restrict__ vadd, const double* __restrict__ logw,
                                                          const double* __restrict__ cen, int S_in, int64_t ld_in,
                                                          const int* __restrict__ ranges, double* __restrict__ bias, int64_t sp) {
    const int64_t j = (int64_t)blockIdx.x * EIG_THREADS + threadIdx.x;
    const int gi = blockIdx.y;
    if (j >= sp) return;
    double b = 0.0;
    if (j < S_in) {
        const int m0 = ranges[4 * gi] >> 1, m1 = ranges[4 * gi + 1] >> 1;
        double acc = 0.0;
        for (int m = m0; m < m1; ++m) {
            const double s = (var ? var[m * ld_in + j] : 0.0) + (vadd ? vadd[m] : 0.0);
            const double d = mu[m * ld_in + j] - cen[m];
            acc += (d * d) * (1.0 / s) + log(s);
        }
        b = (logw ? logw[j] : 0.0) - 0.5 * acc;
    }
    bias[(int64_t)gi * sp + j] = b;
}

// rows k0 .. k0 + KB of a k-major panel, the rows at and behind k_end as zeros (gload_direct of gemm_tile.h with a row edge in
// place of its column edge: the panels' columns are padded to whole tiles)
template <int T, int NW, int KB>
__device__ __forceinline__ void eig_gload(const double* __restrict__ G, int64_t ld, int k0, int64_t x0, int k_end,
                                          Frag<T, NW, KB>& f, int tid) {
    constexpr int TPR = T / 2, RPP = (64 * NW) / TPR;
    const int row = tid / TPR, col = (tid % TPR) * 2;
#pragma unroll
    for (int j = 0; j < (KB * T / 2) / (64 * NW); ++j) {
        const int k = k0 + row + RPP * j;
        if (k < k_end) f.r[j] = *reinterpret_cast<const d2*>(G + (int64_t)k * ld + x0 + col);
        else           f.r[j] = d2{0.0, 0.0};
    }
}

__device__ __forceinline__ double eig_ref(double m) { return m == -INFINITY ? 0.0 : m; }      // exp(-inf - ref) = 0, never NaN

// aop [2M][lda], bop [2M][ldb], bias [G][ldb]; blockIdx = (tile of outer rows, range of inner tiles, group in the table's order);
// pm, ps [G][splits][lda]
__global__ __launch_bounds__(EIG_THREADS) void k_eig_main(const double* __restrict__ aop, int64_t lda, const double* __restrict__ bop,
                                                          int64_t ldb, const double* __restrict__ bias, const int* __restrict__ oidx,
                                                          int S_out, int S_in, const int* __restrict__ ranges, int tiles_per_split,
                                                          int in_tiles, double* __restrict__ pm, double* __restrict__ ps) {
    constexpr int T = EIG_TILE_OUT, TN = EIG_TILE_IN, KB = EIG_KB, NW = 4;
    __shared__ TileLds<T, TN, KB> L;
    __shared__ double red_m[2][T], red_s[2][T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int m0 = (wave >> 1) * (T / 2), wc = wave & 1, n0 = wc * (TN / 2);
    const int gi = blockIdx.z, split = blockIdx.y, splits = gridDim.y;
    const int kb = ranges[4 * gi], ke = ranges[4 * gi + 1];
    const int64_t m_base = (int64_t)blockIdx.x * T;

    // the lane's 8 rows: q = 4 i + r is row m0 + 16 i + lk + 4 r of the tile (C fragment: reg r -> row (l >> 4) + 4 r)
    int own[8];
    double rm[8], rs[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int64_t row = m_base + m0 + 16 * (q >> 2) + lk + 4 * (q & 3);
        own[q] = row < S_out ? oidx[row] : -1;
        rm[q] = -INFINITY;
        rs[q] = 0.0;
    }

    const int t_begin = split * tiles_per_split, t_end = min(in_tiles, t_begin + tiles_per_split);
    for (int jt = t_begin; jt < t_end; ++jt) {
        const int64_t n_base = (int64_t)jt * TN;
        Acc<T, NW, TN> acc;
        acc_zero<T, NW, TN>(acc);
        Frag<T, NW, KB> fa;
        Frag<TN, NW, KB> fb;
        eig_gload<T, NW, KB>(aop, lda, kb, m_base, ke, fa, tid);
        eig_gload<TN, NW, KB>(bop, ldb, kb, n_base, ke, fb, tid);
        for (int k0 = kb; k0 < ke; k0 += KB) {
            __syncthreads();
            lstore_direct<T, NW, KB>(L.As, fa, tid);
            lstore_direct<TN, NW, KB>(L.Bs, fb, tid);
            __syncthreads();
            if (k0 + KB < ke) {
                eig_gload<T, NW, KB>(aop, lda, k0 + KB, m_base, ke, fa, tid);
                eig_gload<TN, NW, KB>(bop, ldb, k0 + KB, n_base, ke, fb, tid);
            }
            tile_mma<T, NW, TN, KB>(L, acc, lane, m0, n0);
        }
        // ---- the epilogue: bias, masks, the running (max, sum) of the lane's rows
        int col[2];
        double bj[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            col[j] = (int)n_base + n0 + 16 * j + lr;
            bj[j] = bias[(int64_t)gi * ldb + col[j]];              // (inside the padded row)
            if (col[j] >= S_in) col[j] = -2;                       // a column that no row may count
        }
        double v[8][2], mn[8];
        bool moved = false;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                v[q][j] = (col[j] == -2 || col[j] == own[q]) ? -INFINITY : acc.v[q >> 2][j][q & 3] + bj[j];
            mn[q] = fmax(rm[q], fmax(v[q][0], v[q][1]));
            moved = moved || mn[q] != rm[q];
        }
        if (__any(moved)) {                                        // (rare after the first tiles: the wave skips 8 exp)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                rs[q] = rs[q] * exp(rm[q] - eig_ref(mn[q]));
                rm[q] = mn[q];
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double ref = eig_ref(rm[q]);
            rs[q] = (rs[q] + exp(v[q][0] - ref)) + exp(v[q][1] - ref);
        }
    }

    // ---- the 16 lanes of a row (xor 1, 2, 4, 8 stays inside them), then the two wave columns in order
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        double mx = rm[q];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
        double sv = rs[q] * exp(rm[q] - eig_ref(mx));
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sv += __shfl_xor(sv, o, 64);
        if (lr == 0) {
            const int row = m0 + 16 * (q >> 2) + lk + 4 * (q & 3);
            red_m[wc][row] = mx;
            red_s[wc][row] = sv;
        }
    }
    __syncthreads();
    if (tid < T && m_base + tid < S_out) {
        const double a = red_m[0][tid], b = red_m[1][tid], mx = fmax(a, b), ref = eig_ref(mx);
        const int64_t at = ((int64_t)gi * splits + split) * lda + m_base + tid;
        pm[at] = mx;
        ps[at] = red_s[0][tid] * exp(a - ref) + red_s[1][tid] * exp(b - ref);
    }
}

// a lane per (outer row, group in the table's order); lse, self [G][S_out] in the caller's group order
__global__ __launch_bounds__(EIG_THREADS) void k_eig_merge(const double* __restrict__ pm, const double* __restrict__ ps, int splits,
                                                           int64_t lda, const double* __restrict__ mu, const double* __restrict__ var,
                                                           const double* __restrict__ vadd, const double* __restrict__ logw,
                                                           int64_t ld_in, const double* __restrict__ y, int64_t ld_out,
                                                           const int* __restrict__ oidx, int S_out, const int* __restrict__ ranges,
                                                           double* __restrict__ lse, double* __restrict__ self) {
    const int i = blockIdx.x * EIG_THREADS + threadIdx.x, gi = blockIdx.y;
    if (i >= S_out) return;
    const int m0 = ranges[4 * gi] >> 1, m1 = ranges[4 * gi + 1] >> 1, g = ranges[4 * gi + 2];
    double mx = -INFINITY, sv = 0.0;
    for (int s = 0; s < splits; ++s) {
        const int64_t at = ((int64_t)gi * splits + s) * lda + i;
        const double a = pm[at], mnew = fmax(mx, a), ref = eig_ref(mnew);
        sv = sv * exp(mx - ref) + ps[at] * exp(a - ref);
        mx = mnew;
    }
    lse[(int64_t)g * S_out + i] = sv > 0.0 ? mx + log(sv) : -INFINITY;
    const int o = oidx[i];
    double acc = 0.0;
    for (int m = m0; m < m1; ++m) {
        const double s = (var ? var[m * ld_in + o] : 0.0) + (vadd ? vadd[m] : 0.0);
        const double d = y[m * ld_out + i] - mu[m * ld_in + o];
        acc += (d * d) / s + log(s);
    }
    self[(int64_t)g * S_out + i] = (logw ? logw[o] : 0.0) - 0.5 * acc;
}

}  // namespace

}  // namespace gpb

using namespace gpb;

namespace {

// the checks the two entry points share; nullptr: fine
const char* eig_sizes(const void* mu_T, int64_t M, int64_t S_in, int64_t ld_in, const void* oidx, int64_t S_out, int64_t ld_out) {
    if (!mu_T) return "mu_T is NULL";
    if (!oidx) return "outer_idx_dev is NULL";
    if (M < 1 || M > EIG_MAX_M) return "M outside 1 .. 4096";
    if (S_in < 1 || S_out < 1) return "need S_in >= 1 and S_out >= 1";
    if (S_in > EIG_MAX_S || S_out > EIG_MAX_S) return "more than 2^31 - 65 samples";
    if (ld_in < S_in) return "ld_in below S_in";
    if (ld_out < S_out) return "ld_out below S_out";
    return nullptr;
}

// the outer indices are checked on the device, before any kernel reads through one (one small copy and a synchronisation)
int eig_check_indices(gpb_ctx* ctx, const char* who, const int* oidx, int64_t S_out, int64_t S_in, int* bad_dev) {
    hipStream_t s = ctx->stream;
    GPB_HIP(hipMemsetAsync(bad_dev, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_eig_check, dim3((unsigned)eig_ceil(S_out, EIG_THREADS)), dim3(EIG_THREADS), 0, s, oidx, (int)S_out, (int)S_in,
                       bad_dev);
    int bad = 0;
    GPB_HIP(hipMemcpyAsync(&bad, bad_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    GPB_HIP(hipStreamSynchronize(s));
    if (bad) GPB_FAIL(GPB_E_ARG, std::string(who) + ": " + std::to_string(bad) + " outer indices outside [0, S_in)");
    return 0;
}

}  // namespace

#define EIG_ARG(who, msg) GPB_FAIL(GPB_E_ARG, std::string(who ": ") + (msg))

extern "C" int gpb_eig_simulate(gpb_ctx* ctx, const double* mu_T, const double* var_T, const double* vadd_dev, int64_t M, int64_t S_in,
                                int64_t ld_in, const int32_t* outer_idx_dev, int64_t S_out, uint64_t seed, double* y_T, double* z_T,
                                int64_t ld_out) {
    if (!ctx) return GPB_E_ARG;
    if (const char* why = eig_sizes(mu_T, M, S_in, ld_in, outer_idx_dev, S_out, ld_out)) EIG_ARG("gpb_eig_simulate", why);
    if (!y_T) EIG_ARG("gpb_eig_simulate", "y_T is NULL");
    GPB_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int* bad = nullptr;
    if (const int rc = ctx_carve(ctx, ctx->eig_ws, [&](Carver<double>& c) { bad = c.take<int>(2, 2); })) return rc;
    if (const int rc = eig_check_indices(ctx, "gpb_eig_simulate", outer_idx_dev, S_out, S_in, bad)) return rc;
    hipLaunchKernelGGL(k_eig_simulate, dim3((unsigned)eig_ceil(S_out, EIG_THREADS), (unsigned)((M + 1) / 2)), dim3(EIG_THREADS), 0, s,
                       mu_T, var_T, vadd_dev, (int)M, (int)S_in, ld_in, outer_idx_dev, (int)S_out, seed, y_T, z_T, ld_out);
    GPB_HIP(hipGetLastError());
    GPB_HIP(hipStreamSynchronize(s));
    return 0;
}

extern "C" int gpb_eig_lse(gpb_ctx* ctx, const double* mu_T, const double* var_T, const double* vadd_dev, const double* logw_dev,
                           int64_t M, int64_t S_in, int64_t ld_in, const double* y_T, const int32_t* outer_idx_dev, int64_t S_out,
                           int64_t ld_out, const int32_t* ranges_host, int G, int splits, int on_device, double* lse_excl,
                           double* self) {
    if (!ctx) return GPB_E_ARG;
    if (const char* why = eig_sizes(mu_T, M, S_in, ld_in, outer_idx_dev, S_out, ld_out)) EIG_ARG("gpb_eig_lse", why);
    if (!y_T) EIG_ARG("gpb_eig_lse", "y_T is NULL");
    if (G < 1 || G > EIG_MAX_GROUPS) EIG_ARG("gpb_eig_lse", "G outside 1 .. 64");
    if (!ranges_host) EIG_ARG("gpb_eig_lse", "ranges_host is NULL");
    for (int g = 0; g < G; ++g)
        if (ranges_host[2 * g] < 0 || ranges_host[2 * g + 1] > M || ranges_host[2 * g] >= ranges_host[2 * g + 1])
            EIG_ARG("gpb_eig_lse", "group " + std::to_string(g) + " is empty or outside [0, M)");
    if (splits < 0 || splits > EIG_MAX_SPLITS) EIG_ARG("gpb_eig_lse", "splits outside 0 .. 64");
    if (on_device != 0 && on_device != 1) EIG_ARG("gpb_eig_lse", "on_device must be 0 or 1");
    if (!lse_excl || !self) EIG_ARG("gpb_eig_lse", "lse_excl or self is NULL");
    GPB_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;

    const EigPlan plan = eig_plan(S_out, S_in, G, splits, ctx->num_cu);
    const int staged = on_device ? 0 : 1;
    EigWs ws;
    if (const int rc = ctx_carve(ctx, ctx->eig_ws, [&](Carver<double>& c) {
            ws.lay(c, M, S_out, plan.sin_p, plan.sout_p, G, plan.splits, staged);
        }))
        return rc;
    if (const int rc = eig_check_indices(ctx, "gpb_eig_lse", outer_idx_dev, S_out, S_in, ws.bad)) return rc;

    // the groups' table, the heaviest first (a workgroup of the whole range runs as long as many of a single data set: it should
    // not start last); equal sizes keep the caller's order
    std::vector<int> order(G);
    for (int g = 0; g < G; ++g) order[g] = g;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return ranges_host[2 * a + 1] - ranges_host[2 * a] > ranges_host[2 * b + 1] - ranges_host[2 * b];
    });
    std::vector<int> table(4 * (size_t)G, 0);
    for (int gi = 0; gi < G; ++gi) {
        const int g = order[gi];
        table[4 * gi] = 2 * ranges_host[2 * g];
        table[4 * gi + 1] = 2 * ranges_host[2 * g + 1];
        table[4 * gi + 2] = g;
    }
    GPB_HIP(hipMemcpyAsync(ws.ranges, table.data(), sizeof(int) * table.size(), hipMemcpyHostToDevice, s));
                                                                   // (table outlives the last synchronisation)

    const dim3 thr(EIG_THREADS);
    const int Si = (int)S_in, So = (int)S_out;
    hipLaunchKernelGGL(k_eig_centre, dim3((unsigned)M), dim3(REDUCE_THREADS), 0, s, mu_T, Si, ld_in, ws.cen);
    hipLaunchKernelGGL(k_eig_pack<true>, dim3((unsigned)(plan.sin_p / EIG_THREADS + 1), (unsigned)M), thr, 0, s, mu_T, var_T, vadd_dev,
                       (const double*)ws.cen, Si, ld_in, ws.bop, plan.sin_p);
    hipLaunchKernelGGL(k_eig_pack<false>, dim3((unsigned)(plan.sout_p / EIG_THREADS + 1), (unsigned)M), thr, 0, s, y_T,
                       (const double*)nullptr, (const double*)nullptr, (const double*)ws.cen, So, ld_out, ws.aop, plan.sout_p);
    hipLaunchKernelGGL(k_eig_bias, dim3((unsigned)(plan.sin_p / EIG_THREADS + 1), (unsigned)G), thr, 0, s, mu_T, var_T, vadd_dev, logw_dev,
                       (const double*)ws.cen, Si, ld_in, (const int*)ws.ranges, ws.bias, plan.sin_p);
    hipLaunchKernelGGL(k_eig_main, dim3((unsigned)plan.out_tiles, (unsigned)plan.splits, (unsigned)G), thr, 0, s, (const double*)ws.aop,
                       plan.sout_p, (const double*)ws.bop, plan.sin_p, (const double*)ws.bias, outer_idx_dev, So, Si,
                       (const int*)ws.ranges, (int)plan.tiles_per_split, (int)plan.in_tiles, ws.pm, ws.ps);
    double* o_lse = staged ? ws.flse : lse_excl;
    double* o_self = staged ? ws.fself : self;
    hipLaunchKernelGGL(k_eig_merge, dim3((unsigned)eig_ceil(S_out, EIG_THREADS), (unsigned)G), thr, 0, s, (const double*)ws.pm,
                       (const double*)ws.ps, plan.splits, plan.sout_p, mu_T, var_T, vadd_dev, logw_dev, ld_in, y_T, ld_out,
                       outer_idx_dev, So, (const int*)ws.ranges, o_lse, o_self);
    GPB_HIP(hipGetLastError());
    if (staged) {
        GPB_HIP(hipMemcpyAsync(lse_excl, ws.flse, sizeof(double) * (size_t)G * S_out, hipMemcpyDeviceToHost, s));
        GPB_HIP(hipMemcpyAsync(self, ws.fself, sizeof(double) * (size_t)G * S_out, hipMemcpyDeviceToHost, s));
    }
    GPB_HIP(hipStreamSynchronize(s));
    return 0;
}
