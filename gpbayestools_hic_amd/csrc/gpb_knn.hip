// gpb_knn.hip — nearest-neighbour distances of resident chains (gpb_chain_knn): for every row of A the kmax smallest squared
// distances to the rows of A itself or of another set B, brute force in fp64, the chains read through their strides as
// gpb_chain_kmeans reads them.  The rule of include/gpbayes.h is reproduced bit for bit by numpy (tests/knn_reference.py); this
// file is built with -ffp-contract=off (build.py), so that no t * t is fused into the sum.
//   k_knn_scale   a lane per row: z = x * inv_scale, padded with zeros to the width DP; a row with a scaled coordinate that is
//                 not finite is written as NaN throughout and counted.  Such a row needs no flag afterwards: every distance
//                 to or from it is NaN, which is neither < anything nor == 0.
//   k_knn_main    a workgroup per (tile of 256 query rows, range of B): a lane holds its query row and its sorted list of the
//                 KP nearest so far in registers (every index a compile-time constant); the rows of B come through LDS in tiles
//                 of 64 and are read as broadcasts, four rows at a time for four independent sums.  A candidate is first compared
//                 with the worst entry of the list; the insertion is the rare branch.  B is walked in ascending row number and
//                 a candidate enters only on strict <: equal distances stay in ascending row number.
//   k_knn_merge   a lane per query row: the lists of the ranges, range after range, entry after entry, through the same
//                 insertion — the rows of a later range have higher numbers, so (distance, row number) order survives.
// DESIGN.md section 29.
#include "gpb_internal.h"
#include "knn_plan.h"

namespace gpb {

namespace {

constexpr int KNN_THREADS = KNN_TILE_A;

// gpb_kmeans.hip's KmGeom: row G (counted outer axis first) is o = G / n_in, i = G % n_in, element j at x[o so + i si + j]
struct KnnGeom {
    int64_t so, si;
    unsigned n_in;
};

// counter: the rows written as NaN
template <int DP>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_scale(const double* __restrict__ x, KnnGeom g, int d, int64_t row0, int64_t n,
                                                           const double* __restrict__ inv, double* __restrict__ z,
                                                           unsigned long long* __restrict__ counter) {
    const int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
    int bad = 0;
    if (i < n) {
        const int64_t G = row0 + i, o = G / g.n_in, in = G - o * g.n_in;
        const double* p = x + o * g.so + in * g.si;
        double* out = z + i * DP;
        bool fin = true;
        for (int j = 0; j < d; ++j) {
            const double v = p[j] * inv[j];
            fin = fin && isfinite(v);
            out[j] = v;
        }
        for (int j = d; j < DP; ++j) out[j] = 0.0;
        if (!fin) {
            for (int j = 0; j < DP; ++j) out[j] = NAN;
            bad = 1;
        }
    }
    const int nb = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(counter, (unsigned long long)nb);
}

// (c, ci) into the ascending list where it is < an entry; the entries behind move down, the last falls out
template <int KP>
__device__ __forceinline__ void knn_insert(double (&r)[KP], int (&id)[KP], double c, int ci) {
#pragma unroll
    for (int q = KP - 1; q >= 1; --q) {
        const bool prev = c < r[q - 1], here = c < r[q];
        r[q] = prev ? r[q - 1] : (here ? c : r[q]);
        id[q] = prev ? id[q - 1] : (here ? ci : id[q]);
    }
    const bool first = c < r[0];
    r[0] = first ? c : r[0];
    id[0] = first ? ci : id[0];
}

// za [rows][DP]: the query rows of this slab; me0: the number of its first row in B (self mode) or -1; zb [nB][DP].
// blockIdx.y = s: the rows [s per_split, (s + 1) per_split) of B.  pr2, pidx [splits][stride][KP], pzeros [splits][stride].
template <int DP, int KP>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_main(const double* __restrict__ za, int rows, int64_t me0,
                                                          const double* __restrict__ zb, int64_t nB, int64_t per_split, int skip_zero,
                                                          double* __restrict__ pr2, int* __restrict__ pidx, int* __restrict__ pzeros,
                                                          int64_t stride) {
    __shared__ double tile[KNN_TILE_B * DP];
    const int tid = threadIdx.x, i = blockIdx.x * KNN_THREADS + tid;
    const bool live = i < rows;
    double z[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) z[j] = live ? za[(int64_t)i * DP + j] : NAN;
    const int me = me0 >= 0 ? (int)(me0 + i) : -1;
    double r[KP];
    int id[KP];
#pragma unroll
    for (int q = 0; q < KP; ++q) r[q] = INFINITY, id[q] = -1;
    int zeros = 0;
    const int64_t b0 = (int64_t)blockIdx.y * per_split, b1 = imin64(nB, b0 + per_split);
    for (int64_t t0 = b0; t0 < b1; t0 += KNN_TILE_B) {
        __syncthreads();
        for (int e = tid; e < KNN_TILE_B * DP; e += KNN_THREADS) tile[e] = t0 + e / DP < b1 ? zb[t0 * DP + e] : NAN;
        __syncthreads();
        const int nrow = (int)imin64(KNN_TILE_B, (b1 - t0 + 3) / 4 * 4);      // (the rows behind b1 are NaN)
#pragma unroll 1
        for (int rr = 0; rr < nrow; rr += 4) {
            const double* b = tile + rr * DP;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < DP; ++j) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double t = z[j] - b[u * DP + j];
                    acc[u] = acc[u] + t * t;
                }
                // Every eight coordinates the four sums are pinned: the loads of a tile's rows stay with their arithmetic (hoisted
                // to the top of the unrolled body they need 8 DP registers), and the arithmetic stays in front of the insertion
                // branches (sunk behind them, row by row, the rows loaded for it stay live across the branches: scratch at
                // DP = 64, and one dependent chain where four were meant).
                if ((j & 7) == 7) asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])::"memory");
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int cand = (int)(t0 + rr + u);
                const double c = acc[u];
                bool ok = cand != me;
                if (ok && c == 0.0) {
                    ++zeros;
                    ok = !skip_zero;
                }
                if (ok && c < r[KP - 1]) knn_insert<KP>(r, id, c, cand);
            }
        }
    }
    if (live) {
        const int64_t at = (int64_t)blockIdx.y * stride + i;
#pragma unroll
        for (int q = 0; q < KP; ++q) pr2[at * KP + q] = r[q], pidx[at * KP + q] = id[q];
        pzeros[at] = zeros;
    }
}

template <int KP>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_merge(const double* __restrict__ pr2, const int* __restrict__ pidx,
                                                           const int* __restrict__ pzeros, int splits, int rows, int64_t stride,
                                                           int kmax, double* __restrict__ r2, int* __restrict__ idx,
                                                           int* __restrict__ zeros) {
    const int i = blockIdx.x * KNN_THREADS + threadIdx.x;
    if (i >= rows) return;
    double r[KP];
    int id[KP];
#pragma unroll
    for (int q = 0; q < KP; ++q) r[q] = INFINITY, id[q] = -1;
    int nz = 0;
    for (int s = 0; s < splits; ++s) {
        const int64_t at = (int64_t)s * stride + i;
        nz += pzeros[at];
#pragma unroll
        for (int q = 0; q < KP; ++q) {
            const double c = pr2[at * KP + q];
            if (c < r[KP - 1]) knn_insert<KP>(r, id, c, pidx[at * KP + q]);
        }
    }
#pragma unroll
    for (int q = 0; q < KP; ++q)
        if (q < kmax) {
            r2[(int64_t)i * kmax + q] = r[q];
            if (idx) idx[(int64_t)i * kmax + q] = id[q];
        }
    if (zeros) zeros[i] = nz;
}

// the checks of a chain's sizes and strides (gpb_chain_kmeans' rule); nullptr: fine, g and n are set
const char* knn_geom(int64_t nsteps, int64_t nwalkers, int64_t d, int64_t step_stride, int64_t walker_stride, KnnGeom& g, int64_t& n) {
    if (nsteps < 1 || nwalkers < 1) return "need nsteps >= 1 and nwalkers >= 1";
    if (nsteps > 0x7fffffffLL || nwalkers > 0x7fffffffLL || (__int128)nsteps * nwalkers > 0x7fffffffLL)
        return "more than 2^31 - 1 rows (nsteps nwalkers)";
    if (walker_stride < d || step_stride < d) return "a stride below d (elements would alias)";
    const bool steps_outer = (__int128)step_stride >= (__int128)walker_stride * nwalkers;
    const bool walkers_outer = (__int128)walker_stride >= (__int128)step_stride * nsteps;
    if (!steps_outer && !walkers_outer) return "neither stride spans the other axis (elements would alias)";
    g = steps_outer ? KnnGeom{step_stride, walker_stride, (unsigned)nwalkers} : KnnGeom{walker_stride, step_stride, (unsigned)nsteps};
    n = nsteps * nwalkers;
    return nullptr;
}

}  // namespace

}  // namespace gpb

using namespace gpb;

#define KNN_ARG(msg) GPB_FAIL(GPB_E_ARG, std::string("gpb_chain_knn: ") + (msg))

extern "C" int gpb_chain_knn(gpb_ctx* ctx, const double* a_dev, int64_t a_nsteps, int64_t a_nwalkers, int64_t a_step_stride,
                             int64_t a_walker_stride, const double* b_dev, int64_t b_nsteps, int64_t b_nwalkers, int64_t b_step_stride,
                             int64_t b_walker_stride, int64_t d, const double* inv_scale_host, int kmax, int skip_zero, int splits,
                             int on_device, double* r2, int32_t* idx, int32_t* zeros, int64_t* n_skipped) {
    if (!ctx) return GPB_E_ARG;
    if (!a_dev) KNN_ARG("a_dev is NULL");
    if (d < 1 || d > MAX_D) KNN_ARG("d outside 1 .. 64");
    KnnGeom ga{}, gb{};
    int64_t nA = 0, nB = 0;
    if (const char* why = knn_geom(a_nsteps, a_nwalkers, d, a_step_stride, a_walker_stride, ga, nA)) KNN_ARG(std::string("A: ") + why);
    const bool cross = b_dev != nullptr;
    if (cross) {
        if (const char* why = knn_geom(b_nsteps, b_nwalkers, d, b_step_stride, b_walker_stride, gb, nB)) KNN_ARG(std::string("B: ") + why);
    } else {
        nB = nA;
    }
    if (kmax < 1 || kmax > KNN_MAX_K) KNN_ARG("kmax outside 1 .. 16");
    if (!inv_scale_host) KNN_ARG("inv_scale_host is NULL");
    for (int64_t j = 0; j < d; ++j)
        if (!(inv_scale_host[j] > 0.0) || !isfinite(inv_scale_host[j])) KNN_ARG("inv_scale_host must be finite and positive");
    if (splits < 0) KNN_ARG("splits below 0");
    if (skip_zero != 0 && skip_zero != 1) KNN_ARG("skip_zero must be 0 or 1");
    if (on_device != 0 && on_device != 1) KNN_ARG("on_device must be 0 or 1");
    if (!r2) KNN_ARG("r2 is NULL");
    if (!n_skipped) KNN_ARG("n_skipped is NULL");
    const int D = (int)d, DP = pick_dpad(d);
    GPB_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;

    const KnnPlan plan = knn_plan(nA, nB, DP, kmax, cross ? 0 : 1, splits, ctx->num_cu, (int64_t)GPB_KNN_WS_MB << 20);
    const int KP = plan.kp, staged = on_device ? 0 : 1;
    KnnWs ws;
    if (const int rc = ctx_carve(ctx, ctx->knn_ws, [&](Carver<int64_t>& c) {
            ws.lay(c, nB, plan.slab, DP, KP, kmax, plan.splits, cross ? 1 : 0, staged);
        }))
        return rc;
    std::vector<double> inv(DP, 1.0);
    for (int j = 0; j < D; ++j) inv[j] = inv_scale_host[j];
    GPB_HIP(hipMemsetAsync(ws.counters, 0, 2 * sizeof(int64_t), s));
    GPB_HIP(hipMemcpyAsync(ws.inv, inv.data(), sizeof(double) * DP, hipMemcpyHostToDevice, s));       // (inv outlives the last sync)
    const dim3 thr(KNN_THREADS);
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + KNN_THREADS - 1) / KNN_THREADS)); };
    auto* cnt = reinterpret_cast<unsigned long long*>(ws.counters);

    // ---- 1. the scaled copy of B (of A in self mode), once
    {
        const int rc = dispatched(ctx, with_dpad(DP, [&](auto Wd) {
            constexpr int DPAD = decltype(Wd)::value;
            hipLaunchKernelGGL(k_knn_scale<DPAD>, blocks(nB), thr, 0, s, cross ? b_dev : a_dev, cross ? gb : ga, D, (int64_t)0, nB,
                               (const double*)ws.inv, ws.zb, cnt + (cross ? 1 : 0));
            return 0;
        }), "k_knn_scale");
        if (rc) return rc;
    }

    // ---- 2. the slabs of A
    for (int64_t a0 = 0; a0 < nA; a0 += plan.slab) {
        const int rows = (int)imin64(plan.slab, nA - a0);
        const double* za = cross ? ws.za : ws.zb + a0 * DP;
        double* o_r2 = staged ? ws.fr2 : r2 + a0 * kmax;
        int* o_idx = !idx ? nullptr : staged ? ws.fidx : idx + a0 * kmax;
        int* o_zeros = !zeros ? nullptr : staged ? ws.fzeros : zeros + a0;
        const int rc = dispatched(ctx, with_dpad(DP, [&](auto Wd) {
            constexpr int DPAD = decltype(Wd)::value;
            if (cross)
                hipLaunchKernelGGL(k_knn_scale<DPAD>, blocks(rows), thr, 0, s, a_dev, ga, D, a0, (int64_t)rows, (const double*)ws.inv,
                                   ws.za, cnt);
            return with_int<4, 8, 16>(KP, [&](auto Wk) {
                constexpr int KPAD = decltype(Wk)::value;
                hipLaunchKernelGGL((k_knn_main<DPAD, KPAD>), dim3(blocks(rows).x, (unsigned)plan.splits), thr, 0, s, za, rows,
                                   cross ? (int64_t)-1 : a0, (const double*)ws.zb, nB, plan.per_split, skip_zero, ws.pr2, ws.pidx,
                                   ws.pzeros, plan.slab);
                hipLaunchKernelGGL(k_knn_merge<KPAD>, blocks(rows), thr, 0, s, (const double*)ws.pr2, (const int*)ws.pidx,
                                   (const int*)ws.pzeros, plan.splits, rows, plan.slab, kmax, o_r2, o_idx, o_zeros);
                return 0;
            });
        }), "k_knn_main");
        if (rc) return rc;
        if (staged) {
            GPB_HIP(hipMemcpyAsync(r2 + a0 * kmax, ws.fr2, sizeof(double) * (size_t)rows * kmax, hipMemcpyDeviceToHost, s));
            if (idx) GPB_HIP(hipMemcpyAsync(idx + a0 * kmax, ws.fidx, sizeof(int32_t) * (size_t)rows * kmax, hipMemcpyDeviceToHost, s));
            if (zeros) GPB_HIP(hipMemcpyAsync(zeros + a0, ws.fzeros, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToHost, s));
        }
    }
    int64_t counters[2];
    GPB_HIP(hipMemcpyAsync(counters, ws.counters, sizeof(counters), hipMemcpyDeviceToHost, s));
    GPB_HIP(hipStreamSynchronize(s));
    GPB_HIP(hipGetLastError());
    // self mode: the one scaled copy is A's, counted in counter 0
    n_skipped[0] = counters[0];
    n_skipped[1] = cross ? counters[1] : 0;
    return 0;
}
