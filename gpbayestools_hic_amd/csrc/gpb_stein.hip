// gpb_stein.hip — kernel Stein discrepancy of a resident point set and Stein thinning (gpb_stein_ksd, gpb_stein_thin): the Langevin
// Stein kernel of the inverse multiquadric base kernel, per pair of rows from the rows, their scores and b = Ginv x, brute force in
// fp64.  The rule of include/gpbayes.h is reproduced bit for bit by numpy (tests/stein_reference.py); this file is built with
// -ffp-contract=off (build.py), so that no product is fused into a sum, and uses the IEEE sqrt and division only.
//   k_stein_prep   a lane per row: x, b = Ginv x and g, padded with zeros to the width DP (a padded coordinate adds +0 to every
//                  sum); a row with a non-finite x, g or b is written as NaN throughout and counted — every kp to or from it is
//                  NaN, which is never < anything; obj = kp(i, i).
//   k_stein_pass   one thinning iteration.  Every workgroup first reduces the (min, row) partials the workgroups of the pass
//                  before left — the kernel boundary is the grid-wide barrier —, workgroup 0 records the pick and its ksd; the
//                  picked row goes to LDS and is read as a broadcast; a lane streams its rows' x, b, g once, adds 2 kp to obj and
//                  keeps its (min, row); the workgroup leaves one partial.  (value, row number) is compared at every level.
//   k_stein_ksd    a workgroup per (tile of 256 query rows, range of column chunks): a lane holds its query row's x, b, g in
//                  registers; the other side comes through LDS in tiles and is read as broadcasts, four rows at a time for four
//                  independent sets of sums.  One partial per (row, chunk of STEIN_CHUNK columns), summed in ascending column.
//   k_stein_rows   a lane per query row adds its chunk partials in ascending order.
//   k_stein_csum / k_stein_final   the sum over rows: block_sum (block_reduce.h) per 256 rows, the chunk sums in ascending order.
// DESIGN.md section 35.
#include "gpb_internal.h"
#include "block_reduce.h"
#include "stein_plan.h"

namespace gpb {

namespace {

static_assert(STEIN_CHUNK == GPB_STEIN_CHUNK, "the header names the chunk width");
static_assert(STEIN_ROW_CHUNK == REDUCE_THREADS && STEIN_THREADS == REDUCE_THREADS, "block_sum adds 256 rows");

// kp from the four sums of a pair (include/gpbayes.h)
__device__ __forceinline__ double stein_kp(double q, double t1, double t3, double t4, double tr) {
    const double s = sqrt(q), i1 = 1.0 / s, i2 = 1.0 / q, i3 = i1 * i2, i5 = i3 * i2;
    return (-3.0 * t1) * i5 + (tr + t3) * i3 + t4 * i1;
}

// the pair (row at xi, bi, gi; row at xj, bj, gj), DP coordinates each
template <int DP>
__device__ __forceinline__ double stein_pair(const double* __restrict__ xi, const double* __restrict__ bi, const double* __restrict__ gi,
                                             const double* xj, const double* bj, const double* gj, double tr) {
    double q = 1.0, t1 = 0.0, t3 = 0.0, t4 = 0.0;
#pragma unroll 4
    for (int l = 0; l < DP; ++l) {
        const double r = xi[l] - xj[l], h = bi[l] - bj[l], a = gi[l], c = gj[l];
        q = q + r * h;
        t1 = t1 + h * h;
        t3 = t3 + (a - c) * h;
        t4 = t4 + a * c;
    }
    return stein_kp(q, t1, t3, t4, tr);
}

template <int DP>
__global__ __launch_bounds__(STEIN_THREADS) void k_stein_prep(const double* __restrict__ x, int64_t xs, const double* __restrict__ g,
                                                              int64_t gs, int64_t n, int d, const double* __restrict__ ginv, double tr,
                                                              double* __restrict__ X, double* __restrict__ B, double* __restrict__ G,
                                                              double* __restrict__ obj, unsigned long long* __restrict__ counter) {
    const int64_t i = (int64_t)blockIdx.x * STEIN_THREADS + threadIdx.x;
    int bad = 0;
    if (i < n) {
        const double *px = x + i * xs, *pg = g + i * gs;
        double *ox = X + i * DP, *ob = B + i * DP, *og = G + i * DP;
        bool fin = true;
        for (int j = 0; j < d; ++j) {
            double acc = 0.0;
            for (int l = 0; l < d; ++l) acc = acc + ginv[j * d + l] * px[l];
            const double xv = px[j], gv = pg[j];
            fin = fin && isfinite(xv) && isfinite(gv) && isfinite(acc);
            ox[j] = xv, ob[j] = acc, og[j] = gv;
        }
        for (int j = d; j < DP; ++j) ox[j] = 0.0, ob[j] = 0.0, og[j] = 0.0;
        if (!fin) {
            for (int j = 0; j < DP; ++j) ox[j] = NAN, ob[j] = NAN, og[j] = NAN;
            bad = 1;
        }
        if (obj) obj[i] = fin ? stein_pair<DP>(ox, ob, og, ox, ob, og, tr) : NAN;
    }
    const int nb = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(counter, (unsigned long long)nb);
}

// (v, r) is a better minimum than (bv, br): r < 0 is "none"; equal values go to the lower row
__device__ __forceinline__ bool stein_better(double v, int r, double bv, int br) {
    if (r < 0) return false;
    if (br < 0) return true;
    return v < bv || (v == bv && r < br);
}

// the workgroup's minimum in every thread; sv [4], sr [4]: LDS, free again after the call
__device__ __forceinline__ void stein_block_min(double& v, int& r, double* sv, int* sr) {
    for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int orow = __shfl_xor(r, o, 64);
        if (stein_better(ov, orow, v, r)) v = ov, r = orow;
    }
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v, sr[threadIdx.x >> 6] = r;
    __syncthreads();
    v = sv[0], r = sr[0];
    for (int w = 1; w < STEIN_THREADS / 64; ++w)
        if (stein_better(sv[w], sr[w], v, r)) v = sv[w], r = sr[w];
    __syncthreads();
}

// pass t = 0 only scans obj; pass t >= 1 picks row pi_t from the partials of pass t - 1, records idx [t - 1] and ksd [t - 1]
// (workgroup 0), adds 2 kp(i, pi_t) to every obj and leaves the new partials.  Workgroup b owns the rows [b per_block, ...).
template <int DP>
__global__ __launch_bounds__(STEIN_THREADS) void k_stein_pass(const double* __restrict__ X, const double* __restrict__ B,
                                                              const double* __restrict__ G, double* __restrict__ obj, int64_t n,
                                                              int64_t per_block, double tr, int t, const double* __restrict__ pmin_in,
                                                              const int* __restrict__ prow_in, int nblk, double* __restrict__ pmin_out,
                                                              int* __restrict__ prow_out, double* __restrict__ S, int* __restrict__ idx,
                                                              double* __restrict__ ksd) {
    __shared__ double pick[3 * DP];
    __shared__ double sv[STEIN_THREADS / 64];
    __shared__ int sr[STEIN_THREADS / 64];
    const int tid = threadIdx.x;
    int pi = -1;
    if (t > 0) {
        double v = 0.0;
        int r = -1;
        for (int k = tid; k < nblk; k += STEIN_THREADS) {
            const double pv = pmin_in[k];
            const int pr = prow_in[k];
            if (stein_better(pv, pr, v, r)) v = pv, r = pr;
        }
        stein_block_min(v, r, sv, sr);
        pi = r;
        if (blockIdx.x == 0 && tid == 0) {
            const double s = pi >= 0 ? S[0] + v : NAN;
            S[0] = s;
            idx[t - 1] = pi;
            ksd[t - 1] = sqrt(s) / (double)t;
        }
        if (pi >= 0) {
            for (int e = tid; e < DP; e += STEIN_THREADS) {
                pick[e] = X[(int64_t)pi * DP + e];
                pick[DP + e] = B[(int64_t)pi * DP + e];
                pick[2 * DP + e] = G[(int64_t)pi * DP + e];
            }
        }
        __syncthreads();
    }
    double bv = 0.0;
    int br = -1;
    const int64_t r0 = (int64_t)blockIdx.x * per_block, r1 = imin64(n, r0 + per_block);
    for (int64_t i = r0 + tid; i < r1; i += STEIN_THREADS) {
        double o = obj[i];
        if (pi >= 0) {
            const double kp = stein_pair<DP>(X + i * DP, B + i * DP, G + i * DP, pick, pick + DP, pick + 2 * DP, tr);
            o = o + 2.0 * kp;
            obj[i] = o;
        }
        if (o == o && stein_better(o, (int)i, bv, br)) bv = o, br = (int)i;
    }
    stein_block_min(bv, br, sv, sr);
    if (tid == 0) pmin_out[blockIdx.x] = bv, prow_out[blockIdx.x] = br;
}

// how k_stein_ksd holds a query row at the padded width DP: LANES lanes per row, each with DP / LANES coordinates of x, b and g in
// registers; U rows of the other side per step.  Three vectors of 32 doubles are 192 registers: from DP = 48 on a row is split
// over two lanes (DESIGN.md section 35 has the compiler's resource report of every instantiation).
template <int DP>
struct SteinShape {
    static constexpr int LANES = DP > 32 ? 2 : 1;
    static constexpr int U = DP < 32 ? 4 : DP < 64 ? 2 : 1;
};

// X, B, G [n][DP]: all rows; the query rows of this launch are a0 .. a0 + rows - 1, STEIN_THREADS / LANES of them per workgroup.
// blockIdx.y = s: the chunks [s chunks_per, (s + 1) chunks_per) of STEIN_CHUNK columns.  part [chunks][stride]: (chunk, query row
// of the slab).  LANES = 2: lane 2k takes the coordinates [0, DP / 2) of row k from q = 1, t = 0; lane 2k + 1 continues the SAME
// sums over [DP / 2, DP) one step later, from the values its partner reached — the order of the rule, l ascending, is kept — and
// finishes kp; both lanes are busy in every step but the first and the last of a tile.
template <int DP, int LANES, int U>
__global__ __launch_bounds__(STEIN_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void k_stein_ksd(const double* __restrict__ X, const double* __restrict__ B,
                                                             const double* __restrict__ G, int64_t n, int64_t a0, int rows,
                                                             int64_t chunks_per, int64_t chunks, double tr, double* __restrict__ part,
                                                             int64_t stride) {
    static_assert(LANES == 1 || LANES == 2, "one lane or a pair of lanes per query row");
    constexpr int H = DP / LANES, QR = STEIN_THREADS / LANES, PIN = DP == 32 ? 2 : 4;     // coordinates between two pins
    constexpr int TB = DP > 32 ? 32 : 64;             // rows of the other side per LDS tile (at most 50 KB for the three arrays)
    // the second half of a tile's row lies PAD doubles further on, so that the two addresses a wave reads at once (its even and
    // its odd lanes') never fall into the same LDS bank (H * 8 bytes = 256 would)
    constexpr int PAD = (LANES == 2 && (H * 8) % 256 == 0) ? 2 : 0, RS = DP + PAD;
    static_assert(STEIN_CHUNK % TB == 0 && TB % U == 0 && DP % LANES == 0 && H % 4 == 0, "whole tiles, whole steps, whole halves");
    __shared__ double tx[TB * RS], tb[TB * RS], tg[TB * RS];
    const int tid = threadIdx.x, hf = tid % LANES, i = blockIdx.x * QR + tid / LANES;
    const bool live = i < rows;
    double x[H], b[H], g[H];
#pragma unroll
    for (int l = 0; l < H; ++l) {
        x[l] = live ? X[(a0 + i) * DP + hf * H + l] : NAN;
        b[l] = live ? B[(a0 + i) * DP + hf * H + l] : NAN;
        g[l] = live ? G[(a0 + i) * DP + hf * H + l] : NAN;
    }
    const int64_t c0 = (int64_t)blockIdx.y * chunks_per, c1 = imin64(chunks, c0 + chunks_per);
    for (int64_t c = c0; c < c1; ++c) {
        double acc = 0.0;
        const int64_t j0 = c * STEIN_CHUNK, j1 = imin64(n, j0 + STEIN_CHUNK);
        for (int64_t t0 = j0; t0 < j1; t0 += TB) {
            __syncthreads();
            for (int e = tid; e < TB * DP; e += STEIN_THREADS) {
                const int row = e / DP, l = e - row * DP, at = row * RS + l + (l >= H ? PAD : 0);
                const bool in = t0 + row < j1;
                tx[at] = in ? X[t0 * DP + e] : NAN;
                tb[at] = in ? B[t0 * DP + e] : NAN;
                tg[at] = in ? G[t0 * DP + e] : NAN;
            }
            __syncthreads();
            const int ngr = (int)imin64(TB / U, (j1 - t0 + U - 1) / U);        // (the rows behind j1 are NaN: they add +0)
            double kq[U], k1[U], k3[U], k4[U];                                  // what this lane reached in the step before
#pragma unroll
            for (int u = 0; u < U; ++u) kq[u] = 1.0, k1[u] = 0.0, k3[u] = 0.0, k4[u] = 0.0;
#pragma unroll 1
            for (int st = 0; st < ngr + LANES - 1; ++st) {
                const int grp = st - hf, gc = grp < 0 ? 0 : grp >= ngr ? ngr - 1 : grp;
                const int off = gc * U * RS + hf * (H + PAD);
                const double *px = tx + off, *pb = tb + off, *pg = tg + off;
                double q[U], t1[U], t3[U], t4[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if constexpr (LANES == 2) {
                        const double sq = __shfl_xor(kq[u], 1, 64), s1 = __shfl_xor(k1[u], 1, 64), s3 = __shfl_xor(k3[u], 1, 64),
                                     s4 = __shfl_xor(k4[u], 1, 64);
                        q[u] = hf ? sq : 1.0, t1[u] = hf ? s1 : 0.0, t3[u] = hf ? s3 : 0.0, t4[u] = hf ? s4 : 0.0;
                    } else {
                        q[u] = 1.0, t1[u] = 0.0, t3[u] = 0.0, t4[u] = 0.0;
                    }
                }
#pragma unroll
                for (int l = 0; l < H; ++l) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const double r = x[l] - px[u * RS + l], h = b[l] - pb[u * RS + l], cg = pg[u * RS + l];
                        q[u] = q[u] + r * h;
                        t1[u] = t1[u] + h * h;
                        t3[u] = t3[u] + (g[l] - cg) * h;
                        t4[u] = t4[u] + g[l] * cg;
                    }
                    // as in k_knn_main: every PIN coordinates the sums are pinned, so that the loads of a tile's rows stay with
                    // their arithmetic instead of being hoisted to the top of the unrolled body
                    if ((l & (PIN - 1)) == PIN - 1) {
#pragma unroll
                        for (int u = 0; u < U; ++u) asm volatile("" : "+v"(q[u]), "+v"(t1[u]), "+v"(t3[u]), "+v"(t4[u])::"memory");
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) kq[u] = q[u], k1[u] = t1[u], k3[u] = t3[u], k4[u] = t4[u];
                if (hf == LANES - 1 && grp >= 0 && grp < ngr) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const double kp = stein_kp(q[u], t1[u], t3[u], t4[u], tr);
                        acc = acc + (kp == kp ? kp : 0.0);                      // (a skipped row adds +0)
                    }
                }
            }
        }
        if (live && hf == LANES - 1) part[c * stride + i] = acc;
    }
}

__global__ __launch_bounds__(STEIN_THREADS) void k_stein_rows(const double* __restrict__ part, int64_t chunks, int64_t stride, int rows,
                                                              int64_t a0, const double* __restrict__ X, int dp, double* __restrict__ rs) {
    const int i = blockIdx.x * STEIN_THREADS + threadIdx.x;
    if (i >= rows) return;
    double a = 0.0;
    for (int64_t c = 0; c < chunks; ++c) a = a + part[c * stride + i];
    const double x0 = X[(a0 + i) * dp];
    rs[a0 + i] = x0 == x0 ? a : NAN;
}

__global__ __launch_bounds__(STEIN_THREADS) void k_stein_csum(const double* __restrict__ rs, const double* __restrict__ X, int dp,
                                                              int64_t n, double* __restrict__ csum) {
    __shared__ double sw[REDUCE_WAVES];
    const int64_t i = (int64_t)blockIdx.x * STEIN_THREADS + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        const double x0 = X[i * dp];
        if (x0 == x0) v = rs[i];
    }
    const double s = block_sum(v, sw);
    if (threadIdx.x == 0) csum[blockIdx.x] = s;
}

__global__ void k_stein_final(const double* __restrict__ csum, int64_t nchunks, int64_t n, const unsigned long long* __restrict__ counter,
                              double* __restrict__ ksd2) {
    double tot = 0.0;
    for (int64_t c = 0; c < nchunks; ++c) tot = tot + csum[c];
    const double nv = (double)(n - (int64_t)counter[0]);
    ksd2[0] = tot / (nv * nv);
}

// the checks both entry points share; nullptr: fine
const char* stein_args(const double* x_dev, const double* g_dev, int64_t n, int64_t d, int64_t xs, int64_t gs, const double* ginv,
                       int on_device) {
    if (!x_dev) return "x_dev is NULL";
    if (!g_dev) return "g_dev is NULL";
    if (n < 1 || n > 0x7fffffffLL) return "n outside 1 .. 2^31 - 1";
    if (d < 1 || d > MAX_D) return "d outside 1 .. 64";
    if (xs < d) return "x_row_stride below d (elements would alias)";
    if (gs < d) return "g_row_stride below d (elements would alias)";
    if (!ginv) return "ginv_host is NULL";
    for (int64_t j = 0; j < d * d; ++j)
        if (!isfinite(ginv[j])) return "ginv_host must be finite";
    for (int64_t j = 0; j < d; ++j)
        if (!(ginv[j * d + j] > 0.0)) return "ginv_host must have a positive diagonal";
    if (on_device != 0 && on_device != 1) return "on_device must be 0 or 1";
    return nullptr;
}

double stein_trace(const double* ginv, int64_t d) {
    double tr = 0.0;
    for (int64_t j = 0; j < d; ++j) tr = tr + ginv[j * d + j];
    return tr;
}

dim3 stein_blocks(int64_t n) { return dim3((unsigned)((n + STEIN_THREADS - 1) / STEIN_THREADS)); }

}  // namespace

}  // namespace gpb

using namespace gpb;

#define STEIN_ARG(fn, msg) GPB_FAIL(GPB_E_ARG, std::string(fn ": ") + (msg))

extern "C" int gpb_stein_thin(gpb_ctx* ctx, const double* x_dev, const double* g_dev, int64_t n, int64_t d, int64_t x_row_stride,
                              int64_t g_row_stride, const double* ginv_host, int64_t m, int on_device, int32_t* idx, double* ksd,
                              double* obj, int64_t* n_skipped) {
    if (!ctx) return GPB_E_ARG;
    if (const char* why = stein_args(x_dev, g_dev, n, d, x_row_stride, g_row_stride, ginv_host, on_device)) STEIN_ARG("gpb_stein_thin", why);
    if (m < 1 || m > STEIN_MAX_M) STEIN_ARG("gpb_stein_thin", "m outside 1 .. 2^20");
    if (!idx) STEIN_ARG("gpb_stein_thin", "idx is NULL");
    if (!ksd) STEIN_ARG("gpb_stein_thin", "ksd is NULL");
    if (!n_skipped) STEIN_ARG("gpb_stein_thin", "n_skipped is NULL");
    const int D = (int)d, DP = pick_dpad(d);
    GPB_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const SteinThinPlan plan = stein_thin_plan(n);
    SteinThinWs ws;
    if (const int rc = ctx_carve(ctx, ctx->stein_ws, [&](Carver<int64_t>& c) { ws.lay(c, n, d, DP, plan.blocks, m); })) return rc;
    HostOut so(ctx, on_device != 0, true);
    int* o_idx = so.at<int>(idx, ws.fidx, m);
    double* o_ksd = so.at<double>(ksd, ws.fksd, m);
    so.at<double>(obj, ws.obj, n);
    const double tr = stein_trace(ginv_host, d);
    GPB_HIP(hipMemsetAsync(ws.counter, 0, 2 * sizeof(int64_t), s));                                   // the counter and S = 0
    GPB_HIP(hipMemcpyAsync(ws.ginv, ginv_host, sizeof(double) * (size_t)(d * d), hipMemcpyHostToDevice, s));   // (pageable: staged at once)
    auto* cnt = reinterpret_cast<unsigned long long*>(ws.counter);
    const dim3 thr(STEIN_THREADS);
    const int rc = dispatched(ctx, with_dpad(DP, [&](auto Wd) {
        constexpr int DPAD = decltype(Wd)::value;
        hipLaunchKernelGGL(k_stein_prep<DPAD>, stein_blocks(n), thr, 0, s, x_dev, x_row_stride, g_dev, g_row_stride, n, D,
                           (const double*)ws.ginv, tr, ws.x, ws.b, ws.g, ws.obj, cnt);
        // the m + 1 passes, enqueued back to back: the kernel boundary is the only barrier, the host waits for nothing
        for (int64_t t = 0; t <= m; ++t) {
            const int in = (int)((t + 1) & 1), out = (int)(t & 1);
            hipLaunchKernelGGL(k_stein_pass<DPAD>, dim3((unsigned)plan.blocks), thr, 0, s, (const double*)ws.x, (const double*)ws.b,
                               (const double*)ws.g, ws.obj, n, plan.per_block, tr, (int)t, (const double*)ws.pmin[in],
                               (const int*)ws.prow[in], plan.blocks, ws.pmin[out], ws.prow[out], ws.S, o_idx, o_ksd);
        }
        return 0;
    }), "k_stein_pass");
    if (rc) return rc;
    if (const int rc2 = so.copy_back()) return rc2;
    int64_t counter = 0;
    GPB_HIP(hipMemcpyAsync(&counter, ws.counter, sizeof(counter), hipMemcpyDeviceToHost, s));
    GPB_HIP(hipStreamSynchronize(s));
    GPB_HIP(hipGetLastError());
    n_skipped[0] = counter;
    return 0;
}

extern "C" int gpb_stein_ksd(gpb_ctx* ctx, const double* x_dev, const double* g_dev, int64_t n, int64_t d, int64_t x_row_stride,
                             int64_t g_row_stride, const double* ginv_host, int splits, int on_device, double* row_sum, double* ksd2,
                             int64_t* n_skipped) {
    if (!ctx) return GPB_E_ARG;
    if (const char* why = stein_args(x_dev, g_dev, n, d, x_row_stride, g_row_stride, ginv_host, on_device)) STEIN_ARG("gpb_stein_ksd", why);
    if (splits < 0 || splits > STEIN_MAX_SPLITS) STEIN_ARG("gpb_stein_ksd", "splits outside 0 .. 64");
    if (!ksd2) STEIN_ARG("gpb_stein_ksd", "ksd2 is NULL");
    if (!n_skipped) STEIN_ARG("gpb_stein_ksd", "n_skipped is NULL");
    const int D = (int)d, DP = pick_dpad(d);
    GPB_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const SteinKsdPlan plan = stein_ksd_plan(n, splits, ctx->num_cu, (int64_t)GPB_STEIN_PART_MB << 20);
    SteinKsdWs ws;
    if (const int rc = ctx_carve(ctx, ctx->stein_ws, [&](Carver<int64_t>& c) { ws.lay(c, n, d, DP, plan.chunks, plan.slab); })) return rc;
    HostOut so(ctx, on_device != 0, true);
    so.at<double>(row_sum, ws.rs, n);
    double* o_ksd2 = so.at<double>(ksd2, ws.fksd2, 1);
    const double tr = stein_trace(ginv_host, d);
    GPB_HIP(hipMemsetAsync(ws.counter, 0, sizeof(int64_t), s));
    GPB_HIP(hipMemcpyAsync(ws.ginv, ginv_host, sizeof(double) * (size_t)(d * d), hipMemcpyHostToDevice, s));
    auto* cnt = reinterpret_cast<unsigned long long*>(ws.counter);
    const dim3 thr(STEIN_THREADS);
    const int64_t row_chunks = stein_ceil(n, STEIN_ROW_CHUNK);
    const int rc = dispatched(ctx, with_dpad(DP, [&](auto Wd) {
        constexpr int DPAD = decltype(Wd)::value;
        hipLaunchKernelGGL(k_stein_prep<DPAD>, stein_blocks(n), thr, 0, s, x_dev, x_row_stride, g_dev, g_row_stride, n, D,
                           (const double*)ws.ginv, tr, ws.x, ws.b, ws.g, (double*)nullptr, cnt);
        for (int64_t a0 = 0; a0 < n; a0 += plan.slab) {
            const int rows = (int)imin64(plan.slab, n - a0);
            using Shape = SteinShape<DPAD>;
            const unsigned tiles = (unsigned)stein_ceil(rows, STEIN_THREADS / Shape::LANES);
            hipLaunchKernelGGL((k_stein_ksd<DPAD, Shape::LANES, Shape::U>), dim3(tiles, (unsigned)plan.splits), thr, 0, s, (const double*)ws.x,
                               (const double*)ws.b, (const double*)ws.g, n, a0, rows, plan.chunks_per, plan.chunks, tr, ws.part,
                               plan.slab);
            hipLaunchKernelGGL(k_stein_rows, stein_blocks(rows), thr, 0, s, (const double*)ws.part, plan.chunks, plan.slab, rows, a0,
                               (const double*)ws.x, DPAD, ws.rs);
        }
        hipLaunchKernelGGL(k_stein_csum, dim3((unsigned)row_chunks), thr, 0, s, (const double*)ws.rs, (const double*)ws.x, DPAD, n,
                           ws.csum);
        return 0;
    }), "k_stein_ksd");
    if (rc) return rc;
    hipLaunchKernelGGL(k_stein_final, dim3(1), dim3(1), 0, s, (const double*)ws.csum, row_chunks, n, (const unsigned long long*)cnt, o_ksd2);
    if (const int rc2 = so.copy_back()) return rc2;
    int64_t counter = 0;
    GPB_HIP(hipMemcpyAsync(&counter, ws.counter, sizeof(counter), hipMemcpyDeviceToHost, s));
    GPB_HIP(hipStreamSynchronize(s));
    GPB_HIP(hipGetLastError());
    n_skipped[0] = counter;
    return 0;
}
