// gpb_curves.hip — posterior bands of the parametrised curves of a resident chain (gpb_chain_curves) and its step-by-step
// trace histograms (gpb_chain_trace_hist): what examples/PlotMCMC.ipynb's plot_zeta_s_posterior / plot_eta_s_posterior /
// plot_yloss_posterior, compute_Delta_d and plot_chain_histogram take from a chain, for a chain that lies in HBM and is read
// through its strides as gpb_chain_marginals reads it.
// The value of curve c at grid point g for sample s, v(c, g, s) = curve_value(fn_c, theta_s[cols_c], aux, grid[c][g]) (curve_fn.h),
// is never stored for the select: the order statistics v_(k), v_(min(k + 1, S - 1)) of every row (c, g) come from a
// most-significant-digit radix select on the order-preserving key (order_key.h), eight passes of 8 bits, and every pass evaluates
// v again from the sample's three or four parameters.
//   k_crv_init     per (row, rank): no digits yet, the rank itself, one group
//   k_crv_count    a workgroup per (slab of samples, chunk of grid points, curve): a lane per sample loads its parameters once and
//                  walks the chunk's grid points; per (grid point, group of ranks with equal digits so far) a 256-bin table in LDS,
//                  one integer LDS atomic per key and group the key belongs to — one per wave where the whole wave meets in one
//                  bin, as it does in the first passes; non-zero bins are flushed with global integer atomics
//   k_crv_advance  a workgroup per row: takes the row's tables (and zeroes them), moves every rank one digit on, regroups the
//                  ranks; after the last pass writes the order statistics
//   k_crv_values   the materialised v, element (c, g, s) at (c G + g) ldv + s — small S, and the closure distance's [1, S] row
//   k_trace_hist   a workgroup per (step, chunk of parameters): the walkers' values searched in the parameter's edges (LDS, the
//                  bin rule of gpb_chain_marginals), counted in LDS and written once
// Every accumulation is an integer add and every kernel evaluates v through the same crv_load / crv_value: the results do not
// depend on arrival order, layout, slab size, on_device, or the curves and grid points that share the call.
#include "gpb_internal.h"
#include "curve_fn.h"
#include "order_key.h"

namespace gpb {

namespace {

constexpr int CRV_THREADS = 256;
constexpr int CRV_MAX_CURVES = 8, CRV_MAX_G = 1024, CRV_MAX_B = 64;
constexpr int CRV_RANKS = 2 * PPD_MAX_Q;
constexpr int CRV_TABLES = 32;                   // 256-bin u32 tables of a counting workgroup: 32 KiB of LDS
constexpr int CRV_VCHUNK = 32;                   // grid points of a k_crv_values workgroup
constexpr int TRACE_SLOTS = 2048;                // (parameters of a chunk) x (B + 1) edges and counters in LDS
typedef unsigned long long u64;

// sample s = t * nw + w, element j at x[t * ss + w * ws + j], whatever the layout
struct CrvGeom {
    int64_t ss, ws;
    unsigned nw;
    __device__ __forceinline__ const double* row(const double* x, int64_t s) const {
        const unsigned t = (unsigned)s / nw, w = (unsigned)s - t * nw;      // (s < 2^31: the entry point)
        return x + (int64_t)t * ss + (int64_t)w * ws;
    }
};

struct CrvDesc {
    int fn, c0, c1, c2, c3;
    __device__ __forceinline__ CrvDesc(const int* __restrict__ desc, int c)
        : fn(desc[c * 5]), c0(desc[c * 5 + 1]), c1(desc[c * 5 + 2]), c2(desc[c * 5 + 3]), c3(desc[c * 5 + 4]) {}
};

// What a sample contributes to a curve: its parameters (fn 0 .. 2) or, for fn 3, the closure distance itself in p0.
struct CrvSample {
    double p0, p1, p2, p3;
};
__device__ __forceinline__ CrvSample crv_load(const CrvDesc& k, const double* __restrict__ row, const double* __restrict__ aux, int d) {
    CrvSample a{0.0, 0.0, 0.0, 0.0};
    if (k.fn == CURVE_FN_DELTA) {
        a.p0 = curve_delta(row, aux, d);
    } else {
        a.p0 = row[k.c0];
        a.p1 = row[k.c1];
        a.p2 = row[k.c2];
        if (k.fn == CURVE_FN_ZETA) a.p3 = row[k.c3];
    }
    return a;
}
__device__ __forceinline__ double crv_value(int fn, const CrvSample& a, double g) {
    return fn == CURVE_FN_DELTA ? a.p0 : curve_param(fn, a.p0, a.p1, a.p2, a.p3, g);
}

// ---------------------------------------------------------------------------------------------------------------- select
__global__ __launch_bounds__(64) void k_crv_init(int nr, PpdLevels lv, u64* __restrict__ prefix, long long* __restrict__ rem,
                                                 u64* __restrict__ gprefix, int* __restrict__ grp, int* __restrict__ ngrp) {
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    long long k0 = 0;
#pragma unroll
    for (int r = 0; r < CRV_RANKS; ++r)             // (constant indices: the by-value argument stays in the kernel-argument segment)
        if (tid == r) k0 = lv.k[r];
    if (tid < nr) {
        prefix[row * nr + tid] = 0ull;
        rem[row * nr + tid] = k0;
        grp[row * nr + tid] = 0;
    }
    if (tid == 0) {
        gprefix[row * nr] = 0ull;
        ngrp[row] = 1;
    }
}

// blockIdx.x: per_block samples from blockIdx.x * per_block; blockIdx.y: GC grid points; blockIdx.z: the curve.  MG: tables per
// grid point in LDS (1 in the first pass, where no rank has a digit yet, else nr); GC * MG <= CRV_TABLES.
__global__ __launch_bounds__(CRV_THREADS) void k_crv_count(const double* __restrict__ x, CrvGeom gm, int d, int64_t S, int64_t per_block,
                                                           int G, int GC, int MG, int nr, int pass, const int* __restrict__ desc,
                                                           const double* __restrict__ aux, const double* __restrict__ grid,
                                                           const u64* __restrict__ gprefix, const int* __restrict__ ngrp,
                                                           unsigned* __restrict__ hist) {
    __shared__ unsigned sh[CRV_TABLES * 256];
    __shared__ u64 sgp[CRV_TABLES];
    __shared__ double sgrid[CRV_TABLES];
    __shared__ int sng[CRV_TABLES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c = blockIdx.z, g0 = blockIdx.y * GC;
    const int gc = min(GC, G - g0);
    const int64_t row0 = (int64_t)c * G + g0;
    const CrvDesc k(desc, c);
    for (int e = tid; e < gc * MG * 256; e += CRV_THREADS) sh[e] = 0u;
    if (tid < gc) {
        sgrid[tid] = grid[row0 + tid];
        sng[tid] = pass == 0 ? 1 : ngrp[row0 + tid];
    }
    if (tid < gc * MG) sgp[tid] = pass == 0 ? 0ull : gprefix[(row0 + tid / MG) * nr + tid % MG];
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const u64 mask = pass == 0 ? 0ull : ~0ull << (shift + 8);
    const int64_t s0 = (int64_t)blockIdx.x * per_block, s1 = imin64(S, s0 + per_block);
    for (int64_t base = s0; base < s1; base += CRV_THREADS) {       // (uniform: the wave votes below need every lane)
        const int64_t s = base + tid;
        const bool live = s < s1;
        CrvSample a{0.0, 0.0, 0.0, 0.0};
        if (live) a = crv_load(k, gm.row(x, s), aux, d);
        for (int gi = 0; gi < gc; ++gi) {
            const u64 key = ppd_key(crv_value(k.fn, a, sgrid[gi]));
            const u64 kp = key & mask;
            const int bin = (int)((key >> shift) & 255ull);
            const int ng = sng[gi];
            for (int g = 0; g < ng; ++g) {
                const bool in = live && kp == sgp[gi * MG + g];
                const u64 m = __ballot(in);
                if (!m) continue;                                  // (m is the same in every lane of the wave)
                unsigned* h = sh + (gi * MG + g) * 256;
                const int leader = __ffsll((long long)m) - 1;
                const int b0 = __shfl(bin, leader, 64);
                if (__ballot(in && bin == b0) == m) {
                    if (lane == leader) atomicAdd(&h[b0], (unsigned)__popcll(m));
                } else if (in) {
                    atomicAdd(&h[bin], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < gc * MG * 256; e += CRV_THREADS) {
        const unsigned v = sh[e];
        if (!v) continue;
        const int t = e >> 8, gi = t / MG, g = t % MG;
        atomicAdd(&hist[((row0 + gi) * nr + g) * 256 + (e & 255)], v);
    }
}

// A workgroup per row.  The tables of the row's ng groups lie at the front of its nr tables.
__global__ __launch_bounds__(CRV_THREADS) void k_crv_advance(int nr, int pass, unsigned* __restrict__ hist, u64* __restrict__ prefix,
                                                             long long* __restrict__ rem, u64* __restrict__ gprefix,
                                                             int* __restrict__ grp, int* __restrict__ ngrp, double* __restrict__ order) {
    __shared__ unsigned sh[CRV_RANKS * 256];
    __shared__ u64 sp[CRV_RANKS];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int ng = ngrp[row];
    unsigned* h = hist + row * nr * 256;
    for (int e = tid; e < ng * 256; e += CRV_THREADS) {
        sh[e] = h[e];
        h[e] = 0u;
    }
    __syncthreads();
    const int shift = 56 - 8 * pass;
    if (tid < nr) {
        const int g = grp[row * nr + tid];
        const long long want = rem[row * nr + tid];
        long long cum = 0;
        int b = 0;
        for (; b < 255; ++b) {
            const long long cnt = (long long)sh[g * 256 + b];
            if (want < cum + cnt) break;
            cum += cnt;
        }
        const u64 p = prefix[row * nr + tid] | ((u64)b << shift);
        prefix[row * nr + tid] = p;
        rem[row * nr + tid] = want - cum;
        sp[tid] = p;
        if (pass == 7) order[row * nr + tid] = ppd_unkey(p);
    }
    __syncthreads();
    if (tid == 0 && pass < 7) {
        int n = 0;
        for (int r = 0; r < nr; ++r) {
            int g = 0;
            while (g < n && gprefix[row * nr + g] != sp[r]) ++g;
            if (g == n) gprefix[row * nr + n++] = sp[r];
            grp[row * nr + r] = g;
        }
        ngrp[row] = n;
    }
}

// ---------------------------------------------------------------------------------------------------------------- values
__global__ __launch_bounds__(CRV_THREADS) void k_crv_values(const double* __restrict__ x, CrvGeom gm, int d, int64_t S, int64_t per_block,
                                                            int G, const int* __restrict__ desc, const double* __restrict__ aux,
                                                            const double* __restrict__ grid, double* __restrict__ values, int64_t ldv) {
    const int tid = threadIdx.x;
    const int c = blockIdx.z, g0 = blockIdx.y * CRV_VCHUNK;
    const int gc = min(CRV_VCHUNK, G - g0);
    const int64_t row0 = (int64_t)c * G + g0;
    const CrvDesc k(desc, c);
    const int64_t s0 = (int64_t)blockIdx.x * per_block, s1 = imin64(S, s0 + per_block);
    for (int64_t s = s0 + tid; s < s1; s += CRV_THREADS) {
        const CrvSample a = crv_load(k, gm.row(x, s), aux, d);
        for (int gi = 0; gi < gc; ++gi) values[(row0 + gi) * ldv + s] = crv_value(k.fn, a, grid[row0 + gi]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- trace histogram
// blockIdx.x: the step; blockIdx.y: a chunk of PC parameters.  hist [d][nsteps][B], outside [d][nsteps] (either may be nullptr).
__global__ __launch_bounds__(CRV_THREADS) void k_trace_hist(const double* __restrict__ x, int64_t ss, int64_t ws, int64_t nsteps,
                                                            int64_t nw, int64_t d, int B, int PC, const double* __restrict__ edges,
                                                            long long* __restrict__ hist, long long* __restrict__ outside) {
    __shared__ double se[TRACE_SLOTS];
    __shared__ unsigned sc[TRACE_SLOTS];
    const int tid = threadIdx.x, B1 = B + 1;
    const int64_t t = blockIdx.x, j0 = (int64_t)blockIdx.y * PC;
    const int dc = (int)imin64(PC, d - j0);
    for (int e = tid; e < dc * B1; e += CRV_THREADS) {
        se[e] = edges[j0 * B1 + e];
        sc[e] = 0u;
    }
    __syncthreads();
    const double* xt = x + t * ss + j0;
    const int q = CRV_THREADS / dc, r = CRV_THREADS % dc;
    int64_t w = tid / dc;
    int jj = tid % dc;
    while (w < nw) {
        const double v = xt[w * ws + jj];
        const double* e = se + jj * B1;
        int code = B;                                                    // outside (NaN: neither comparison holds)
        if (v >= e[0] && v <= e[B]) {
            int lo = 0, hi = B;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (v >= e[mid]) lo = mid;
                else hi = mid;
            }
            code = lo;
        }
        atomicAdd(&sc[jj * B1 + code], 1u);
        jj += r;
        w += q;
        if (jj >= dc) {
            jj -= dc;
            ++w;
        }
    }
    __syncthreads();
    for (int e = tid; e < dc * B1; e += CRV_THREADS) {
        const int64_t j = j0 + e / B1;
        const int b = e % B1;
        if (b < B) {
            if (hist) hist[(j * nsteps + t) * B + b] = (long long)sc[e];
        } else if (outside) {
            outside[j * nsteps + t] = (long long)sc[e];
        }
    }
}

// the slabs of S samples for a launch whose other grid dimensions hold `others` workgroups: whole multiples of the workgroup
void crv_slabs(const gpb_ctx* ctx, int64_t S, int64_t others, int64_t* nb, int64_t* per_block) {
    const int64_t wgs = 8 * (int64_t)ctx->num_cu;
    int64_t n = (wgs + others - 1) / others;
    n = imin64(n, (S + 4 * CRV_THREADS - 1) / (4 * CRV_THREADS));        // four samples per lane at least
    n = n < 1 ? 1 : n;
    *per_block = round_up((S + n - 1) / n, CRV_THREADS);
    *nb = (S + *per_block - 1) / *per_block;
}

// the shapes and strides rule gpb_chain_marginals applies, under the caller's name
int crv_check_chain(gpb_ctx* ctx, const char* who, int64_t nsteps, int64_t nwalkers, int64_t d, int64_t step_stride,
                    int64_t walker_stride) {
    const std::string w(who);
    if (nsteps < 1 || nwalkers < 1 || d < 1) GPB_FAIL(GPB_E_ARG, w + ": need nsteps >= 1, nwalkers >= 1 and d >= 1");
    if (nsteps > 0x7fffffffLL || nwalkers > 0x7fffffffLL || d > 0x7fffffffLL)
        GPB_FAIL(GPB_E_ARG, w + ": more than 2^31 - 1 steps, walkers or parameters");
    if (walker_stride < d || step_stride < d) GPB_FAIL(GPB_E_ARG, w + ": a stride below d (elements would alias)");
    const bool steps_outer = (__int128)step_stride >= (__int128)walker_stride * nwalkers;
    const bool walkers_outer = (__int128)walker_stride >= (__int128)step_stride * nsteps;
    if (!steps_outer && !walkers_outer) GPB_FAIL(GPB_E_ARG, w + ": neither stride spans the other axis (elements would alias)");
    return 0;
}

}  // namespace

}  // namespace gpb

using namespace gpb;

#define CRV_ARG(msg) GPB_FAIL(GPB_E_ARG, "gpb_chain_curves: " msg)

extern "C" int gpb_chain_curves(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d, int64_t step_stride,
                                int64_t walker_stride, int ncurves, const int32_t* desc_host, const double* aux_host,
                                const double* grid_host, int G, const double* q_host, int nq, int on_device, double* order,
                                double* values, int64_t ldv) {
    if (!ctx || !x_dev || !desc_host || !grid_host) return GPB_E_ARG;
    if (const int rc = crv_check_chain(ctx, "gpb_chain_curves", nsteps, nwalkers, d, step_stride, walker_stride)) return rc;
    if ((__int128)nsteps * nwalkers > 0x7fffffffLL) CRV_ARG("nsteps nwalkers above 2^31 - 1");
    const int64_t S = nsteps * nwalkers;
    if (ncurves < 1 || ncurves > CRV_MAX_CURVES) CRV_ARG("ncurves outside 1 .. 8");
    if (G < 1 || G > CRV_MAX_G) CRV_ARG("G outside 1 .. 1024");
    bool need_aux = false;
    for (int c = 0; c < ncurves; ++c) {
        const int32_t* k = desc_host + 5 * c;
        if (k[0] < 0 || k[0] > 3) CRV_ARG("fn outside 0 .. 3");
        if (k[0] == CURVE_FN_DELTA) {
            need_aux = true;
            continue;
        }
        const int npar = k[0] == CURVE_FN_ZETA ? 4 : 3;
        for (int i = 1; i <= npar; ++i)
            if (k[i] < 0 || k[i] >= d) CRV_ARG("a column outside [0, d)");
    }
    if (need_aux) {
        if (!aux_host) CRV_ARG("fn 3 needs aux (truth [d] | width [d])");
        for (int64_t j = 0; j < d; ++j) {
            if (!isfinite(aux_host[j])) CRV_ARG("aux: a truth value that is not finite");
            if (!isfinite(aux_host[d + j]) || !(aux_host[d + j] > 0.0)) CRV_ARG("aux: a width that is not finite and positive");
        }
    }
    for (int64_t i = 0; i < (int64_t)ncurves * G; ++i)
        if (!isfinite(grid_host[i])) CRV_ARG("a grid value that is not finite");
    PpdLevels lv;
    for (int i = 0; i < PPD_MAX_Q; ++i) {
        lv.q[i] = 0.0;
        lv.k[2 * i] = lv.k[2 * i + 1] = 0;
    }
    lv.nq = 0;
    if (order) {
        if (!q_host || nq < 1 || nq > PPD_MAX_Q) CRV_ARG("nq outside 1 .. 16");
        lv.nq = nq;
        for (int i = 0; i < nq; ++i) {
            const double q = q_host[i];
            if (!(q >= 0.0 && q <= 1.0)) CRV_ARG("a level outside [0, 1]");
            lv.q[i] = q;
            const long long k = (long long)floor(q * (double)(S - 1));       // numpy's virtual index (n - 1) q, floored
            lv.k[2 * i] = k;
            lv.k[2 * i + 1] = k + 1 < S ? k + 1 : S - 1;
        }
    }
    if (values && ldv < S) CRV_ARG("ldv < S");
    if (!order && !values) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    const int64_t R = (int64_t)ncurves * G, nr = order ? 2 * nq : 0;
    CurvesWs ws;
    if (const int rc = ctx_carve(ctx, ctx->curves_ws, [&](Carver<int64_t>& c) { ws.lay(c, ncurves, R, nr, need_aux ? 2 * d : 0); }))
        return rc;
    GPB_HIP(hipMemcpyAsync(ws.desc, desc_host, sizeof(int) * 5 * ncurves, hipMemcpyHostToDevice, ctx->stream));
    GPB_HIP(hipMemcpyAsync(ws.grid, grid_host, sizeof(double) * R, hipMemcpyHostToDevice, ctx->stream));
    if (need_aux) GPB_HIP(hipMemcpyAsync(ws.aux, aux_host, sizeof(double) * 2 * d, hipMemcpyHostToDevice, ctx->stream));
    HostOut so(ctx, on_device != 0);
    double *d_or, *d_va;
    so.out(d_or, order, R * nr);
    const int64_t ldw = so.out2d(d_va, values, R, S, ldv);
    if (const int rc = so.reserve()) return rc;
    const CrvGeom gm{step_stride, walker_stride, (unsigned)nwalkers};
    int64_t nb, per_block;
    if (order) {
        long long* rem = reinterpret_cast<long long*>(ws.rem);
        u64 *prefix = reinterpret_cast<u64*>(ws.prefix), *gprefix = reinterpret_cast<u64*>(ws.gprefix);
        GPB_HIP(hipMemsetAsync(ws.hist, 0, sizeof(unsigned) * R * nr * 256, ctx->stream));
        hipLaunchKernelGGL(k_crv_init, dim3((unsigned)R), dim3(64), 0, ctx->stream, (int)nr, lv, prefix, rem, gprefix, ws.grp, ws.ngrp);
        for (int pass = 0; pass < 8; ++pass) {
            const int MG = pass == 0 ? 1 : (int)nr;
            const int GC = (int)imin64(G, CRV_TABLES / MG);
            const int64_t nchunks = (G + GC - 1) / GC;
            crv_slabs(ctx, S, nchunks * ncurves, &nb, &per_block);
            hipLaunchKernelGGL(k_crv_count, dim3((unsigned)nb, (unsigned)nchunks, (unsigned)ncurves), dim3(CRV_THREADS), 0, ctx->stream,
                               x_dev, gm, (int)d, S, per_block, G, GC, MG, (int)nr, pass, ws.desc, ws.aux, ws.grid, gprefix, ws.ngrp,
                               ws.hist);
            hipLaunchKernelGGL(k_crv_advance, dim3((unsigned)R), dim3(CRV_THREADS), 0, ctx->stream, (int)nr, pass, ws.hist, prefix, rem,
                               gprefix, ws.grp, ws.ngrp, d_or);
        }
    }
    if (values) {
        const int64_t nchunks = (G + CRV_VCHUNK - 1) / CRV_VCHUNK;
        crv_slabs(ctx, S, nchunks * ncurves, &nb, &per_block);
        hipLaunchKernelGGL(k_crv_values, dim3((unsigned)nb, (unsigned)nchunks, (unsigned)ncurves), dim3(CRV_THREADS), 0, ctx->stream, x_dev,
                           gm, (int)d, S, per_block, G, ws.desc, ws.aux, ws.grid, d_va, ldw);
    }
    GPB_HIP(hipGetLastError());
    return so.finish();
}

#define TRC_ARG(msg) GPB_FAIL(GPB_E_ARG, "gpb_chain_trace_hist: " msg)

extern "C" int gpb_chain_trace_hist(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d, int64_t step_stride,
                                    int64_t walker_stride, const double* edges_host, int B, int on_device, int64_t* hist,
                                    int64_t* outside) {
    if (!ctx || !x_dev || !edges_host) return GPB_E_ARG;
    if (const int rc = crv_check_chain(ctx, "gpb_chain_trace_hist", nsteps, nwalkers, d, step_stride, walker_stride)) return rc;
    if (B < 1 || B > CRV_MAX_B) TRC_ARG("B outside 1 .. 64");
    for (int64_t j = 0; j < d; ++j) {
        const double* e = edges_host + j * (B + 1);
        for (int b = 0; b <= B; ++b)
            if (!isfinite(e[b]) || (b > 0 && !(e[b] > e[b - 1]))) TRC_ARG("edges must be finite and strictly increasing");
    }
    const int PC = TRACE_SLOTS / (B + 1);
    const int64_t nchunks = (d + PC - 1) / PC;
    if (nchunks > 65535) TRC_ARG("too many parameters for one launch");
    if (!hist && !outside) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    double* edges = nullptr;
    if (const int rc = ctx_carve(ctx, ctx->curves_ws, [&](Carver<int64_t>& c) { edges = c.take<double>(d * (B + 1)); })) return rc;
    GPB_HIP(hipMemcpyAsync(edges, edges_host, sizeof(double) * d * (B + 1), hipMemcpyHostToDevice, ctx->stream));
    HostOut so(ctx, on_device != 0);
    double *d_h, *d_o;                              // (64-bit counts: the stage is carved in 8-byte units)
    so.out(d_h, reinterpret_cast<double*>(hist), d * nsteps * B);
    so.out(d_o, reinterpret_cast<double*>(outside), d * nsteps);
    if (const int rc = so.reserve()) return rc;
    hipLaunchKernelGGL(k_trace_hist, dim3((unsigned)nsteps, (unsigned)nchunks), dim3(CRV_THREADS), 0, ctx->stream, x_dev, step_stride,
                       walker_stride, nsteps, nwalkers, d, B, PC, edges, reinterpret_cast<long long*>(d_h),
                       reinterpret_cast<long long*>(d_o));
    GPB_HIP(hipGetLastError());
    return so.finish();
}
