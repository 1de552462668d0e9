// gpb_marg.hip — corner-plot marginals of a resident chain (gpb_chain_marginals): per parameter a histogram over given bin edges
// and the number of samples outside them, per pair of parameters a B x B histogram — np.histogram / np.histogram2d of every
// column and column pair of a chain that lies in HBM as [nsteps, nwalkers, d] (the stretch sampler's store) or [nwalkers, nsteps,
// d] (the pickles), read through its strides.  Bin rule: x is in bin b of parameter j iff e[j][b] <= x < e[j][b + 1], the last
// bin also takes x == e[j][B]; everything else, NaN included, is outside.  With weights every sample adds the integer
// llrint(w_t * wscale) clamped to [0, 2^32] instead of 1.
//   k_marg_weights one lane per sample: its integer weight
//   k_marg_code    each value of the chain is read ONCE (fp64, a lane per (sample, parameter), the parameters fastest) and
//                  binary-searched in its parameter's edges (LDS); one byte per value, its bin or 255 = outside, goes to a [S, d]
//                  workspace; the same lanes count h1 and outside in an LDS table that is flushed once per workgroup
//   k_marg_pairs   a workgroup per (tile of pairs, range of samples): its pairs' B x B tables in LDS (u32, weighted u64), a lane
//                  per (sample, pair) with the pairs fastest — the lanes of a wave spread over the tables, which is what keeps a
//                  concentrated chain's equal codes from meeting in one address — reads two code bytes and does one LDS integer
//                  atomic; the non-zero bins are flushed once with global 64-bit integer atomics
// Every accumulation is an integer add: no floating-point sum anywhere, so the counts do not depend on arrival order, layout,
// the sample groups, on_device, the pairs that share the call or the outputs requested.
#include "gpb_internal.h"

namespace gpb {

namespace {

constexpr int MARG_THREADS = 256;
constexpr int MARG_MAX_B = 64;
constexpr int MARG_CODE_SLOTS = 2048;            // (parameters of a chunk) x (B + 1) edges, and as many h1 | outside counters, in LDS
constexpr int MARG_TILE_BYTES = 48 << 10;        // LDS of a pairs workgroup's tables: three workgroups fit a CU's 160 KiB
constexpr int MARG_MAX_TP = 256;                 // pairs of a tile at most
constexpr unsigned char MARG_OUT = 255;
typedef unsigned long long u64;

// How sample G (counted outer axis first) is found in the chain: G = o * n_in + i, element j at x[o * so + i * si + j].  The
// outer axis is the one whose stride spans the other (the steps of the sampler's store, the walkers of a pickle), so that
// consecutive samples are neighbours in memory; the counts do not depend on the order.  With weights nwalkers = 1 and G = t.
struct MargGeom {
    int64_t so, si;
    unsigned n_in;
};

__global__ __launch_bounds__(MARG_THREADS) void k_marg_weights(const double* __restrict__ w, double wscale, int64_t g0, int64_t Sg,
                                                               u64* __restrict__ qw) {
    const int64_t s = (int64_t)blockIdx.x * MARG_THREADS + threadIdx.x;
    if (s >= Sg) return;
    const double z = w[g0 + s] * wscale;
    u64 q = 0;                                                 // (NaN fails both comparisons)
    if (z >= 4294967296.0) q = 1ull << 32;
    else if (z > 0.0) q = (u64)llrint(z);
    qw[s] = q;
}

// pairs[p] = (i, j), all i < j in lexicographic order: lane i writes its row
__global__ __launch_bounds__(MARG_THREADS) void k_marg_allpairs(int64_t d, int* __restrict__ pairs) {
    const int64_t i = (int64_t)blockIdx.x * MARG_THREADS + threadIdx.x;
    if (i >= d - 1) return;
    int* p = pairs + 2 * (i * (2 * d - i - 1) / 2);
    for (int64_t j = i + 1; j < d; ++j, p += 2) {
        p[0] = (int)i;
        p[1] = (int)j;
    }
}

// ---------------------------------------------------------------------------------------------------------------- codes, h1
// blockIdx.x: a range of per_block samples of the group [g0, g0 + Sg); blockIdx.y: a chunk of PC parameters.
// codes (or nullptr) [Sg][d]; h1 [d][B] and outside [d] (do_h1) are added to.
__global__ __launch_bounds__(MARG_THREADS) void k_marg_code(const double* __restrict__ x, MargGeom g, int64_t d, int B, int PC,
                                                            const double* __restrict__ edges, int64_t g0, int64_t Sg,
                                                            int64_t per_block, const u64* __restrict__ qw,
                                                            unsigned char* __restrict__ codes, int do_h1, u64* __restrict__ h1,
                                                            u64* __restrict__ outside) {
    __shared__ double se[MARG_CODE_SLOTS];
    __shared__ u64 sh[MARG_CODE_SLOTS];
    const int tid = threadIdx.x, B1 = B + 1;
    const int64_t j0 = (int64_t)blockIdx.y * PC;
    const int dc = (int)imin64(PC, d - j0);
    for (int k = tid; k < dc * B1; k += MARG_THREADS) {
        se[k] = edges[j0 * B1 + k];
        sh[k] = 0;
    }
    __syncthreads();
    const int64_t sb0 = (int64_t)blockIdx.x * per_block;
    const int64_t nloc = imin64(per_block, Sg - sb0);                    // (< 2^31: the launcher)
    const int64_t o0 = (g0 + sb0) / g.n_in;
    const unsigned i0 = (unsigned)((g0 + sb0) % g.n_in);
    const int q = MARG_THREADS / dc, r = MARG_THREADS % dc;
    int64_t ds = tid / dc;
    int jj = tid % dc;
    while (ds < nloc) {
        const unsigned iw = i0 + (unsigned)ds;                           // (i0 < 2^31, ds < 2^31)
        const int64_t o = o0 + iw / g.n_in, i = iw % g.n_in;
        const double v = x[o * g.so + i * g.si + j0 + jj];
        const double* e = se + jj * B1;
        int code = MARG_OUT;
        if (v >= e[0] && v <= e[B]) {                                    // (NaN: neither)
            int lo = 0, hi = B;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (v >= e[mid]) lo = mid;
                else hi = mid;
            }
            code = lo;
        }
        if (codes) codes[(sb0 + ds) * d + j0 + jj] = (unsigned char)code;
        if (do_h1) atomicAdd(&sh[jj * B1 + (code == MARG_OUT ? B : code)], qw ? qw[sb0 + ds] : 1ull);
        jj += r;
        ds += q;
        if (jj >= dc) {
            jj -= dc;
            ++ds;
        }
    }
    if (!do_h1) return;                                                  // (uniform)
    __syncthreads();
    for (int k = tid; k < dc * B1; k += MARG_THREADS) {
        const u64 v = sh[k];
        if (!v) continue;
        const int64_t j = j0 + k / B1;
        const int b = k % B1;
        atomicAdd(b < B ? &h1[j * B + b] : &outside[j], v);
    }
}

// ---------------------------------------------------------------------------------------------------------------- pairs
// blockIdx.x: TP pairs from p0 = blockIdx.x * TP; blockIdx.y: per_range samples of the group.  CT: u32 counts (a range holds
// fewer than 2^32 samples) or u64 weighted sums.  h2 [npairs][B][B] is added to.
template <typename CT>
__global__ __launch_bounds__(MARG_THREADS) void k_marg_pairs(const unsigned char* __restrict__ codes, const u64* __restrict__ qw,
                                                             const int* __restrict__ pairs, int64_t npairs, int64_t d, int B,
                                                             int TP, int64_t Sg, int64_t per_range, u64* __restrict__ h2) {
    extern __shared__ u64 marg_tiles[];
    __shared__ int pi[MARG_MAX_TP], pj[MARG_MAX_TP];
    CT* tile = reinterpret_cast<CT*>(marg_tiles);
    const int tid = threadIdx.x, BB = B * B;
    const int64_t p0 = (int64_t)blockIdx.x * TP;
    const int npt = (int)imin64(TP, npairs - p0);
    for (int k = tid; k < npt * BB; k += MARG_THREADS) tile[k] = 0;
    if (tid < npt) {
        pi[tid] = pairs[2 * (p0 + tid)];
        pj[tid] = pairs[2 * (p0 + tid) + 1];
    }
    __syncthreads();
    const int64_t s1 = imin64(Sg, ((int64_t)blockIdx.y + 1) * per_range);
    const int q = MARG_THREADS / npt, r = MARG_THREADS % npt;
    int64_t s = (int64_t)blockIdx.y * per_range + tid / npt;
    int p = tid % npt;
    while (s < s1) {
        const unsigned char* row = codes + s * d;
        const int a = row[pi[p]], b = row[pj[p]];
        if (a != MARG_OUT && b != MARG_OUT) atomicAdd(&tile[(p * B + a) * B + b], qw ? (CT)qw[s] : (CT)1);
        p += r;
        s += q;
        if (p >= npt) {
            p -= npt;
            ++s;
        }
    }
    __syncthreads();
    for (int k = tid; k < npt * BB; k += MARG_THREADS) {
        const CT v = tile[k];
        if (v) atomicAdd(&h2[p0 * BB + k], (u64)v);
    }
}

}  // namespace

// Everything of one call on the context's stream.  Workspace (8-byte units): edges [d][B + 1] | h1 [d][B] | outside [d] |
// h2 [npairs][B][B] | pairs [npairs][2] (int) | integer weights [Sg] | codes [Sg][d] (bytes); the results stay in it for the
// caller to copy out (st_h1, st_out, st_h2).
int launch_chain_marginals(gpb_ctx* ctx, const double* x, int64_t n, int64_t nw, int64_t d, int64_t ss, int64_t ws, bool steps_outer,
                           const double* edges_host, int B, const int32_t* pairs_host, int64_t npairs, const double* w, double wscale,
                           bool need_h1, bool need_h2, int64_t** st_h1, int64_t** st_out, int64_t** st_h2) {
    const int64_t S = n * nw, B1 = B + 1, BB = (int64_t)B * B;
    const int64_t n_edges = d * B1, n_h1 = d * B, n_h2 = need_h2 ? npairs * BB : 0, n_pairs = need_h2 ? npairs : 0;
    // the samples go through in groups whose codes (and integer weights) stay under the cap; the grouping changes no count
    const int64_t per_sample = (need_h2 ? d : 0) + (w ? 8 : 0);
    int64_t Sg = per_sample ? ctx->marg_ws_bytes / per_sample : S;
    Sg = Sg < 1 ? 1 : (Sg > S ? S : Sg);
    if (Sg > 0x40000000LL) Sg = 0x40000000LL;                    // (the kernels' 32-bit sample offsets)
    const int64_t n_qw = w ? Sg : 0, n_codes = need_h2 ? Sg * d : 0;            // (codes: bytes)
    MargWs mw;
    if (const int rc = ctx_carve(ctx, ctx->marg_ws, [&](Carver<int64_t>& c) { mw.lay(c, n_edges, n_h1, d, n_h2, n_pairs, n_qw, n_codes); }))
        return rc;
    double* edges = mw.edges;
    u64 *h1 = reinterpret_cast<u64*>(mw.h1), *out = reinterpret_cast<u64*>(mw.out), *h2 = reinterpret_cast<u64*>(mw.h2),
        *qw = reinterpret_cast<u64*>(mw.qw);
    int* pairs = mw.pairs;
    unsigned char* codes = mw.codes;
    GPB_HIP(hipMemcpyAsync(edges, edges_host, sizeof(double) * n_edges, hipMemcpyHostToDevice, ctx->stream));
    GPB_HIP(hipMemsetAsync(h1, 0, sizeof(u64) * (n_h1 + d + n_h2), ctx->stream));
    if (need_h2) {
        if (pairs_host)
            GPB_HIP(hipMemcpyAsync(pairs, pairs_host, sizeof(int) * 2 * npairs, hipMemcpyHostToDevice, ctx->stream));
        else
            hipLaunchKernelGGL(k_marg_allpairs, dim3((unsigned)((d + MARG_THREADS - 1) / MARG_THREADS)), dim3(MARG_THREADS), 0,
                               ctx->stream, d, pairs);
    }
    const MargGeom g = steps_outer ? MargGeom{ss, ws, (unsigned)nw} : MargGeom{ws, ss, (unsigned)n};
    const int PC = MARG_CODE_SLOTS / (int)B1;
    const int64_t nchunks = (d + PC - 1) / PC;
    const int64_t wgs = 8 * (int64_t)ctx->num_cu;                // workgroups a launch aims at: a few per CU, many samples each
    // pairs: as many B x B tables per workgroup as fit; the ranges so long that a flush is small against the codes read
    const int csz = w ? 8 : 4;
    const int TP = (int)imin64(imin64(MARG_TILE_BYTES / (BB * csz), MARG_MAX_TP), n_pairs > 0 ? n_pairs : 1);
    const int64_t ntiles = need_h2 ? (npairs + TP - 1) / TP : 0;
    if (nchunks > 65535) GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: too many parameters for one launch");
    for (int64_t g0 = 0; g0 < S; g0 += Sg) {
        const int64_t sg = imin64(Sg, S - g0);
        if (w)
            hipLaunchKernelGGL(k_marg_weights, dim3((unsigned)((sg + MARG_THREADS - 1) / MARG_THREADS)), dim3(MARG_THREADS), 0,
                               ctx->stream, w, wscale, g0, sg, qw);
        if (need_h1 || need_h2) {
            const int64_t dc = imin64(PC, d);
            int64_t nb = (sg * dc + 16 * MARG_THREADS - 1) / (16 * MARG_THREADS);      // 16 values per lane at least
            nb = nb < 1 ? 1 : (nb > wgs ? wgs : nb);
            const int64_t per_block = (sg + nb - 1) / nb;
            nb = (sg + per_block - 1) / per_block;
            hipLaunchKernelGGL(k_marg_code, dim3((unsigned)nb, (unsigned)nchunks), dim3(MARG_THREADS), 0, ctx->stream, x, g, d, B, PC,
                               edges, g0, sg, per_block, w ? qw : nullptr, need_h2 ? codes : nullptr, need_h1 ? 1 : 0, h1, out);
        }
        if (need_h2) {
            int64_t nr = (wgs + ntiles - 1) / ntiles;
            nr = imin64(nr, (sg + 2047) / 2048);                 // 2048 samples per range at least
            nr = nr < 1 ? 1 : (nr > 65535 ? 65535 : nr);
            const int64_t per_range = (sg + nr - 1) / nr;
            nr = (sg + per_range - 1) / per_range;
            const size_t lds = (size_t)TP * BB * csz;
            if (w)
                hipLaunchKernelGGL(k_marg_pairs<u64>, dim3((unsigned)ntiles, (unsigned)nr), dim3(MARG_THREADS), lds, ctx->stream,
                                   codes, qw, pairs, npairs, d, B, TP, sg, per_range, h2);
            else
                hipLaunchKernelGGL(k_marg_pairs<unsigned>, dim3((unsigned)ntiles, (unsigned)nr), dim3(MARG_THREADS), lds, ctx->stream,
                                   codes, nullptr, pairs, npairs, d, B, TP, sg, per_range, h2);
        }
    }
    GPB_HIP(hipGetLastError());
    *st_h1 = reinterpret_cast<int64_t*>(h1);
    *st_out = reinterpret_cast<int64_t*>(out);
    *st_h2 = reinterpret_cast<int64_t*>(h2);
    return 0;
}

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_chain_marginals(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d, int64_t step_stride,
                                   int64_t walker_stride, const double* edges_host, int B, const int32_t* pairs_host, int64_t npairs,
                                   const double* w_dev, double wscale, int on_device, int64_t* h1, int64_t* h2, int64_t* outside) {
    if (!ctx || !x_dev || !edges_host) return GPB_E_ARG;
    if (nsteps < 1 || nwalkers < 1 || d < 1) GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: need nsteps >= 1, nwalkers >= 1 and d >= 1");
    if (nsteps > 0x7fffffffLL || nwalkers > 0x7fffffffLL || d > 0x7fffffffLL)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: more than 2^31 - 1 steps, walkers or parameters");
    if (B < 1 || B > MARG_MAX_B) GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: B outside 1 .. 64");
    if (walker_stride < d || step_stride < d) GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: a stride below d (elements would alias)");
    const bool steps_outer = (__int128)step_stride >= (__int128)walker_stride * nwalkers;
    const bool walkers_outer = (__int128)walker_stride >= (__int128)step_stride * nsteps;
    if (!steps_outer && !walkers_outer)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: neither stride spans the other axis (elements would alias)");
    if (w_dev && nwalkers != 1) GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: weights need nwalkers == 1 (a flat particle set)");
    if (w_dev && (!(wscale > 0.0) || !isfinite(wscale))) GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: wscale must be positive and finite");
    for (int64_t j = 0; j < d; ++j) {
        const double* e = edges_host + j * (B + 1);
        for (int b = 0; b <= B; ++b)
            if (!isfinite(e[b]) || (b > 0 && !(e[b] > e[b - 1])))
                GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: edges must be finite and strictly increasing");
    }
    if (npairs < 0) GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: npairs < 0");
    if ((__int128)npairs * B * B > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: npairs B^2 above 2^31 - 1");
    if (pairs_host) {
        for (int64_t p = 0; p < npairs; ++p) {
            const int64_t i = pairs_host[2 * p], j = pairs_host[2 * p + 1];
            if (i < 0 || i >= d || j < 0 || j >= d) GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: a pair index outside [0, d)");
            if (i == j) GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: a pair (i, i)");
        }
    } else if (h2 && npairs != d * (d - 1) / 2) {
        GPB_FAIL(GPB_E_ARG, "gpb_chain_marginals: without a pair list npairs must be d (d - 1) / 2");
    }
    const bool need_h2 = h2 && npairs > 0, need_h1 = h1 || outside;
    if (!need_h1 && !need_h2) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    int64_t *s_h1 = nullptr, *s_out = nullptr, *s_h2 = nullptr;
    if (const int rc = launch_chain_marginals(ctx, x_dev, nsteps, nwalkers, d, step_stride, walker_stride, steps_outer, edges_host, B,
                                              pairs_host, npairs, w_dev, wscale, need_h1, need_h2, &s_h1, &s_out, &s_h2))
        return rc;
    HostOut so(ctx, on_device != 0, true);
    so.at(h1, s_h1, d * B);
    so.at(outside, s_out, d);
    if (need_h2) so.at(h2, s_h2, npairs * B * B);
    return so.finish();
}
