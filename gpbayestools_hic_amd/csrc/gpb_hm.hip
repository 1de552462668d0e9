// gpb_hm.hip — history matching (Craig et al. 1997; Vernon, Goldstein & Bower 2010): candidate rows in a box, the univariate
// implausibility of every candidate under every observable, and the maps of it over the parameters.
//   k_hm_uniform   gpb_hm_uniform: a lane per (row, parameter): x = lo + (hi - lo) u, u = u01 of philox(seed, R lo, R hi, j, 16) with
//                  R the ABSOLUTE row — a row's bits do not depend on how a call is cut into slabs.  Contraction off: the product
//                  and the sum round separately, which numpy restates bit for bit
//   k_hm_impl      gpb_hm_implausibility: a lane per sample walks its column of the observable-major mu_T / var_T (every load
//                  coalesced, eight observables' loads in flight), I_m = |y_m - mu| / sqrt(var + vadd_m); the K <= 4 largest kept in
//                  registers by a branch-free insertion (strict comparison: the lowest observable wins a tie), the maximum of every range of observables either in the same walk
//                  (ranges ascending and disjoint: the emulators of a chain) or in a walk of its own per range; the samples
//                  with an undefined I are counted by one integer atomic per wave
//   k_hm_key / k_hm_unkey  the minima as order_key.h's order-preserving 64-bit keys and back, in the caller's arrays
//   k_hm_code      as k_marg_code: every value of x read ONCE and binary-searched in its parameter's edges (LDS), a code byte per
//                  value; the same lanes keep (key minimum, count, NROY count) per (parameter, bin) in LDS, flushed once
//   k_hm_pairs     as k_marg_pairs: a workgroup per (tile of pairs, range of samples), the pairs' B x B tables of (u64 key
//                  minimum, u32 count, u32 NROY count) in LDS, a lane per (sample, pair) with the pairs fastest — the lanes of a
//                  wave spread over the tables, so a concentrated sample set does not serialise on one address; the bins that
//                  were hit are flushed with global 64-bit integer atomics
// Every accumulation is an integer add or an integer minimum: no floating-point reduction anywhere, so no output depends on
// arrival order, on the slabs a caller cuts the samples into, or on the outputs requested.
#include "gpb_internal.h"
#include "order_key.h"
#include "philox.h"

namespace gpb {

namespace {

constexpr int HM_THREADS = 256;
constexpr int HM_MAX_D = 512;
constexpr int HM_MAX_M = 4096;
constexpr int HM_MAX_K = 4;
constexpr int HM_MAX_G = 64;
constexpr int HM_UNROLL = 8;                     // observables whose loads a lane of k_hm_impl issues together
constexpr int HM_MAX_B = 64;
constexpr int HM_CODE_SLOTS = 2048;              // (parameters of a chunk) x (B + 1): edges and (key, count, NROY) tables in LDS, 48 KiB
constexpr int HM_TILE_BYTES = 64 << 10;          // LDS of a pairs workgroup's tables (16 bytes per bin): one pair at B = 64; two workgroups fit a CU's 160 KiB
constexpr int HM_MAX_TP = 256;
constexpr unsigned char HM_OUT = 255;
typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------------------- candidates
__global__ __launch_bounds__(HM_THREADS) void k_hm_uniform(const double* __restrict__ box, int d, uint64_t row0, int64_t S, uint64_t seed,
                                                           double* __restrict__ X, int64_t ld) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * HM_THREADS + threadIdx.x;
    if (e >= S * d) return;
    const int64_t r = e / d;
    const int j = (int)(e - r * d);
    const uint64_t R = row0 + (uint64_t)r;
    const U4 p = philox(seed, (uint32_t)R, (uint32_t)(R >> 32), (uint32_t)j, 16u);
    const double u = u01(p.x, p.y);
    const double lo = box[j], w = box[d + j] - lo;
    const double t = w * u;
    X[r * ld + j] = lo + t;
}

// ---------------------------------------------------------------------------------------------------------------- implausibility
struct HmRanges {
    int m0[HM_MAX_G], m1[HM_MAX_G];
};

__device__ __forceinline__ double hm_I(double y, double mu, double var, double vadd, bool& bad) {
    const double r = fabs(y - mu), v = var + vadd;
    if (v > 0.0 && r == r) {
        const double q = r / sqrt(v);
        return q == q ? q : 0.0;                                 // (inf / inf: an observable masked by vadd = +inf stays 0)
    }
    if (r == 0.0) return 0.0;
    bad = true;
    return INFINITY;
}

// inline_groups: the ranges are ascending and disjoint, their maxima come out of the one walk over the observables
__global__ __launch_bounds__(HM_THREADS) void k_hm_impl(const double* __restrict__ mu_T, const double* __restrict__ var_T, int M, int64_t S,
                                                        int64_t ld, const double* __restrict__ yexp, const double* __restrict__ vadd,
                                                        HmRanges rg, int G, int inline_groups, int K, double* __restrict__ top_T,
                                                        int* __restrict__ arg, double* __restrict__ gmax_T, int64_t ldo,
                                                        u64* __restrict__ bad_dev) {
    const int64_t s = (int64_t)blockIdx.x * HM_THREADS + threadIdx.x;
    const bool live = s < S;
    bool bad = false;
    if (live) {
        double t0 = -1.0, t1 = -1.0, t2 = -1.0, t3 = -1.0;       // (every I is >= 0)
        int a0 = 0;
        int cg = 0;
        double gm = -1.0;
        const bool groups = gmax_T && G > 0;
        // HM_UNROLL observables' loads are issued before the first is used: a lane has that many loads of each array in flight
        for (int mb = 0; mb < M; mb += HM_UNROLL) {
            double pm[HM_UNROLL], pv[HM_UNROLL];
#pragma unroll
            for (int u = 0; u < HM_UNROLL; ++u) {
                const bool in = mb + u < M;
                pm[u] = in ? mu_T[(int64_t)(mb + u) * ld + s] : 0.0;
                pv[u] = in && var_T ? var_T[(int64_t)(mb + u) * ld + s] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < HM_UNROLL; ++u) {
                const int m = mb + u;
                if (m >= M) break;                               // (uniform)
                const double I = hm_I(yexp[m], pm[u], pv[u], vadd ? vadd[m] : 0.0, bad);
                // insertion into the sorted four, branch-free; a strict comparison: the earlier of equal values stays in front
                a0 = I > t0 ? m : a0;
                double c = I;
                double n = c > t0 ? c : t0; c = c > t0 ? t0 : c; t0 = n;
                n = c > t1 ? c : t1; c = c > t1 ? t1 : c; t1 = n;
                n = c > t2 ? c : t2; c = c > t2 ? t2 : c; t2 = n;
                t3 = c > t3 ? c : t3;
                if (groups && inline_groups && cg < G) {         // (uniform over the wave)
                    if (m >= rg.m0[cg]) gm = I > gm ? I : gm;
                    if (m + 1 == rg.m1[cg]) {
                        gmax_T[(int64_t)cg * ldo + s] = gm;
                        gm = -1.0;
                        ++cg;
                    }
                }
            }
        }
        top_T[s] = t0;
        if (K > 1) top_T[ldo + s] = t1;
        if (K > 2) top_T[2 * ldo + s] = t2;
        if (K > 3) top_T[3 * ldo + s] = t3;
        if (arg) arg[s] = a0;
        if (groups && !inline_groups) {
            bool again = false;                                  // (counted above already)
            for (int g = 0; g < G; ++g) {
                double mx = -1.0;
                for (int m = rg.m0[g]; m < rg.m1[g]; ++m) {
                    const double I = hm_I(yexp[m], mu_T[(int64_t)m * ld + s], var_T ? var_T[(int64_t)m * ld + s] : 0.0,
                                          vadd ? vadd[m] : 0.0, again);
                    mx = I > mx ? I : mx;
                }
                gmax_T[(int64_t)g * ldo + s] = mx;
            }
        }
    }
    const u64 b = __ballot(live && bad);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(bad_dev, (u64)__popcll(b));
}

// ---------------------------------------------------------------------------------------------------------------- maps
// the minima of the caller's arrays as keys (init: the key of +inf and zero counts)
__global__ __launch_bounds__(HM_THREADS) void k_hm_key(double* __restrict__ mn, long long* __restrict__ cnt, long long* __restrict__ nroy,
                                                       int64_t n, int init) {
    const int64_t i = (int64_t)blockIdx.x * HM_THREADS + threadIdx.x;
    if (i >= n) return;
    u64* k = reinterpret_cast<u64*>(mn);
    k[i] = ppd_key(init ? (double)INFINITY : mn[i]);
    if (init) {
        cnt[i] = 0;
        nroy[i] = 0;
    }
}

__global__ __launch_bounds__(HM_THREADS) void k_hm_unkey(double* __restrict__ mn, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * HM_THREADS + threadIdx.x;
    if (i >= n) return;
    mn[i] = ppd_unkey(reinterpret_cast<const u64*>(mn)[i]);
}

__global__ __launch_bounds__(HM_THREADS) void k_hm_allpairs(int64_t d, int* __restrict__ pairs) {
    const int64_t i = (int64_t)blockIdx.x * HM_THREADS + threadIdx.x;
    if (i >= d - 1) return;
    int* p = pairs + 2 * (i * (2 * d - i - 1) / 2);
    for (int64_t j = i + 1; j < d; ++j, p += 2) {
        p[0] = (int)i;
        p[1] = (int)j;
    }
}

// blockIdx.x: per_block samples of the group [g0, g0 + Sg); blockIdx.y: a chunk of PC parameters.  codes (or nullptr) [Sg][d];
// key1 / cnt1 / nroy1 [d][B] (do_1d) take the minimum / are added to.
__global__ __launch_bounds__(HM_THREADS) void k_hm_code(const double* __restrict__ x, int64_t row_stride, int64_t d, int B, int PC,
                                                        const double* __restrict__ edges, const double* __restrict__ score, double cutoff,
                                                        int64_t g0, int64_t Sg, int64_t per_block, unsigned char* __restrict__ codes,
                                                        int do_1d, u64* __restrict__ key1, u64* __restrict__ cnt1, u64* __restrict__ nroy1) {
    __shared__ double se[HM_CODE_SLOTS];
    __shared__ u64 sk[HM_CODE_SLOTS];
    __shared__ unsigned sc[HM_CODE_SLOTS], sn[HM_CODE_SLOTS];
    const int tid = threadIdx.x, B1 = B + 1;
    const int64_t j0 = (int64_t)blockIdx.y * PC;
    const int dc = (int)imin64(PC, d - j0);
    const u64 kinf = ppd_key((double)INFINITY);
    for (int k = tid; k < dc * B1; k += HM_THREADS) {
        se[k] = edges[j0 * B1 + k];
        sk[k] = kinf;
        sc[k] = 0;
        sn[k] = 0;
    }
    __syncthreads();
    const int64_t sb0 = (int64_t)blockIdx.x * per_block;
    const int64_t nloc = imin64(per_block, Sg - sb0);
    const int q = HM_THREADS / dc, r = HM_THREADS % dc;
    int64_t ds = tid / dc;
    int jj = tid % dc;
    while (ds < nloc) {
        const int64_t row = g0 + sb0 + ds;
        const double v = x[row * row_stride + j0 + jj];
        const double* e = se + jj * B1;
        int code = HM_OUT;
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
        if (do_1d && code != HM_OUT) {
            const double sv = score[row];
            const int k = jj * B1 + code;
            atomicMin(&sk[k], ppd_key(sv));
            atomicAdd(&sc[k], 1u);
            if (sv < cutoff) atomicAdd(&sn[k], 1u);
        }
        jj += r;
        ds += q;
        if (jj >= dc) {
            jj -= dc;
            ++ds;
        }
    }
    if (!do_1d) return;                                                  // (uniform)
    __syncthreads();
    for (int k = tid; k < dc * B1; k += HM_THREADS) {
        const unsigned c = sc[k];
        const int b = k % B1;
        if (!c || b == B) continue;
        const int64_t o = (j0 + k / B1) * B + b;
        atomicMin(&key1[o], sk[k]);
        atomicAdd(&cnt1[o], (u64)c);
        if (sn[k]) atomicAdd(&nroy1[o], (u64)sn[k]);
    }
}

// blockIdx.x: TP pairs from p0 = blockIdx.x * TP; blockIdx.y: per_range samples of the group.  Dynamic LDS: keys [TP][B][B] (u64) |
// counts | NROY counts (u32 each): a range holds fewer than 2^32 samples.
__global__ __launch_bounds__(HM_THREADS) void k_hm_pairs(const unsigned char* __restrict__ codes, const double* __restrict__ score,
                                                         double cutoff, const int* __restrict__ pairs, int64_t npairs, int64_t d, int B,
                                                         int TP, int64_t Sg, int64_t per_range, u64* __restrict__ key2,
                                                         u64* __restrict__ cnt2, u64* __restrict__ nroy2) {
    extern __shared__ u64 hm_tiles[];
    const int tid = threadIdx.x, BB = B * B;
    const int64_t p0 = (int64_t)blockIdx.x * TP;
    const int npt = (int)imin64(TP, npairs - p0);
    u64* tk = hm_tiles;
    unsigned* tc = reinterpret_cast<unsigned*>(hm_tiles + (int64_t)TP * BB);
    unsigned* tn = tc + (int64_t)TP * BB;
    const u64 kinf = ppd_key((double)INFINITY);
    for (int k = tid; k < npt * BB; k += HM_THREADS) {
        tk[k] = kinf;
        tc[k] = 0;
        tn[k] = 0;
    }
    __syncthreads();
    const int64_t s1 = imin64(Sg, ((int64_t)blockIdx.y + 1) * per_range);
    const int q = HM_THREADS / npt, r = HM_THREADS % npt;
    int64_t s = (int64_t)blockIdx.y * per_range + tid / npt;
    int p = tid % npt;
    while (s < s1) {
        const unsigned char* row = codes + s * d;
        const int a = row[pairs[2 * (p0 + p)]], b = row[pairs[2 * (p0 + p) + 1]];
        if (a != HM_OUT && b != HM_OUT) {
            const double sv = score[s];
            const int k = (p * B + a) * B + b;
            atomicMin(&tk[k], ppd_key(sv));
            atomicAdd(&tc[k], 1u);
            if (sv < cutoff) atomicAdd(&tn[k], 1u);
        }
        p += r;
        s += q;
        if (p >= npt) {
            p -= npt;
            ++s;
        }
    }
    __syncthreads();
    for (int k = tid; k < npt * BB; k += HM_THREADS) {
        const unsigned c = tc[k];
        if (!c) continue;
        atomicMin(&key2[p0 * BB + k], tk[k]);
        atomicAdd(&cnt2[p0 * BB + k], (u64)c);
        if (tn[k]) atomicAdd(&nroy2[p0 * BB + k], (u64)tn[k]);
    }
}

inline unsigned hm_blocks(int64_t n) { return (unsigned)((n + HM_THREADS - 1) / HM_THREADS); }

}  // namespace

int launch_hm_uniform(gpb_ctx* ctx, const double* lo_host, const double* hi_host, int d, uint64_t row0, int64_t S, uint64_t seed,
                      double* X, int64_t ld) {
    HmWs hw;
    if (const int rc = ctx_carve(ctx, ctx->hm_ws, [&](Carver<int64_t>& c) { hw.lay(c, 2 * d, 0, 0, 0); })) return rc;
    GPB_HIP(hipMemcpyAsync(hw.box, lo_host, sizeof(double) * d, hipMemcpyHostToDevice, ctx->stream));
    GPB_HIP(hipMemcpyAsync(hw.box + d, hi_host, sizeof(double) * d, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_hm_uniform, dim3(hm_blocks(S * d)), dim3(HM_THREADS), 0, ctx->stream, hw.box, d, row0, S, seed, X, ld);
    GPB_HIP(hipGetLastError());
    return 0;
}

// Everything of one gpb_hm_maps call on the context's stream.  Workspace (8-byte units): edges [d][B + 1] | pairs [npairs][2]
// (int) | one code byte per (sample, parameter) of a sample group (ctx->marg_ws_bytes caps it, as for gpb_chain_marginals).
int launch_hm_maps(gpb_ctx* ctx, const double* x, int64_t S, int64_t d, int64_t row_stride, const double* score, double cutoff,
                   const double* edges_host, int B, const int32_t* pairs_host, int64_t npairs, int init, double* min1, int64_t* cnt1,
                   int64_t* nroy1, double* min2, int64_t* cnt2, int64_t* nroy2) {
    const bool need1 = min1 != nullptr, need2 = min2 != nullptr && npairs > 0;
    const int64_t B1 = B + 1, BB = (int64_t)B * B, n1 = d * B, n2 = npairs * BB;
    int64_t Sg = need2 ? ctx->marg_ws_bytes / d : S;
    Sg = Sg < 1 ? 1 : (Sg > S ? S : Sg);
    if (Sg > 0x40000000LL) Sg = 0x40000000LL;
    HmWs hw;
    if (const int rc = ctx_carve(ctx, ctx->hm_ws, [&](Carver<int64_t>& c) { hw.lay(c, 0, d * B1, need2 ? npairs : 0, need2 ? Sg * d : 0); }))
        return rc;
    GPB_HIP(hipMemcpyAsync(hw.edges, edges_host, sizeof(double) * d * B1, hipMemcpyHostToDevice, ctx->stream));
    if (need2) {
        if (pairs_host)
            GPB_HIP(hipMemcpyAsync(hw.pairs, pairs_host, sizeof(int) * 2 * npairs, hipMemcpyHostToDevice, ctx->stream));
        else
            hipLaunchKernelGGL(k_hm_allpairs, dim3(hm_blocks(d)), dim3(HM_THREADS), 0, ctx->stream, d, hw.pairs);
    }
    if (need1)
        hipLaunchKernelGGL(k_hm_key, dim3(hm_blocks(n1)), dim3(HM_THREADS), 0, ctx->stream, min1, reinterpret_cast<long long*>(cnt1),
                           reinterpret_cast<long long*>(nroy1), n1, init);
    if (need2)
        hipLaunchKernelGGL(k_hm_key, dim3(hm_blocks(n2)), dim3(HM_THREADS), 0, ctx->stream, min2, reinterpret_cast<long long*>(cnt2),
                           reinterpret_cast<long long*>(nroy2), n2, init);
    const int PC = HM_CODE_SLOTS / (int)B1;
    const int64_t nchunks = (d + PC - 1) / PC;                   // (d <= 2^31 - 1, PC >= 31: the launcher's grid holds it below)
    if (nchunks > 65535) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: too many parameters for one launch");
    const int64_t wgs = 8 * (int64_t)ctx->num_cu;
    const int TP = (int)imin64(imin64(HM_TILE_BYTES / (BB * 16), HM_MAX_TP), npairs > 0 ? npairs : 1);
    const int64_t ntiles = need2 ? (npairs + TP - 1) / TP : 0;
    for (int64_t g0 = 0; g0 < S; g0 += Sg) {
        const int64_t sg = imin64(Sg, S - g0);
        const int64_t dc = imin64(PC, d);
        int64_t nb = (sg * dc + 16 * HM_THREADS - 1) / (16 * HM_THREADS);
        nb = nb < 1 ? 1 : (nb > wgs ? wgs : nb);
        const int64_t per_block = (sg + nb - 1) / nb;
        nb = (sg + per_block - 1) / per_block;
        hipLaunchKernelGGL(k_hm_code, dim3((unsigned)nb, (unsigned)nchunks), dim3(HM_THREADS), 0, ctx->stream, x, row_stride, d, B, PC,
                           hw.edges, score, cutoff, g0, sg, per_block, need2 ? hw.codes : nullptr, need1 ? 1 : 0,
                           reinterpret_cast<u64*>(min1), reinterpret_cast<u64*>(cnt1), reinterpret_cast<u64*>(nroy1));
        if (need2) {
            int64_t nr = (wgs + ntiles - 1) / ntiles;
            nr = imin64(nr, (sg + 2047) / 2048);
            nr = nr < 1 ? 1 : (nr > 65535 ? 65535 : nr);
            const int64_t per_range = (sg + nr - 1) / nr;
            nr = (sg + per_range - 1) / per_range;
            hipLaunchKernelGGL(k_hm_pairs, dim3((unsigned)ntiles, (unsigned)nr), dim3(HM_THREADS), (size_t)TP * BB * 16, ctx->stream,
                               hw.codes, score + g0, cutoff, hw.pairs, npairs, d, B, TP, sg, per_range, reinterpret_cast<u64*>(min2),
                               reinterpret_cast<u64*>(cnt2), reinterpret_cast<u64*>(nroy2));
        }
    }
    if (need1) hipLaunchKernelGGL(k_hm_unkey, dim3(hm_blocks(n1)), dim3(HM_THREADS), 0, ctx->stream, min1, n1);
    if (need2) hipLaunchKernelGGL(k_hm_unkey, dim3(hm_blocks(n2)), dim3(HM_THREADS), 0, ctx->stream, min2, n2);
    GPB_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_hm_uniform(gpb_ctx* ctx, const double* lo_host, const double* hi_host, int64_t d, uint64_t row0, int64_t S,
                              uint64_t seed, double* X_dev, int64_t ld) {
    if (!ctx || !lo_host || !hi_host || !X_dev) return GPB_E_ARG;
    if (d < 1 || d > HM_MAX_D) GPB_FAIL(GPB_E_ARG, "gpb_hm_uniform: d outside 1 .. 512");
    if (S < 1 || S > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_hm_uniform: S outside 1 .. 2^31 - 1");
    if (ld < d) GPB_FAIL(GPB_E_ARG, "gpb_hm_uniform: ld < d");
    if ((S * d + HM_THREADS - 1) / HM_THREADS > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_hm_uniform: S d too large for one launch");
    for (int64_t j = 0; j < d; ++j)
        if (!isfinite(lo_host[j]) || !isfinite(hi_host[j]) || !(hi_host[j] > lo_host[j]))
            GPB_FAIL(GPB_E_ARG, "gpb_hm_uniform: bounds must be finite with hi > lo");
    GPB_HIP(hipSetDevice(ctx->device));
    return launch_hm_uniform(ctx, lo_host, hi_host, (int)d, row0, S, seed, X_dev, ld);
}

extern "C" int gpb_hm_implausibility(gpb_ctx* ctx, const double* mu_T, const double* var_T, int64_t M, int64_t S, int64_t ld,
                                     const double* yexp_dev, const double* vadd_dev, const int32_t* ranges_host, int G, int K,
                                     double* top_T, int32_t* arg, double* gmax_T, int64_t ldo, int64_t* bad_dev) {
    if (!ctx || !mu_T || !yexp_dev || !top_T || !bad_dev) return GPB_E_ARG;
    if (M < 1 || M > HM_MAX_M) GPB_FAIL(GPB_E_ARG, "gpb_hm_implausibility: M outside 1 .. 4096");
    if (K < 1 || K > HM_MAX_K || K > M) GPB_FAIL(GPB_E_ARG, "gpb_hm_implausibility: K outside 1 .. min(4, M)");
    if (S < 1 || S > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_hm_implausibility: S outside 1 .. 2^31 - 1");
    if (ld < S || ldo < S) GPB_FAIL(GPB_E_ARG, "gpb_hm_implausibility: ld or ldo below S");
    if (G < 0 || G > HM_MAX_G) GPB_FAIL(GPB_E_ARG, "gpb_hm_implausibility: G outside 0 .. 64");
    if (G > 0 && !ranges_host) GPB_FAIL(GPB_E_ARG, "gpb_hm_implausibility: G > 0 without ranges");
    HmRanges rg;
    int inline_groups = 1;
    for (int g = 0; g < G; ++g) {
        const int64_t m0 = ranges_host[2 * g], m1 = ranges_host[2 * g + 1];
        if (m0 < 0 || m1 > M || m0 >= m1) GPB_FAIL(GPB_E_ARG, "gpb_hm_implausibility: a range that is empty or not inside [0, M)");
        rg.m0[g] = (int)m0;
        rg.m1[g] = (int)m1;
        if (g > 0 && m0 < rg.m1[g - 1]) inline_groups = 0;
    }
    for (int g = G; g < HM_MAX_G; ++g) rg.m0[g] = rg.m1[g] = 0;
    GPB_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_hm_impl, dim3(hm_blocks(S)), dim3(HM_THREADS), 0, ctx->stream, mu_T, var_T, (int)M, S, ld, yexp_dev, vadd_dev, rg,
                       G, inline_groups, K, top_T, arg, gmax_T, ldo, reinterpret_cast<u64*>(bad_dev));
    GPB_HIP(hipGetLastError());
    return 0;
}

extern "C" int gpb_hm_maps(gpb_ctx* ctx, const double* x_dev, int64_t S, int64_t d, int64_t row_stride, const double* score_dev,
                           double cutoff, const double* edges_host, int B, const int32_t* pairs_host, int64_t npairs, int init,
                           double* min1, int64_t* cnt1, int64_t* nroy1, double* min2, int64_t* cnt2, int64_t* nroy2) {
    if (!ctx || !x_dev || !score_dev || !edges_host) return GPB_E_ARG;
    if (S < 1 || d < 1) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: need S >= 1 and d >= 1");
    if (S > 0x7fffffffLL || d > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: more than 2^31 - 1 samples or parameters");
    if (B < 1 || B > HM_MAX_B) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: B outside 1 .. 64");
    if (row_stride < d) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: row_stride below d");
    if (!isfinite(cutoff)) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: cutoff must be finite");
    if (init != 0 && init != 1) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: init must be 0 or 1");
    if ((min1 != nullptr) != (cnt1 != nullptr) || (min1 != nullptr) != (nroy1 != nullptr) || (min2 != nullptr) != (cnt2 != nullptr) ||
        (min2 != nullptr) != (nroy2 != nullptr))
        GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: the outputs come in triples (min, cnt, nroy), whole or NULL");
    for (int64_t j = 0; j < d; ++j) {
        const double* e = edges_host + j * (B + 1);
        for (int b = 0; b <= B; ++b)
            if (!isfinite(e[b]) || (b > 0 && !(e[b] > e[b - 1]))) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: edges must be finite and strictly increasing");
    }
    if (npairs < 0) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: npairs < 0");
    if ((__int128)npairs * B * B > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: npairs B^2 above 2^31 - 1");
    if (pairs_host) {
        for (int64_t p = 0; p < npairs; ++p) {
            const int64_t i = pairs_host[2 * p], j = pairs_host[2 * p + 1];
            if (i < 0 || i >= d || j < 0 || j >= d) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: a pair index outside [0, d)");
            if (i == j) GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: a pair (i, i)");
        }
    } else if (min2 && npairs != d * (d - 1) / 2) {
        GPB_FAIL(GPB_E_ARG, "gpb_hm_maps: without a pair list npairs must be d (d - 1) / 2");
    }
    if (!min1 && !(min2 && npairs > 0)) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    return launch_hm_maps(ctx, x_dev, S, d, row_stride, score_dev, cutoff, edges_host, B, pairs_host, npairs, init, min1, cnt1, nroy1, min2,
                          cnt2, nroy2);
}
