// gpb_psis.hip — Pareto-smoothed importance sampling over the sample axis of [R][ld] arrays of log ratios, and the PSIS-LOO / WAIC
// reductions of [R][ld] arrays of pointwise log-likelihoods (Vehtari, Simpson, Gelman, Yao, Gabry, JMLR 2024; Vehtari, Gelman,
// Gabry, Stat. Comput. 2017), step for step what ArviZ's _psislw / _gpdfit / _gpinv compute.  Per row, S finite log ratios lr:
//   1 shift      x = lr - max(lr); the maximum is exact and order free.
//   2 cutoff     M = min(S // 5, ceil(3 sqrt(S))); cutoff = max((M + 1)-th largest x, ln DBL_MIN); the tail is {x > cutoff}, n_tail
//                its size (<= M; smaller when values tie with the cutoff).  The order statistic comes from an exact radix select on
//                the order-preserving key of order_key.h: six passes over the row, eleven bits each (nine in the last).
//   3 short tail n_tail <= 4: khat = +inf, nothing is smoothed.
//   4 fit        the tail is sorted ascending, ties by sample index: every tail value's rank is counted against tiles of the tail
//                staged in LDS, and t_j = exp(x_j) - exp(cutoff) is written at its rank into LDS.  psis_fit.h has the fit: the
//                candidates are shared out over the waves, a wave's lanes stride over the tail and fold by __shfl_down.
//   5 replace    the j-th smallest tail value (j = 1 .. n_tail) becomes ln(sigma expm1(-khat log1p(-p_j)) / khat + exp(cutoff)),
//                p_j = (j - 1/2) / n_tail (-sigma log1p(-p_j) in place of the fraction at khat == 0); a non-finite khat smooths nothing.
//   6 truncate and normalise   values above 0 become 0; lw = x - ln sum exp(x); ess = (sum exp x)^2 / sum exp(2 x) = 1 / sum exp(2 lw).
// gpb_psis_loo takes ll, runs the same steps on lr = -ll and reduces in the same passes: elpd_loo = ln sum exp(lw + ll),
// lppd = ln sum exp(ll) - ln S, p_waic = sum (ll - mean ll)^2 / (S - 1) (the mean from the first pass), loo_pit = sum exp(lw)
// Phi(zc) with Phi(z) = erfc(-z / sqrt 2) / 2, min ll.
// One workgroup of PSIS_THREADS threads per row and ONE kernel: the row is read nine times (maximum; six select passes; the
// gather of the tail; the sums) and a tenth time when lw is written.  Sums over the samples: thread t adds s = t, t + PSIS_THREADS,
// ... in ascending order, a wave folds its 64 threads by __shfl_down, thread 0 adds the sixteen wave sums in order; the smoothed tail
// is summed the same way over its ranks and added to the body's sum.  Every tree is fixed by S and n_tail alone, there is no
// floating-point atomic (the histogram and the gather count with integer atomics in LDS, and what they count does not depend
// on the order), and a row's bits depend on nothing but the row.
#include "gpb_internal.h"
#include "order_key.h"
#include "psis_fit.h"
#include <float.h>
#include <math.h>

// Nothing in this file may be contracted (build.py compiles it with -ffp-contract=off): psis_fit.h's host check runs the same
// operations in the same order.

namespace gpb {

namespace {

constexpr int PSIS_THREADS = 1024;
constexpr int PSIS_WAVES = PSIS_THREADS / 64;
constexpr int PSIS_BINS = 2048;                  // eleven bits per select pass
constexpr int PSIS_PASSES = 6;
constexpr int PSIS_NSUM = 8;                     // sums one reduction carries
static_assert(PSIS_BINS == 2 * PSIS_THREADS, "the suffix scan gives every thread two bins");
static_assert(GPB_PSIS_LANES == 64, "psis_fit.h folds a wave");

struct PsisShared {
    unsigned hist[PSIS_BINS];
    unsigned scan[2][PSIS_THREADS];
    double red[PSIS_NSUM][PSIS_WAVES];
    double tile_x[PSIS_THREADS];
    unsigned tile_i[PSIS_THREADS];
    double cand_b[GPB_PSIS_MAX_CAND + 4], cand_L[GPB_PSIS_MAX_CAND + 4], cand_w[GPB_PSIS_MAX_CAND + 4];
    double bc[PSIS_NSUM];                        // broadcast slots
    unsigned long long prefix;
    unsigned kth, count;
};

__device__ __forceinline__ double wave_fold(double v) {
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// sums[0 .. K) of every thread -> the block's sums in sh.bc[0 .. K) (all threads may read them after the call)
template <int K>
__device__ __forceinline__ void block_sums(PsisShared& sh, const double (&v)[K]) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    __syncthreads();
    for (int q = 0; q < K; ++q) {
        const double f = wave_fold(v[q]);
        if (lane == 0) sh.red[q][wv] = f;
    }
    __syncthreads();
    if (t < K) {
        double a = sh.red[t][0];
        for (int i = 1; i < PSIS_WAVES; ++i) a = a + sh.red[t][i];
        sh.bc[t] = a;
    }
    __syncthreads();
}
template <int K>
__device__ __forceinline__ void block_maxes(PsisShared& sh, const double (&v)[K]) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    __syncthreads();
    for (int q = 0; q < K; ++q) {
        const double f = wave_max(v[q]);
        if (lane == 0) sh.red[q][wv] = f;
    }
    __syncthreads();
    if (t < K) {
        double a = sh.red[t][0];
        for (int i = 1; i < PSIS_WAVES; ++i) a = sh.red[t][i] > a ? sh.red[t][i] : a;
        sh.bc[t] = a;
    }
    __syncthreads();
}

__device__ __forceinline__ double norm_cdf(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

// out columns of gpb_psis_loo: GPB_LOO_* of include/gpbayes.h
// LOO: in = ll, lr = -ll.  tails: this row's n_cap doubles of LDS follow the PsisShared block.  gx / gi / gs / gr: the row's
// slices of the workspace — the gathered tail's x and sample index, the sample index by rank, the rank by gathered position.
template <bool LOO>
__global__ __launch_bounds__(PSIS_THREADS) void k_psis_row(const double* __restrict__ in_T, const double* __restrict__ zc_T, int64_t S,
                                                           int64_t ld, int64_t n_cap, double cutmin, double* __restrict__ khat_out,
                                                           int64_t* __restrict__ ntail_out, double* __restrict__ ess_out,
                                                           double* __restrict__ lw_T, double* __restrict__ loo_out,
                                                           double* __restrict__ gx_all, unsigned* __restrict__ gi_all,
                                                           unsigned* __restrict__ gs_all, unsigned* __restrict__ gr_all) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PsisShared& sh = *reinterpret_cast<PsisShared*>(smem);
    double* ts = reinterpret_cast<double*>(smem + sizeof(PsisShared));
    const int64_t r = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const double* in = in_T + r * ld;
    const double* zc = (LOO && zc_T) ? zc_T + r * ld : nullptr;
    double* gx = gx_all + r * n_cap;
    unsigned* gi = gi_all + r * n_cap;
    unsigned* gs = gs_all + r * n_cap;
    unsigned* gr = gr_all + r * n_cap;

    // ---- 1: the maximum of lr (LOO: and the maximum and the sum of ll)
    double mx, ll_max = 0.0, ll_mean = 0.0;
    {
        double m[2] = {-INFINITY, -INFINITY}, a[1] = {0.0};
        for (int64_t s = t; s < S; s += PSIS_THREADS) {
            const double v = in[s];
            const double lr = LOO ? -v : v;
            m[0] = lr > m[0] ? lr : m[0];
            if (LOO) {
                m[1] = v > m[1] ? v : m[1];
                a[0] = a[0] + v;
            }
        }
        block_maxes<2>(sh, m);
        mx = sh.bc[0];
        ll_max = sh.bc[1];
        if (LOO) {
            block_sums<1>(sh, a);
            ll_mean = sh.bc[0] / (double)S;
        }
    }
    // ---- 2: the (M + 1)-th largest x by radix select, most significant digit first
    const int64_t Mt = psis_tail_max(S);
    if (t == 0) {
        sh.prefix = 0ull;
        sh.kth = (unsigned)(Mt + 1);
        sh.count = 0u;
    }
    for (int p = 0; p < PSIS_PASSES; ++p) {
        const int shift = p < 5 ? 53 - 11 * p : 0;            // the digit's lowest bit
        const unsigned mask = p < 5 ? 0x7ffu : 0x1ffu;
        const int above = p < 5 ? shift + 11 : 9;            // bits below the prefix found so far
        sh.hist[t] = 0u;
        sh.hist[t + PSIS_THREADS] = 0u;
        __syncthreads();
        const unsigned long long pre = sh.prefix;
        for (int64_t s0 = 0; s0 < S; s0 += PSIS_THREADS) {       // (uniform trip count: the ballots below need whole waves)
            const int64_t s = s0 + t;
            bool act = s < S;
            unsigned d = 0u;
            if (act) {
                const double v = in[s];
                const unsigned long long key = ppd_key(__dsub_rn(LOO ? -v : v, mx));
                act = p == 0 || (key >> above) == pre;
                d = (unsigned)(key >> shift) & mask;
            }
            // lanes of a wave mostly share their leading digits: the lanes that agree with the first active one add once
            const unsigned long long am = __ballot(act);
            if (am) {
                const int leader = __ffsll((long long)am) - 1;
                const unsigned dl = (unsigned)__shfl((int)d, leader);
                const unsigned long long same = __ballot(act && d == dl);
                if (act) {
                    if (d == dl) {
                        if (lane == leader) atomicAdd(&sh.hist[dl], (unsigned)__popcll(same));
                    } else {
                        atomicAdd(&sh.hist[d], 1u);
                    }
                }
            }
        }
        __syncthreads();
        // suffix sums over pairs of bins: scan[t] = entries in bins >= 2 t
        const unsigned h0 = sh.hist[2 * t], h1 = sh.hist[2 * t + 1];
        int cur = 0;
        sh.scan[0][t] = h0 + h1;
        __syncthreads();
        for (int off = 1; off < PSIS_THREADS; off <<= 1) {
            const unsigned v = sh.scan[cur][t] + (t + off < PSIS_THREADS ? sh.scan[cur][t + off] : 0u);
            sh.scan[cur ^ 1][t] = v;
            cur ^= 1;
            __syncthreads();
        }
        const unsigned k = sh.kth;
        const unsigned mine = sh.scan[cur][t], higher = t + 1 < PSIS_THREADS ? sh.scan[cur][t + 1] : 0u;
        __syncthreads();
        if (mine >= k && higher < k) {                       // exactly one thread: the k-th largest lies in one of its two bins
            unsigned dsel, knew;
            if (higher + h1 >= k) {
                dsel = 2u * t + 1u;
                knew = k - higher;
            } else {
                dsel = 2u * t;
                knew = k - higher - h1;
            }
            sh.prefix = p < 5 ? ((pre << 11) | dsel) : ((pre << 9) | dsel);
            sh.kth = knew;
        }
        __syncthreads();
    }
    const double xk = ppd_unkey(sh.prefix);
    const double cutoff = xk > cutmin ? xk : cutmin;
    const double ecut = exp(cutoff);
    // ---- the tail, gathered in whatever order the threads arrive (its sort does not depend on it)
    for (int64_t s = t; s < S; s += PSIS_THREADS) {
        const double v = in[s];
        const double x = __dsub_rn(LOO ? -v : v, mx);
        if (x > cutoff) {
            const unsigned pos = atomicAdd(&sh.count, 1u);
            if (pos < (unsigned)n_cap) {                     // (n_tail <= M <= n_cap always; the store stays inside the row's slice)
                gx[pos] = x;
                gi[pos] = (unsigned)s;
            }
        }
    }
    __syncthreads();
    const int n = (int)(sh.count < (unsigned)n_cap ? sh.count : (unsigned)n_cap);
    // ---- 3, 4: ranks, the sorted excesses, the fit
    double khat = INFINITY, sigma = NAN;
    if (n >= GPB_PSIS_MIN_TAIL) {
        for (int e0 = 0; e0 < n; e0 += PSIS_THREADS) {
            const int e = e0 + t;
            const double xe = e < n ? gx[e] : 0.0;
            const unsigned ie = e < n ? gi[e] : 0u;
            unsigned rank = 0u;
            for (int b0 = 0; b0 < n; b0 += PSIS_THREADS) {
                __syncthreads();
                if (b0 + t < n) {
                    sh.tile_x[t] = gx[b0 + t];
                    sh.tile_i[t] = gi[b0 + t];
                }
                __syncthreads();
                const int cnt = n - b0 < PSIS_THREADS ? n - b0 : PSIS_THREADS;
                for (int j = 0; j < cnt; ++j) {
                    const double xj = sh.tile_x[j];
                    rank += (xj < xe || (xj == xe && sh.tile_i[j] < ie)) ? 1u : 0u;
                }
            }
            if (e < n) {
                ts[rank] = __dsub_rn(exp(xe), ecut);
                gs[rank] = ie;
                gr[e] = rank;
            }
        }
        __syncthreads();
        const int m = psis_m_est(n);
        const double tq = ts[psis_quartile_index(n)], tl = ts[n - 1];
        for (int i = wv; i < m; i += PSIS_WAVES) {
            const double b = psis_candidate(i + 1, m, tq, tl);
            const double f = wave_fold(psis_lane_sum(ts, n, b, lane));
            if (lane == 0) {
                sh.cand_b[i] = b;
                sh.cand_L[i] = psis_profile(n, b, f / (double)n);
            }
        }
        __syncthreads();
        if (t < m) sh.cand_w[t] = psis_weight(sh.cand_L, m, t);
        __syncthreads();
        if (t == 0) sh.bc[0] = psis_bhat(sh.cand_b, sh.cand_w, m);
        __syncthreads();
        const double bh = sh.bc[0];
        if (wv == 0) {
            const double f = wave_fold(psis_lane_sum(ts, n, bh, lane));
            if (lane == 0) {
                double kh, sg;
                psis_finish(n, bh, f, &kh, &sg);
                sh.bc[1] = kh;
                sh.bc[2] = sg;
            }
        }
        __syncthreads();
        khat = sh.bc[1];
        sigma = sh.bc[2];
        __syncthreads();
    }
    // ---- 5: the smoothed values at their ranks, truncated at 0
    const bool smoothed = n >= GPB_PSIS_MIN_TAIL && khat - khat == 0.0;
    if (smoothed) {
        for (int j = t; j < n; j += PSIS_THREADS) {
            const double v = psis_smoothed(j, n, khat, sigma, ecut);
            ts[j] = v > 0.0 ? 0.0 : v;
        }
    }
    __syncthreads();
    const double bodycut = smoothed ? cutoff : INFINITY;
    // ---- 6: the sums.  [0] sum e  [1] sum e e  [2] sum exp(x + ll - c)  [3] sum e Phi(zc)  [4] sum exp(ll - max)  [5] sum dev^2
    double c_shift = 0.0;
    if (LOO) {
        double m[1] = {-mx};                                 // min ll: what x + ll is for every sample that keeps its weight
        if (smoothed)
            for (int j = t; j < n; j += PSIS_THREADS) {
                const double v = ts[j] + in[gs[j]];
                m[0] = v > m[0] ? v : m[0];
            }
        block_maxes<1>(sh, m);
        c_shift = sh.bc[0];
    }
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t s = t; s < S; s += PSIS_THREADS) {
        const double v = in[s];
        const double x = __dsub_rn(LOO ? -v : v, mx);
        if (x <= bodycut) {
            const double e = exp(x);
            acc[0] = acc[0] + e;
            acc[1] = acc[1] + e * e;
            if (LOO) {
                acc[2] = acc[2] + exp((x + v) - c_shift);
                if (zc) acc[3] = acc[3] + e * norm_cdf(zc[s]);
            }
        }
        if (LOO) {
            acc[4] = acc[4] + exp(v - ll_max);
            const double dv = v - ll_mean;
            acc[5] = acc[5] + dv * dv;
        }
    }
    block_sums<6>(sh, acc);
    double body[6];
    for (int q = 0; q < 6; ++q) body[q] = sh.bc[q];
    double tl4[4] = {0.0, 0.0, 0.0, 0.0};
    if (smoothed) {
        for (int j = t; j < n; j += PSIS_THREADS) {
            const double x = ts[j];
            const double e = exp(x);
            tl4[0] = tl4[0] + e;
            tl4[1] = tl4[1] + e * e;
            if (LOO) {
                const unsigned s = gs[j];
                tl4[2] = tl4[2] + exp((x + in[s]) - c_shift);
                if (zc) tl4[3] = tl4[3] + e * norm_cdf(zc[s]);
            }
        }
    }
    block_sums<4>(sh, tl4);
    const double s1 = body[0] + sh.bc[0], s2 = body[1] + sh.bc[1], s3 = body[2] + sh.bc[2], s4 = body[3] + sh.bc[3];
    const double lse = log(s1);
    const double ess = s1 * s1 / s2;
    if (t == 0) {
        if (khat_out) khat_out[r] = khat;
        if (ntail_out) ntail_out[r] = n;
        if (ess_out) ess_out[r] = ess;
        if (LOO) {
            double* o = loo_out + r * GPB_LOO_NOUT;
            o[GPB_LOO_ELPD] = (log(s3) + c_shift) - lse;
            o[GPB_LOO_LPPD] = (log(body[4]) + ll_max) - log((double)S);
            o[GPB_LOO_PWAIC] = S > 1 ? body[5] / (double)(S - 1) : NAN;
            o[GPB_LOO_KHAT] = khat;
            o[GPB_LOO_ESS] = ess;
            o[GPB_LOO_NTAIL] = (double)n;
            o[GPB_LOO_PIT] = zc ? s4 / s1 : NAN;
            o[GPB_LOO_MINLL] = -mx;
        }
    }
    // ---- lw: the body by sample, then the tail by rank (disjoint entries)
    if (lw_T) {
        double* lw = lw_T + r * ld;
        for (int64_t s = t; s < S; s += PSIS_THREADS) {
            const double v = in[s];
            const double x = __dsub_rn(LOO ? -v : v, mx);
            if (x <= bodycut) lw[s] = x - lse;
        }
        if (smoothed)
            for (int j = t; j < n; j += PSIS_THREADS) lw[gs[j]] = ts[j] - lse;
    }
}

template <bool LOO>
int launch_psis(gpb_ctx* ctx, const char* who, const double* in_T, const double* zc_T, int64_t R, int64_t S, int64_t ld, int on_device,
                double* khat, int64_t* n_tail, double* ess, double* lw_T, double* out) {
    if (R < 1 || R > 0x7fffffffLL || S < 1 || ld < S) GPB_FAIL(GPB_E_ARG, std::string(who) + ": need 1 <= R <= 2^31 - 1, S >= 1 and ld >= S");
    if (S > GPB_PSIS_MAX_S) GPB_FAIL(GPB_E_ARG, std::string(who) + ": S above 2^24 (the tail of a row must fit in LDS)");
    GPB_HIP(hipSetDevice(ctx->device));
    const int64_t Mt = psis_tail_max(S), n_cap = Mt > 1 ? Mt : 1;
    const bool host = !on_device;
    double *gx, *d_in = nullptr, *d_zc = nullptr, *d_lw = nullptr, *d_khat = nullptr, *d_ess = nullptr, *d_out = nullptr;
    int64_t* d_nt = nullptr;
    unsigned *gi, *gs, *gr;
    if (const int rc = ctx_carve(ctx, ctx->loo_ws, [&](Carver<double>& c) {
            gx = c.take<double>(R * n_cap);
            gi = c.take<unsigned>(R * n_cap);
            gs = c.take<unsigned>(R * n_cap);
            gr = c.take<unsigned>(R * n_cap);
            if (host) {
                d_in = c.take<double>(R * ld);
                d_zc = zc_T ? c.take<double>(R * ld) : nullptr;
                d_lw = lw_T ? c.take<double>(R * ld) : nullptr;
                d_khat = khat ? c.take<double>(R) : nullptr;
                d_ess = ess ? c.take<double>(R) : nullptr;
                d_nt = n_tail ? c.take<int64_t>(R) : nullptr;
                d_out = out ? c.take<double>(R * GPB_LOO_NOUT) : nullptr;
            }
        }))
        return rc;
    if (host) {
        GPB_HIP(hipMemcpyAsync(d_in, in_T, sizeof(double) * (size_t)(R * ld), hipMemcpyHostToDevice, ctx->stream));
        if (zc_T) GPB_HIP(hipMemcpyAsync(d_zc, zc_T, sizeof(double) * (size_t)(R * ld), hipMemcpyHostToDevice, ctx->stream));
    } else {
        d_in = const_cast<double*>(in_T);
        d_zc = const_cast<double*>(zc_T);
        d_lw = lw_T;
        d_khat = khat;
        d_ess = ess;
        d_nt = n_tail;
        d_out = out;
    }
    const size_t lds = sizeof(PsisShared) + sizeof(double) * (size_t)n_cap;
    if (lds > 64 * 1024)
        GPB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_psis_row<LOO>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_psis_row<LOO>, dim3((unsigned)R), dim3(PSIS_THREADS), lds, ctx->stream, d_in, d_zc, S, ld, n_cap, log(DBL_MIN),
                       d_khat, d_nt, d_ess, d_lw, d_out, gx, gi, gs, gr);
    GPB_HIP(hipGetLastError());
    if (host) {
        const auto back = [&](void* dst, const void* src, size_t bytes) {
            return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
        };
        GPB_HIP(back(lw_T, d_lw, sizeof(double) * (size_t)(R * ld)));
        GPB_HIP(back(khat, d_khat, sizeof(double) * (size_t)R));
        GPB_HIP(back(ess, d_ess, sizeof(double) * (size_t)R));
        GPB_HIP(back(n_tail, d_nt, sizeof(int64_t) * (size_t)R));
        GPB_HIP(back(out, d_out, sizeof(double) * (size_t)(R * GPB_LOO_NOUT)));
        GPB_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

}  // namespace

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_psis(gpb_ctx* ctx, const double* lr_T, int64_t R, int64_t S, int64_t ld, int on_device, double* khat, int64_t* n_tail,
                        double* ess, double* lw_T) {
    if (!ctx || !lr_T) return GPB_E_ARG;
    return launch_psis<false>(ctx, "gpb_psis", lr_T, nullptr, R, S, ld, on_device, khat, n_tail, ess, lw_T, nullptr);
}

extern "C" int gpb_psis_loo(gpb_ctx* ctx, const double* ll_T, const double* zc_T, int64_t R, int64_t S, int64_t ld, int on_device,
                            double* out) {
    if (!ctx || !ll_T || !out) return GPB_E_ARG;
    return launch_psis<true>(ctx, "gpb_psis_loo", ll_T, zc_T, R, S, ld, on_device, nullptr, nullptr, nullptr, nullptr, out);
}
