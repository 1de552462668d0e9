// gpb_rank.hip — rank-normalised split-R-hat (bulk and folded) and bulk / tail / mean / quantile effective sample sizes of a
// resident chain (gpb_chain_rank_diag; Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021), per parameter, of a chain that lies in
// HBM as gpb_mcmc_diag reads it.  The statistic is specified in include/gpbayes.h; DESIGN.md section 32 has the reasons.
// One parameter at a time, the global rank transform — a device LSD radix sort of (order-preserving 64-bit key, 32-bit position):
//   k_rank_gather    the kept draws through the strides -> keys ppd_key(x + 0.0) (folded: of |x - med|) and positions; the OR of
//                    key ^ first key over all draws, one integer atomic per wave: a byte of it that is zero is a digit all keys share
//   k_rsort_plan     one lane: which of the eight passes are skipped and which buffer each of the others reads
//   k_rsort_count    per sort block of 4096 keys: the digit histogram in LDS (integer atomics)
//   k_rsort_offsets  one workgroup, lane = digit: exclusive scan over the blocks, then over the digits
//   k_rsort_scatter  per sort block, 16 rounds of 256 keys in order: the rank of a key among the equal digits of its wave from
//                    eight wave-64 ballots, the waves and rounds in order from LDS counters — every pass is stable, as LSD needs
//   k_rank_runs      per sorted position: the run of equal keys around it (neighbours, else two binary searches) -> 2 r = first +
//                    last + 1 (1-based), written at the draw's position
//   k_rank_order     the median and the quantile levels from the sorted keys, numpy's arithmetic
// then its series, split chains (first and second half of every walker) as the columns:
//   k_rank_pack      one lane per (series, split chain): z = ndtri((r - 3/8) / (n + 1/4)), x, the indicators x <= q_p, and z of the
//                    folded ranks: compensated two-pass mean and variance; the centred series into Y (not for the folded one)
// and for a group of parameters at once:
//   k_rank_stats     one workgroup per series: W, the variance of the chain means, R-hat of the bulk and the folded series
//   k_diag_gram      diag_gram.h: the band of Y Y^T per series, its diagonal sums
//   k_rank_lags      one lane per lag: A(t) = the block partials in block-row order / (m h), k_diag_lags' order: the same bits
//                    for every band that holds the lag
//   k_rank_geyer     one lane per series: Stan's rho-hat, Geyer's initial positive and initial monotone sequence, tau, ESS
// No floating-point atomics, every sum in one fixed order; built with -ffp-contract=off: numpy's interpolation bit for bit.
#include "gpb_internal.h"
#include "diag_gram.h"
#include "block_reduce.h"
#include "ndtri.h"
#include "order_key.h"
#include <math.h>

namespace gpb {

namespace {

constexpr int RANK_THREADS = REDUCE_THREADS;
constexpr int SORT_THREADS = 256;
constexpr int SORT_WAVES = SORT_THREADS / 64;
constexpr int SORT_ROUNDS = 16;
constexpr int SORT_TILE = SORT_THREADS * SORT_ROUNDS;          // keys per sort block
constexpr int PLAN_SKIP = 8, PLAN_SRC = 16;                     // offsets in the plan (RankWs)

struct RankLevels {
    long long lo[GPB_RANK_MAX_Q], hi[GPB_RANK_MAX_Q];           // the two order statistics of level k
    double g[GPB_RANK_MAX_Q];                                    // the fractional part of p (n - 1)
    int nq;
};

// kept draw i = tk * nw + w (tk < 2 h: kept step, the second half starts at step nsteps - h) of parameter j
__device__ __forceinline__ double kept_value(const double* __restrict__ x, int64_t i, int64_t nw, int64_t h, int64_t nsteps,
                                             int64_t ss, int64_t ws, int64_t j) {
    const int64_t tk = i / nw, w = i % nw;
    const int64_t t = tk < h ? tk : tk + (nsteps - 2 * h);
    return x[t * ss + w * ws + j] + 0.0;                         // (-0.0 + 0.0 = +0.0)
}

// ---------------------------------------------------------------------------------------------------------------- gather
// med: nullptr for the values themselves, else the keys are those of |x - *med|
__global__ __launch_bounds__(SORT_THREADS) void k_rank_gather(const double* __restrict__ x, int64_t n, int64_t nw, int64_t h,
                                                              int64_t nsteps, int64_t ss, int64_t ws, int64_t j,
                                                              const double* __restrict__ med, uint64_t* __restrict__ keys,
                                                              unsigned* __restrict__ pos, unsigned* __restrict__ plan) {
    const int64_t i = (int64_t)blockIdx.x * SORT_THREADS + threadIdx.x;
    const double m = med ? *med : 0.0;
    double v0 = kept_value(x, 0, nw, h, nsteps, ss, ws, j);
    if (med) v0 = fabs(v0 - m);
    const uint64_t k0 = ppd_key(v0);
    uint64_t diff = 0;
    if (i < n) {
        double v = kept_value(x, i, nw, h, nsteps, ss, ws, j);
        if (med) v = fabs(v - m);
        const uint64_t k = ppd_key(v);
        keys[i] = k;
        pos[i] = (unsigned)i;
        diff = k ^ k0;
    }
    for (int o = 32; o >= 1; o >>= 1) diff |= (uint64_t)__shfl_xor((unsigned long long)diff, o, 64);
    if ((threadIdx.x & 63) == 0 && diff) atomicOr(reinterpret_cast<unsigned long long*>(plan), (unsigned long long)diff);
}

__global__ void k_rsort_plan(unsigned* __restrict__ plan) {
    if (threadIdx.x || blockIdx.x) return;
    const uint64_t diff = *reinterpret_cast<const unsigned long long*>(plan);
    unsigned src = 0;
    for (int p = 0; p < 8; ++p) {
        const unsigned skip = ((diff >> (8 * p)) & 255u) == 0u;
        plan[PLAN_SKIP + p] = skip;
        plan[PLAN_SRC + p] = src;
        src ^= skip ? 0u : 1u;
    }
    plan[PLAN_SRC + 8] = src;                                   // where the sorted keys lie
}

// ---------------------------------------------------------------------------------------------------------------- one pass
__global__ __launch_bounds__(SORT_THREADS) void k_rsort_count(const uint64_t* __restrict__ k0, const uint64_t* __restrict__ k1,
                                                              int64_t n, int pass, const unsigned* __restrict__ plan,
                                                              unsigned* __restrict__ counts) {
    if (plan[PLAN_SKIP + pass]) return;
    __shared__ unsigned hist[256];
    const uint64_t* src = plan[PLAN_SRC + pass] ? k1 : k0;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * SORT_TILE;
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const int64_t i = i0 + r * SORT_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&hist[(unsigned)(src[i] >> (8 * pass)) & 255u], 1u);
    }
    __syncthreads();
    counts[(int64_t)blockIdx.x * 256 + threadIdx.x] = hist[threadIdx.x];
}

// counts[b][digit] -> the digit's keys in the blocks in front of b; base[digit] -> the keys of smaller digits
__global__ __launch_bounds__(256) void k_rsort_offsets(int64_t nsb, int pass, const unsigned* __restrict__ plan,
                                                       unsigned* __restrict__ counts, unsigned* __restrict__ base) {
    if (plan[PLAN_SKIP + pass]) return;
    __shared__ unsigned tot[256];
    const int t = threadIdx.x;
    unsigned run = 0;
    for (int64_t b = 0; b < nsb; ++b) {
        const unsigned c = counts[b * 256 + t];
        counts[b * 256 + t] = run;
        run += c;
    }
    tot[t] = run;
    __syncthreads();
    if (t == 0) {
        unsigned s = 0;
        for (int dgt = 0; dgt < 256; ++dgt) {
            const unsigned c = tot[dgt];
            tot[dgt] = s;
            s += c;
        }
    }
    __syncthreads();
    base[t] = tot[t];
}

__global__ __launch_bounds__(SORT_THREADS) void k_rsort_scatter(uint64_t* __restrict__ k0, uint64_t* __restrict__ k1,
                                                                unsigned* __restrict__ p0, unsigned* __restrict__ p1, int64_t n,
                                                                int pass, const unsigned* __restrict__ plan,
                                                                const unsigned* __restrict__ counts,
                                                                const unsigned* __restrict__ base) {
    if (plan[PLAN_SKIP + pass]) return;
    __shared__ unsigned run[256];
    __shared__ unsigned wcnt[SORT_WAVES][256];
    const bool from1 = plan[PLAN_SRC + pass] != 0;
    const uint64_t* sk = from1 ? k1 : k0;
    const unsigned* sp = from1 ? p1 : p0;
    uint64_t* dk = from1 ? k0 : k1;
    unsigned* dp = from1 ? p0 : p1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    run[tid] = base[tid] + counts[(int64_t)blockIdx.x * 256 + tid];
    for (int w = 0; w < SORT_WAVES; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * SORT_TILE;
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const int64_t i = i0 + r * SORT_THREADS + tid;
        if (i0 + r * SORT_THREADS >= n) break;                  // (uniform)
        const bool valid = i < n;
        const uint64_t key = valid ? sk[i] : 0;
        const unsigned ps = valid ? sp[i] : 0;
        const unsigned dgt = (unsigned)(key >> (8 * pass)) & 255u;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (dgt >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const unsigned below = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && below == 0) wcnt[wave][dgt] = (unsigned)__popcll(same);
        __syncthreads();
        if (valid) {
            unsigned off = run[dgt] + below;
            for (int w = 0; w < wave; ++w) off += wcnt[w][dgt];
            dk[off] = key;
            dp[off] = ps;
        }
        __syncthreads();
        unsigned s = 0;
        for (int w = 0; w < SORT_WAVES; ++w) {
            s += wcnt[w][tid];
            wcnt[w][tid] = 0;
        }
        run[tid] += s;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- ranks
__global__ __launch_bounds__(RANK_THREADS) void k_rank_runs(const uint64_t* __restrict__ k0, const uint64_t* __restrict__ k1,
                                                            const unsigned* __restrict__ p0, const unsigned* __restrict__ p1,
                                                            int64_t n, const unsigned* __restrict__ plan, unsigned* __restrict__ r2) {
    const int64_t s = (int64_t)blockIdx.x * RANK_THREADS + threadIdx.x;
    if (s >= n) return;
    const bool in1 = plan[PLAN_SRC + 8] != 0;
    const uint64_t* S = in1 ? k1 : k0;
    const unsigned* P = in1 ? p1 : p0;
    const uint64_t key = S[s];
    int64_t a = s, b = s + 1;                                   // the run is [a, b)
    if (s > 0 && S[s - 1] == key) {
        int64_t lo = 0, hi = s - 1;                             // the first index with S == key lies in [lo, hi]
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (S[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        a = lo;
    }
    if (s + 1 < n && S[s + 1] == key) {
        int64_t lo = s + 2, hi = n;                             // the first index with S > key lies in [lo, hi]
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (S[mid] > key) hi = mid;
            else lo = mid + 1;
        }
        b = lo;
    }
    r2[P[s]] = (unsigned)(a + b + 1);                           // 2 x the mean of the 1-based positions a + 1 ... b
}

__global__ void k_rank_order(const uint64_t* __restrict__ k0, const uint64_t* __restrict__ k1, int64_t n,
                             const unsigned* __restrict__ plan, RankLevels lv, double* __restrict__ med, double* __restrict__ quant) {
    const int k = threadIdx.x;
    if (blockIdx.x || k > lv.nq) return;
    const uint64_t* S = plan[PLAN_SRC + 8] ? k1 : k0;
    if (k == lv.nq) {
        *med = (ppd_unkey(S[n / 2 - 1]) + ppd_unkey(S[n / 2])) / 2.0;         // (n = 2 h nwalkers is even)
        return;
    }
    const double lo = ppd_unkey(S[lv.lo[k]]), hi = ppd_unkey(S[lv.hi[k]]), g = lv.g[k];
    const double diff = hi - lo;
    quant[k] = g >= 0.5 ? hi - diff * (1.0 - g) : lo + diff * g;
}

__global__ __launch_bounds__(RANK_THREADS) void k_rank_widen(const unsigned* __restrict__ r2, int64_t n, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * RANK_THREADS + threadIdx.x;
    if (i < n) out[i] = (int64_t)r2[i];
}

// ---------------------------------------------------------------------------------------------------------------- pack
// blockIdx.y = series s: 0 z | 1 x | 2 + k the indicator of level k | K z of the folded ranks (no Y).  lane = split chain c.
template <int MODE>      // 0: z of ranks, 1: x, 2: indicator
__device__ __forceinline__ double series_value(const double* __restrict__ x, const unsigned* __restrict__ r2, int64_t i, int64_t t,
                                               int64_t w, int64_t ss, int64_t ws, int64_t j, double qn, double q) {
    if (MODE == 0) return ndtri(((double)r2[i] * 0.5 - 0.375) / qn);
    const double v = x[t * ss + w * ws + j] + 0.0;
    if (MODE == 1) return v;
    return v <= q ? 1.0 : 0.0;
}

template <int MODE>
__device__ __forceinline__ void pack_chain(const double* __restrict__ x, const unsigned* __restrict__ r2, int64_t nw, int64_t h,
                                           int64_t nsteps, int64_t ss, int64_t ws, int64_t j, int64_t c, double q, double* y,
                                           int64_t mp, int64_t hp, double* __restrict__ st) {
    const int64_t half = c >= nw ? 1 : 0, w = c - half * nw;
    const int64_t tk0 = half * h, t0 = half * (nsteps - h);
    const double qn = (double)(2 * h * nw) + 0.25;
    const double v0 = series_value<MODE>(x, r2, tk0 * nw + w, t0, w, ss, ws, j, qn, q);
    bool differs = false;
    Kahan a;
    for (int64_t t = 0; t < h; ++t) {
        const double v = series_value<MODE>(x, r2, (tk0 + t) * nw + w, t0 + t, w, ss, ws, j, qn, q);
        differs |= v != v0;
        a.add(v);
        if (y) y[t * mp] = v;
    }
    // a chain all of whose values are equal: its mean is its value (a rounded mean of equal values often is not), its variance 0
    const double mean = differs ? a.s / (double)h : v0;
    Kahan c2;
    for (int64_t t = 0; t < h; ++t) {
        const double v = y ? y[t * mp] : series_value<MODE>(x, r2, (tk0 + t) * nw + w, t0 + t, w, ss, ws, j, qn, q);
        const double e = v - mean;
        c2.add(e * e);
        if (y) y[t * mp] = e;
    }
    if (y)
        for (int64_t t = h; t < hp; ++t) y[t * mp] = 0.0;
    st[0] = mean;
    st[1] = c2.s / (double)(h - 1);
}

__global__ __launch_bounds__(RANK_THREADS) void k_rank_pack(const double* __restrict__ x, const unsigned* __restrict__ r2b,
                                                            const unsigned* __restrict__ r2f, int64_t nw, int64_t h, int64_t nsteps,
                                                            int64_t ss, int64_t ws, int64_t j, int K, const double* __restrict__ quant,
                                                            int64_t hp, int64_t mp, double* __restrict__ Y, double* __restrict__ cstat) {
    const int64_t c = (int64_t)blockIdx.x * RANK_THREADS + threadIdx.x;
    const int s = blockIdx.y;
    if (c >= mp) return;
    if (s == K && !r2f) return;                                 // (the folded series was not asked for)
    double* y = s < K ? Y + (int64_t)s * hp * mp + c : nullptr;
    double* st = cstat + ((int64_t)s * mp + c) * 2;
    if (c >= 2 * nw) {
        if (y)
            for (int64_t t = 0; t < hp; ++t) y[t * mp] = 0.0;
        st[0] = st[1] = 0.0;
        return;
    }
    if (s == 0) pack_chain<0>(x, r2b, nw, h, nsteps, ss, ws, j, c, 0.0, y, mp, hp, st);
    else if (s == K) pack_chain<0>(x, r2f, nw, h, nsteps, ss, ws, j, c, 0.0, y, mp, hp, st);
    else if (s == 1) pack_chain<1>(x, r2b, nw, h, nsteps, ss, ws, j, c, 0.0, y, mp, hp, st);
    else pack_chain<2>(x, r2b, nw, h, nsteps, ss, ws, j, c, quant[s - 2], y, mp, hp, st);
}

// ---------------------------------------------------------------------------------------------------------------- moments, R-hat
// blockIdx.x = series s <= K, blockIdx.y = parameter jj of the group
__global__ __launch_bounds__(RANK_THREADS) void k_rank_stats(const double* __restrict__ cstat, int64_t m, int64_t mp, int64_t h, int K,
                                                             int64_t j0, int fold, double* __restrict__ mom, double* __restrict__ rhat) {
    __shared__ double sw[REDUCE_WAVES];
    const int tid = threadIdx.x, s = blockIdx.x;
    const int64_t jj = blockIdx.y;
    if (s == K && !fold) return;
    const double* st = cstat + (jj * (K + 1) + s) * mp * 2;
    const double first = st[0];
    Kahan am, av;
    double other = 0.0;
    for (int64_t c = tid; c < m; c += RANK_THREADS) {
        am.add(st[2 * c]);
        av.add(st[2 * c + 1]);
        other += st[2 * c] != first ? 1.0 : 0.0;
    }
    const double hm = block_sum(am.s, sw) / (double)m;
    const double W = block_sum(av.s, sw) / (double)m;
    const double nother = block_sum(other, sw);                 // (a sum of zeros and ones: exact)
    Kahan ab;
    for (int64_t c = tid; c < m; c += RANK_THREADS) {
        const double e = st[2 * c] - hm;
        ab.add(e * e);
    }
    const double vm = nother > 0.0 ? block_sum(ab.s, sw) / (double)(m - 1) : 0.0;      // equal chain means: exactly 0
    if (tid == 0) {
        double* o = mom + (jj * (K + 1) + s) * 2;
        o[0] = W;
        o[1] = vm;
        if (rhat && (s == 0 || s == K)) {
            const double hd = (double)h, B = hd * vm;
            const double vp = (hd - 1.0) / hd * W + B / hd;
            rhat[(j0 + jj) * 2 + (s == K ? 1 : 0)] = vp == 0.0 ? NAN : sqrt(vp / W);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- lags
// A[y][k], y = blockIdx.y = (parameter of the group, series): k_diag_lags' sum — lag k = 64 D + r lives on diagonal r of the blocks of
// block diagonal D and, for r > 0, on diagonal r - 64 of those of D + 1; block row by block row — over m h
__global__ __launch_bounds__(RANK_THREADS) void k_rank_lags(const double* __restrict__ part, int64_t nb, int64_t pstride, int64_t max_lag,
                                                            double mh, double* __restrict__ A) {
    const int64_t k = (int64_t)blockIdx.x * RANK_THREADS + threadIdx.x;
    if (k > max_lag) return;
    const int64_t y = blockIdx.y;
    const int64_t D = k / 64, r = k % 64;
    const double* p0 = part + (y * pstride + D * nb) * 128 + 63 + r;
    const double* p1 = part + (y * pstride + (D + 1) * nb) * 128 + 63 + r - 64;
    double s = 0.0;
    for (int64_t I = 0; I + D < nb; ++I) {
        s += p0[I * 128];
        if (r > 0 && I + D + 1 < nb) s += p1[I * 128];
    }
    A[y * (max_lag + 1) + k] = s / mh;
}

// ---------------------------------------------------------------------------------------------------------------- Geyer
// one lane per (parameter of the group, series < K)
__global__ __launch_bounds__(64) void k_rank_geyer(const double* __restrict__ A, const double* __restrict__ mom, int64_t h, int64_t m,
                                                   int K, int64_t max_lag, int64_t j0, int64_t dg, double* __restrict__ Rw,
                                                   double* __restrict__ ess, int* __restrict__ stop, double* __restrict__ sd) {
    const int64_t y = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (y >= dg * K) return;
    const int64_t jj = y / K, s = y % K, j = j0 + jj;
    const double* a = A + y * (max_lag + 1);
    double* R = Rw + y * (max_lag + 3);
    const double hd = (double)h, n = (double)(m * h);
    const double mean_var = a[0] * hd / (hd - 1.0);
    const double var_plus = mean_var * (hd - 1.0) / hd + mom[(jj * (K + 1) + s) * 2 + 1];
    if (s == 1 && sd) sd[j] = sqrt(var_plus);
    if (!ess && !stop) return;
    double e = NAN;
    int st = -1;
    if (var_plus != 0.0) {
        if (max_lag < 1) {
            st = (int)max_lag | GPB_RANK_NO_BAND;
        } else {
            for (int64_t k = 0; k < max_lag + 3; ++k) R[k] = 0.0;
            double re = 1.0, ro = 1.0 - (mean_var - a[1]) / var_plus;
            R[0] = re;
            R[1] = ro;
            int64_t t = 1;
            bool beyond = false;
            while (t < h - 3 && re + ro > 0.0) {
                if (t + 2 > max_lag) {
                    beyond = true;
                    break;
                }
                re = 1.0 - (mean_var - a[t + 1]) / var_plus;
                ro = 1.0 - (mean_var - a[t + 2]) / var_plus;
                if (re + ro >= 0.0) {
                    R[t + 1] = re;
                    R[t + 2] = ro;
                }
                t += 2;
            }
            if (beyond) {
                st = (int)max_lag | GPB_RANK_NO_BAND;
            } else {
                const int64_t max_t = t - 2;
                if (re > 0.0) R[max_t + 1] = re;
                for (t = 1; t <= max_t - 2; t += 2)
                    if (R[t + 1] + R[t + 2] > R[t - 1] + R[t]) R[t + 1] = R[t + 2] = (R[t - 1] + R[t]) / 2.0;
                double sum = 0.0;
                for (int64_t k = 0; k <= max_t; ++k) sum += R[k];
                double tau = -1.0 + 2.0 * sum + R[max_t + 1];
                const double floor_tau = 1.0 / log10(n);
                tau = tau > floor_tau ? tau : floor_tau;
                e = n / tau;
                st = (int)max_t;
            }
        }
    }
    if (ess) ess[j * K + s] = e;
    if (stop) stop[j * K + s] = st;
}

}  // namespace

struct RankWant {
    bool rank2, rhat, acf;          // acf: ess, stop or sd
};

static int launch_rank_diag(gpb_ctx* ctx, const double* x, int64_t nsteps, int64_t nw, int64_t d, int64_t ss, int64_t ws,
                            const RankLevels& lv, int64_t max_lag, const RankWant& want, RankStage& out) {
    const int64_t h = nsteps / 2, m = 2 * nw, n = m * h;
    const int K = 2 + lv.nq;
    const int64_t hp = round_up(h, 64), mp = round_up(m, 16), nb = hp / 64;
    const int64_t nd = want.acf ? imin64((max_lag + 63) / 64, nb - 1) + 1 : 0;
    const int64_t nblk = nd * nb, nband = nblk + nb;
    if (nblk > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_chain_rank_diag: more than 2^31 - 1 blocks in the band");
    const int64_t nsb = (n + SORT_TILE - 1) / SORT_TILE;
    const bool series = want.rhat || want.acf;
    RankWs rw;
    Carver<int64_t> c0, c1;
    rw.lay(c0, n, nsb, 0, K, hp, mp, nband, max_lag);
    rw.lay(c1, n, nsb, 1, K, hp, mp, nband, max_lag);
    const int64_t fixed = c0.total(), per = c1.total() - c0.total();
    int64_t G = series ? (ctx->rank_ws_bytes / 8 - fixed) / per : 1;
    G = G < 1 ? 1 : (G > d ? d : G);
    if (G * K > 65535) G = 65535 / K;
    if (const int rc = ctx_carve(ctx, ctx->rank_ws, [&](Carver<int64_t>& cv) { rw.lay(cv, n, nsb, series ? G : 0, K, hp, mp, nband, max_lag); }))
        return rc;
    const dim3 gN((unsigned)((n + SORT_THREADS - 1) / SORT_THREADS)), gS((unsigned)nsb);
    hipStream_t st = ctx->stream;
    for (int64_t j0 = 0; j0 < d; j0 += G) {
        const int64_t dg = imin64(G, d - j0);
        for (int64_t jj = 0; jj < dg; ++jj) {
            const int64_t j = j0 + jj;
            for (int fold = 0; fold < (want.rhat ? 2 : 1); ++fold) {
                unsigned* r2 = fold ? rw.r2f : rw.r2b;
                GPB_HIP(hipMemsetAsync(rw.plan, 0, 32 * sizeof(unsigned), st));
                hipLaunchKernelGGL(k_rank_gather, gN, dim3(SORT_THREADS), 0, st, x, n, nw, h, nsteps, ss, ws, j,
                                   fold ? out.median + j : (const double*)nullptr, rw.keys[0], rw.pos[0], rw.plan);
                hipLaunchKernelGGL(k_rsort_plan, dim3(1), dim3(64), 0, st, rw.plan);
                for (int p = 0; p < 8; ++p) {
                    hipLaunchKernelGGL(k_rsort_count, gS, dim3(SORT_THREADS), 0, st, rw.keys[0], rw.keys[1], n, p, rw.plan, rw.counts);
                    hipLaunchKernelGGL(k_rsort_offsets, dim3(1), dim3(256), 0, st, nsb, p, rw.plan, rw.counts, rw.base);
                    hipLaunchKernelGGL(k_rsort_scatter, gS, dim3(SORT_THREADS), 0, st, rw.keys[0], rw.keys[1], rw.pos[0], rw.pos[1], n, p,
                                       rw.plan, rw.counts, rw.base);
                }
                if (want.rank2 || series)                       // (median and quant alone need the sorted keys only)
                    hipLaunchKernelGGL(k_rank_runs, gN, dim3(RANK_THREADS), 0, st, rw.keys[0], rw.keys[1], rw.pos[0], rw.pos[1], n,
                                       rw.plan, r2);
                if (!fold)
                    hipLaunchKernelGGL(k_rank_order, dim3(1), dim3(64), 0, st, rw.keys[0], rw.keys[1], n, rw.plan, lv, out.median + j,
                                       out.quant + j * lv.nq);
            }
            if (want.rank2) hipLaunchKernelGGL(k_rank_widen, gN, dim3(RANK_THREADS), 0, st, rw.r2b, n, out.rank2 + j * n);
            if (series)
                hipLaunchKernelGGL(k_rank_pack, dim3((unsigned)((mp + RANK_THREADS - 1) / RANK_THREADS), (unsigned)(K + 1)),
                                   dim3(RANK_THREADS), 0, st, x, rw.r2b, want.rhat ? rw.r2f : (const unsigned*)nullptr, nw, h, nsteps, ss,
                                   ws, j, K, out.quant + j * lv.nq, hp, mp, rw.Y + jj * K * hp * mp, rw.cstat + jj * (K + 1) * mp * 2);
        }
        if (!series) continue;
        hipLaunchKernelGGL(k_rank_stats, dim3((unsigned)(K + 1), (unsigned)dg), dim3(RANK_THREADS), 0, st, rw.cstat, m, mp, h, K, j0,
                           want.rhat ? 1 : 0, rw.mom, want.rhat ? out.rhat : (double*)nullptr);
        if (!want.acf) continue;
        hipLaunchKernelGGL(k_diag_gram, dim3((unsigned)nblk, (unsigned)(dg * K)), dim3(GEMM_THREADS), 0, st, rw.Y, hp, mp, nb, nband,
                           rw.part);
        hipLaunchKernelGGL(k_rank_lags, dim3((unsigned)((max_lag + RANK_THREADS) / RANK_THREADS), (unsigned)(dg * K)), dim3(RANK_THREADS),
                           0, st, rw.part, nb, nband, max_lag, (double)(m * h), rw.acov);
        hipLaunchKernelGGL(k_rank_geyer, dim3((unsigned)((dg * K + 63) / 64)), dim3(64), 0, st, rw.acov, rw.mom, h, m, K, max_lag, j0, dg,
                           rw.R, out.ess, out.stop, out.sd);
    }
    GPB_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_chain_rank_diag(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d, int64_t step_stride,
                                   int64_t walker_stride, const double* probs_host, int nq, int64_t max_lag, int on_device,
                                   int64_t* rank2, double* median, double* quant, double* rhat, double* ess, int32_t* stop, double* sd) {
    if (!ctx || !x_dev) return GPB_E_ARG;
    if (nsteps < 4) GPB_FAIL(GPB_E_ARG, "gpb_chain_rank_diag: need nsteps >= 4");
    if (nwalkers < 1 || d < 1) GPB_FAIL(GPB_E_ARG, "gpb_chain_rank_diag: need nwalkers >= 1 and d >= 1");
    if (nsteps > 0x7fffffffLL || nwalkers > 0x7fffffffLL || d > 0x7fffffffLL)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_rank_diag: more than 2^31 - 1 steps, walkers or parameters");
    const int64_t h = nsteps / 2;
    if ((__int128)2 * h * nwalkers > (__int128)0x7fffffffLL)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_rank_diag: more than 2^31 - 1 kept draws per parameter");
    if (nq < 1 || nq > GPB_RANK_MAX_Q || !probs_host) GPB_FAIL(GPB_E_ARG, "gpb_chain_rank_diag: need 1 <= nq <= 8 levels");
    for (int k = 0; k < nq; ++k)
        if (!(probs_host[k] > 0.0 && probs_host[k] < 1.0)) GPB_FAIL(GPB_E_ARG, "gpb_chain_rank_diag: a level outside (0, 1)");
    if (max_lag < 0 || max_lag > h - 1) GPB_FAIL(GPB_E_ARG, "gpb_chain_rank_diag: max_lag outside [0, nsteps / 2 - 1]");
    if (walker_stride < d || step_stride < d) GPB_FAIL(GPB_E_ARG, "gpb_chain_rank_diag: a stride below d (elements would alias)");
    const bool steps_outer = (__int128)step_stride >= (__int128)walker_stride * nwalkers;
    const bool walkers_outer = (__int128)walker_stride >= (__int128)step_stride * nsteps;
    if (!steps_outer && !walkers_outer)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_rank_diag: neither stride spans the other axis (elements would alias)");
    if (!rank2 && !median && !quant && !rhat && !ess && !stop && !sd) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    const int64_t n = 2 * h * nwalkers;
    RankLevels lv;
    lv.nq = nq;
    for (int k = 0; k < GPB_RANK_MAX_Q; ++k) {
        const double virt = k < nq ? probs_host[k] * (double)(n - 1) : 0.0;     // numpy's virtual index of the "linear" method
        const double fl = floor(virt);
        lv.lo[k] = (long long)fl;
        lv.hi[k] = lv.lo[k] + 1 < n ? lv.lo[k] + 1 : n - 1;
        lv.g[k] = virt - fl;
    }
    const RankWant want{rank2 != nullptr, rhat != nullptr, ess || stop || sd};
    // the kernels write every statistic they compute into the stage; what the caller wants is copied from there
    RankStage s;
    if (const int rc = ctx_carve(ctx, ctx->out_stage, [&](Carver<double>& cv) { s.lay(cv, d, nq, rank2 && !on_device ? d * n : 0); })) return rc;
    RankStage k = s;
    if (rank2 && on_device) k.rank2 = rank2;       // (d n int64: straight into the caller's device memory, staged for host memory only)
    if (!ess) k.ess = nullptr;
    if (!stop) k.stop = nullptr;
    if (!sd) k.sd = nullptr;
    if (const int rc = launch_rank_diag(ctx, x_dev, nsteps, nwalkers, d, step_stride, walker_stride, lv, max_lag, want, k)) return rc;
    const int64_t K = 2 + nq;
    HostOut so(ctx, on_device != 0, true);
    if (!on_device) so.at(rank2, s.rank2, d * n);
    so.at(median, s.median, d);
    so.at(quant, s.quant, d * nq);
    so.at(rhat, s.rhat, 2 * d);
    so.at(ess, s.ess, d * K);
    so.at(stop, s.stop, d * K);
    so.at(sd, s.sd, d);
    return so.finish();
}
