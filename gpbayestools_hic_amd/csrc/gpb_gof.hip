// gpb_gof.hip — goodness of fit of a set of posterior rows, data set by data set: the two pieces src/mcmc.py:23-65 (mvn_loglike)
// computes and throws away, 1/2 dY^T C^-1 dY and sum ln L_ii, kept per row and emulator, with the whitened residuals, the
// closed-form predictive p-value and the leave-one-data-set-out reweighting.  Per row w, with dY = y[w] - yexp and
// Cw = C[w] + Cadd = L L^T:
//   k_gof_row     one workgroup per row.  dY is appended to Cw as row M, and the left-looking Cholesky of gpb_sens.hip runs over the
//                 M + 1 rows: row M of the factor is z = L^-1 dY (z_j = (dY_j - sum_{k<j} z_k L_jk) / L_jj is the factorisation's
//                 own formula for an entry of row M), so the substitution costs no pass of its own.  The dot products are carried
//                 in two doubles (dot2_sub, as k_sens_row carries them).  The M + 1 rows live in LDS while (M + 1) (M | 1) <=
//                 GOF_LDS_DOUBLES; the leading dimension M | 1 is odd, so lane i at row i, 8 (M | 1) bytes apart, falls on 32
//                 different 8-byte bank pairs per half wave.  Larger rows are factorised in place in their slab of C_dev with z in
//                 the workspace.  Thread 0 then sums z^2 and ln L_ii in index order and evaluates p = Q(M / 2, chi2 / 2)
//                 (chi2_sf.h).  The row leaves chi2 and ll with the caller, z, the pulls dY_m / sqrt(Cw_mm), p and a flag in the
//                 workspace.
//   k_gof_chunk   one thread per observable (and one for the two scalars) and chunk of 256 consecutive rows: the chunk's sums of
//                 wt, wt p, wt z, wt z z, wt pull, wt pull pull by ONE tree, sixteen runs of sixteen rows.  A row with wt == 0 or
//                 a raised flag is skipped by a branch.
//   k_gof_add     one thread per entry adds the chunk sums to acc in chunk order.
//   k_inf_min / k_inf_chunk / k_inf_add   gpb_gof_influence: the exact minimum of an emulator's ll over the rows used, then the
//                 same chunk trees over the importance weights wt exp(-(ll - min)) and their moments of the parameters.
// No floating-point atomics; the only atomic is the integer count of bad rows.  The slab rule is gpb_sens_accumulate's: a call
// must start on a chunk boundary.
#include "gpb_internal.h"
#include "chi2_sf.h"
#include <math.h>

// Nothing in this file may be contracted (build.py compiles it with -ffp-contract=off, as it compiles gpb_sens.hip, for the
// reason given there): dot2_sub is error free only when every operation is rounded on its own.

namespace gpb {

namespace {

constexpr int GOF_THREADS = 256;
constexpr int GOF_CHUNK = 256;                   // rows per tree
constexpr int GOF_RUN = 16;                      // rows per run of the tree
constexpr int64_t GOF_LDS_DOUBLES = GPB_GOF_LDS_DOUBLES;
static_assert(GOF_CHUNK == GOF_RUN * GOF_RUN, "the tree is GOF_RUN runs of GOF_RUN rows");
static_assert(GOF_LDS_DOUBLES * 8 <= 64 * 1024, "the row kernel's dynamic LDS stays within the 64 KiB a launch may ask for unannounced");

__host__ __device__ inline int64_t gof_ld(int64_t M) { return M | 1; }
inline bool gof_in_lds(int64_t M) { return (M + 1) * gof_ld(M) <= GOF_LDS_DOUBLES; }

// k_sens_row's (hi, lo) -= x y (Dot2: TwoProduct by fma, TwoSum, the two errors added to lo); a copy, so that gpb_sens.hip and
// the bits of its tests stay as they are
__device__ __forceinline__ void dot2_sub(double& hi, double& lo, double x, double y) {
    const double p = -__dmul_rn(x, y);
    const double pe = -fma(x, y, p);
    const double s = __dadd_rn(hi, p);
    const double bb = __dsub_rn(s, hi);
    const double se = __dadd_rn(__dsub_rn(hi, __dsub_rn(s, bb)), __dsub_rn(p, bb));
    hi = s;
    lo = __dadd_rn(lo, __dadd_rn(se, pe));
}

// zw [W][M], pull [W][M], pw [W], flag [W] of the workspace
__global__ __launch_bounds__(GOF_THREADS) void k_gof_row(const double* __restrict__ y, double* Cg, const double* __restrict__ yexp,
                                                         const double* __restrict__ Cadd, const double* __restrict__ wt, int M,
                                                         int in_lds, double* __restrict__ chi2_out, double* __restrict__ ll_out,
                                                         double* zw, double* __restrict__ pull, double* __restrict__ pw,
                                                         int* __restrict__ flag, unsigned long long* nbad) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int64_t w = blockIdx.x;
    const int t = threadIdx.x;
    if (wt && wt[w] == 0.0) {                    // (uniform: the whole workgroup leaves; the row's outputs say it was not evaluated)
        if (t == 0) {
            flag[w] = 0;
            chi2_out[w] = NAN;
            ll_out[w] = NAN;
        }
        return;
    }
    const int ld = in_lds ? (int)gof_ld(M) : M;
    double* C = in_lds ? sm : Cg + w * (int64_t)M * M;
    double* zr = in_lds ? sm + (int64_t)M * ld : zw + w * (int64_t)M;      // row M of the augmented matrix
    const double* Cw = Cg + w * (int64_t)M * M;
    const double* yw = y + w * (int64_t)M;
    for (int64_t e = t; e < (int64_t)M * M; e += GOF_THREADS) {
        const int i = (int)(e / M), k = (int)(e - (int64_t)i * M);
        const double v = Cadd ? Cw[e] + Cadd[e] : Cw[e];
        C[(int64_t)i * ld + k] = v;
        if (i == k) pull[w * M + i] = __dsub_rn(yw[i], yexp[i]) / sqrt(v);
    }
    for (int m = t; m < M; m += GOF_THREADS) zr[m] = __dsub_rn(yw[m], yexp[m]);
    __syncthreads();
    // left-looking Cholesky over rows j .. M (row M: dY, becoming z), the sums in two doubles.  Every thread reads the same pivot
    // after the barrier: the exit is uniform.
    bool bad = false;
    for (int j = 0; j < M; ++j) {
        const double* Lj = C + (int64_t)j * ld;
        for (int i = j + t; i <= M; i += GOF_THREADS) {
            double* Li = i < M ? C + (int64_t)i * ld : zr;
            double hi = Li[j], lo = 0.0;
            for (int k = 0; k < j; ++k) dot2_sub(hi, lo, Li[k], Lj[k]);
            Li[j] = __dadd_rn(hi, lo);
        }
        __syncthreads();
        const double ajj = Lj[j];
        if (!(ajj > 0.0)) {
            bad = true;
            break;
        }
        const double dd = sqrt(ajj);
        __syncthreads();
        for (int i = j + 1 + t; i <= M; i += GOF_THREADS) {
            double* Li = i < M ? C + (int64_t)i * ld : zr;
            Li[j] = Li[j] / dd;
        }
        if (t == 0) C[(int64_t)j * ld + j] = dd;
        __syncthreads();
    }
    if (bad) {
        if (t == 0) {
            flag[w] = 1;
            chi2_out[w] = NAN;
            ll_out[w] = NAN;
            atomicAdd(nbad, 1ull);
        }
        return;
    }
    if (in_lds)
        for (int m = t; m < M; m += GOF_THREADS) zw[w * M + m] = zr[m];
    if (t == 0) {
        double chi2 = 0.0, sld = 0.0;
        for (int m = 0; m < M; ++m) {
            const double z = zr[m];
            chi2 = __dadd_rn(chi2, __dmul_rn(z, z));
            sld = __dadd_rn(sld, log(C[(int64_t)m * ld + m]));
        }
        chi2_out[w] = chi2;
        ll_out[w] = __dsub_rn(__dmul_rn(-0.5, chi2), sld);
        pw[w] = chi2_sf(chi2, (double)M);
        flag[w] = 0;
    }
}

// thread q < M: the four sums of observable q; thread q == M: sum wt and sum wt p
__global__ __launch_bounds__(GOF_THREADS) void k_gof_chunk(const double* __restrict__ wt, int64_t W, int M,
                                                           const double* __restrict__ zw, const double* __restrict__ pull,
                                                           const double* __restrict__ pw, const int* __restrict__ flag,
                                                           double* __restrict__ part, int64_t nacc) {
    const int64_t c = blockIdx.x;
    const int q = (int)(blockIdx.y * GOF_THREADS + threadIdx.x);
    if (q > M) return;
    const bool scal = q == M;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int g = 0; g < GOF_RUN; ++g) {
        double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
        for (int k = 0; k < GOF_RUN; ++k) {
            const int64_t w = c * GOF_CHUNK + g * GOF_RUN + k;
            double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
            if (w < W && flag[w] == 0) {
                const double a = wt ? wt[w] : 1.0;
                if (a != 0.0) {
                    if (scal) {
                        t0 = a;
                        t1 = __dmul_rn(a, pw[w]);
                    } else {
                        const double z = zw[w * M + q], u = pull[w * M + q];
                        t0 = __dmul_rn(a, z);
                        t1 = __dmul_rn(a, __dmul_rn(z, z));
                        t2 = __dmul_rn(a, u);
                        t3 = __dmul_rn(a, __dmul_rn(u, u));
                    }
                }
            }
            r0 = __dadd_rn(r0, t0);
            r1 = __dadd_rn(r1, t1);
            r2 = __dadd_rn(r2, t2);
            r3 = __dadd_rn(r3, t3);
        }
        s0 = __dadd_rn(s0, r0);
        s1 = __dadd_rn(s1, r1);
        s2 = __dadd_rn(s2, r2);
        s3 = __dadd_rn(s3, r3);
    }
    double* out = part + c * nacc;
    if (scal) {
        out[GPB_GOF_ACC_W] = s0;
        out[GPB_GOF_ACC_P] = s1;
    } else {
        out[GPB_GOF_ACC_Z + q] = s0;
        out[GPB_GOF_ACC_Z2(M) + q] = s1;
        out[GPB_GOF_ACC_PULL(M) + q] = s2;
        out[GPB_GOF_ACC_PULL2(M) + q] = s3;
    }
}

__global__ __launch_bounds__(GOF_THREADS) void k_gof_add(const double* __restrict__ part, int64_t nchunks, int64_t nacc,
                                                         double* __restrict__ acc, long long* cnt, int64_t W) {
    const int64_t e = (int64_t)blockIdx.x * GOF_THREADS + threadIdx.x;
    if (e == 0) cnt[0] += W;
    if (e >= nacc) return;
    double a = acc[e];
    for (int64_t c = 0; c < nchunks; ++c) a = __dadd_rn(a, part[c * nacc + e]);
    acc[e] = a;
}

__global__ __launch_bounds__(GOF_THREADS) void k_chi2_sf(const double* __restrict__ x, int64_t n, double ndf, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * GOF_THREADS + threadIdx.x;
    if (i < n) out[i] = chi2_sf(x[i], ndf);
}

// one workgroup per emulator: the minimum of ll over the rows used (+inf when there is none).  A minimum is exact and does not
// depend on the order it is taken in.
__global__ __launch_bounds__(GOF_THREADS) void k_inf_min(const double* __restrict__ ll, int64_t S, int64_t ld,
                                                         const double* __restrict__ wt, double* __restrict__ mn) {
    __shared__ double red[GOF_THREADS];
    const int e = blockIdx.x, t = threadIdx.x;
    double m = INFINITY;
    for (int64_t s = t; s < S; s += GOF_THREADS) {
        const double v = ll[e * ld + s];
        if (v == v && (!wt || wt[s] != 0.0) && v < m) m = v;
    }
    red[t] = m;
    __syncthreads();
    for (int h = GOF_THREADS / 2; h > 0; h >>= 1) {
        if (t < h && red[t + h] < red[t]) red[t] = red[t + h];
        __syncthreads();
    }
    if (t == 0) mn[e] = red[0];
}

// thread q < d: sum w x_q and sum w x_q x_q of chunk c, emulator e; thread q == d: sum w and sum w w
__global__ __launch_bounds__(GOF_THREADS) void k_inf_chunk(const double* __restrict__ ll, int64_t S, int64_t ld,
                                                           const double* __restrict__ x, int d, const double* __restrict__ wt,
                                                           const double* __restrict__ mn, double* __restrict__ part, int E) {
    const int64_t c = blockIdx.x;
    const int e = blockIdx.y;
    const int q = (int)(blockIdx.z * GOF_THREADS + threadIdx.x);
    if (q > d) return;
    const bool scal = q == d;
    const double m0 = mn[e];
    double s0 = 0.0, s1 = 0.0;
    for (int g = 0; g < GOF_RUN; ++g) {
        double r0 = 0.0, r1 = 0.0;
        for (int k = 0; k < GOF_RUN; ++k) {
            const int64_t s = c * GOF_CHUNK + g * GOF_RUN + k;
            double t0 = 0.0, t1 = 0.0;
            if (s < S) {
                const double v = ll[e * ld + s];
                const double a = wt ? wt[s] : 1.0;
                if (v == v && a != 0.0) {
                    const double wgt = __dmul_rn(a, exp(-__dsub_rn(v, m0)));
                    if (scal) {
                        t0 = wgt;
                        t1 = __dmul_rn(wgt, wgt);
                    } else {
                        const double xv = x[s * d + q];
                        t0 = __dmul_rn(wgt, xv);
                        t1 = __dmul_rn(wgt, __dmul_rn(xv, xv));
                    }
                }
            }
            r0 = __dadd_rn(r0, t0);
            r1 = __dadd_rn(r1, t1);
        }
        s0 = __dadd_rn(s0, r0);
        s1 = __dadd_rn(s1, r1);
    }
    double* out = part + (c * E + e) * (int64_t)(2 + 2 * d);
    if (scal) {
        out[0] = s0;
        out[1] = s1;
    } else {
        out[2 + q] = s0;
        out[2 + d + q] = s1;
    }
}

__global__ __launch_bounds__(GOF_THREADS) void k_inf_add(const double* __restrict__ part, int64_t nchunks, int E, int nent,
                                                         double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * GOF_THREADS + threadIdx.x;
    if (i >= (int64_t)E * nent) return;
    double a = 0.0;
    for (int64_t c = 0; c < nchunks; ++c) a = __dadd_rn(a, part[c * E * nent + i]);
    out[i] = a;
}

}  // namespace

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_gof_accumulate(gpb_ctx* ctx, int64_t W, int64_t M, const double* y_dev, double* C_dev, const double* yexp_dev,
                                  const double* Cadd_dev, const double* wt_dev, double* chi2_out, double* ll_out, double* acc_dev,
                                  int64_t* cnt_dev) {
    if (!ctx || !y_dev || !C_dev || !yexp_dev || !chi2_out || !ll_out || !acc_dev || !cnt_dev) return GPB_E_ARG;
    if (W < 0 || M < 1) GPB_FAIL(GPB_E_ARG, "gpb_gof_accumulate: need W >= 0 and M >= 1");
    if (M > GPB_GOF_MAX_M) GPB_FAIL(GPB_E_ARG, "gpb_gof_accumulate: M above 2048");
    if (W > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_gof_accumulate: more than 2^31 - 1 rows in one call");
    if (W == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    long long seen = 0;
    GPB_HIP(hipMemcpyAsync(&seen, cnt_dev, sizeof(seen), hipMemcpyDeviceToHost, ctx->stream));
    GPB_HIP(hipStreamSynchronize(ctx->stream));
    if (seen < 0 || seen % GOF_CHUNK != 0)
        GPB_FAIL(GPB_E_STATE, "gpb_gof_accumulate: the rows seen so far are not a multiple of 256 (only the last slab may be ragged)");
    const bool in_lds = gof_in_lds(M);
    const int64_t nacc = GPB_GOF_ACC_DOUBLES(M), nchunks = (W + GOF_CHUNK - 1) / GOF_CHUNK;
    double *zw, *pull, *pw, *part;
    int* flag;
    if (const int rc = ctx_carve(ctx, ctx->gof_ws, [&](Carver<double>& c) {
            zw = c.take<double>(W * M);
            pull = c.take<double>(W * M);
            pw = c.take<double>(W);
            part = c.take<double>(nchunks * nacc);
            flag = c.take<int>(W);
        }))
        return rc;
    const size_t lds = in_lds ? sizeof(double) * (size_t)((M + 1) * gof_ld(M)) : 0;
    hipLaunchKernelGGL(k_gof_row, dim3((unsigned)W), dim3(GOF_THREADS), lds, ctx->stream, y_dev, C_dev, yexp_dev, Cadd_dev, wt_dev,
                       (int)M, in_lds ? 1 : 0, chi2_out, ll_out, zw, pull, pw, flag, reinterpret_cast<unsigned long long*>(cnt_dev + 1));
    hipLaunchKernelGGL(k_gof_chunk, dim3((unsigned)nchunks, (unsigned)((M + 1 + GOF_THREADS - 1) / GOF_THREADS)), dim3(GOF_THREADS), 0,
                       ctx->stream, wt_dev, W, (int)M, zw, pull, pw, flag, part, nacc);
    hipLaunchKernelGGL(k_gof_add, dim3((unsigned)((nacc + GOF_THREADS - 1) / GOF_THREADS)), dim3(GOF_THREADS), 0, ctx->stream, part,
                       nchunks, nacc, acc_dev, reinterpret_cast<long long*>(cnt_dev), W);
    GPB_HIP(hipGetLastError());
    return 0;
}

extern "C" int gpb_chi2_sf(gpb_ctx* ctx, const double* x_dev, int64_t n, double ndf, double* out_dev) {
    if (!ctx || !x_dev || !out_dev) return GPB_E_ARG;
    if (n < 0 || n > 0x7fffffffLL || !(ndf > 0.0) || ndf == INFINITY)
        GPB_FAIL(GPB_E_ARG, "gpb_chi2_sf: need 0 <= n <= 2^31 - 1 and a finite ndf > 0");
    if (n == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_chi2_sf, dim3((unsigned)((n + GOF_THREADS - 1) / GOF_THREADS)), dim3(GOF_THREADS), 0, ctx->stream, x_dev, n, ndf,
                       out_dev);
    GPB_HIP(hipGetLastError());
    return 0;
}

extern "C" int gpb_gof_influence(gpb_ctx* ctx, const double* ll_T, int64_t E, int64_t S, int64_t ld, const double* x_dev, int64_t d,
                                 const double* wt_dev, double* out_dev) {
    if (!ctx || !ll_T || !x_dev || !out_dev) return GPB_E_ARG;
    if (E < 1 || E > GPB_GOF_MAX_E || d < 1 || d > GPB_GOF_MAX_D) GPB_FAIL(GPB_E_ARG, "gpb_gof_influence: need 1 <= E <= 64 and 1 <= d <= 512");
    if (S < 1 || S > 0x7fffffffLL || ld < S) GPB_FAIL(GPB_E_ARG, "gpb_gof_influence: need 1 <= S <= 2^31 - 1 and ld >= S");
    GPB_HIP(hipSetDevice(ctx->device));
    const int nent = (int)(2 + 2 * d);
    const int64_t nchunks = (S + GOF_CHUNK - 1) / GOF_CHUNK;
    double *mn, *part;
    if (const int rc = ctx_carve(ctx, ctx->gof_ws, [&](Carver<double>& c) {
            mn = c.take<double>(E);
            part = c.take<double>(nchunks * E * nent);
        }))
        return rc;
    hipLaunchKernelGGL(k_inf_min, dim3((unsigned)E), dim3(GOF_THREADS), 0, ctx->stream, ll_T, S, ld, wt_dev, mn);
    hipLaunchKernelGGL(k_inf_chunk, dim3((unsigned)nchunks, (unsigned)E, (unsigned)((d + 1 + GOF_THREADS - 1) / GOF_THREADS)),
                       dim3(GOF_THREADS), 0, ctx->stream, ll_T, S, ld, x_dev, (int)d, wt_dev, mn, part, (int)E);
    hipLaunchKernelGGL(k_inf_add, dim3((unsigned)((E * nent + GOF_THREADS - 1) / GOF_THREADS)), dim3(GOF_THREADS), 0, ctx->stream,
                       part, nchunks, (int)E, nent, out_dev);
    GPB_HIP(hipGetLastError());
    return 0;
}
