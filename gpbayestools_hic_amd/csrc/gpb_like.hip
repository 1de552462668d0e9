// gpb_like.hip — PC -> observable transform, batched multivariate-normal log-likelihood, prior box and the
// compaction of a batch to the rows inside it.  (The stretch move that drives them: gpb_stretch.hip.)
//   k_obs       Emulator.predict after the per-GP calls            src/emulator.py:555-605
//   k_loglike   Chain._predict block + mvn_loglike, fused          src/mcmc.py:23-65,153-166,288-293
//   k_box       strict prior box + constant                        src/mcmc.py:194-198,275-276,296-297
#include "gpb_internal.h"
#include <math.h>

namespace gpb {

// ------------------------------------------------------------------ observable transform
// The emulator's observables from the principal components of one walker, in the four modes: the mean of column m from the
// PC means zm[P], the model covariance entry (i, j) from the PC variances zv[P] and the observable means mo[M].
struct ObsModel {
    int P, M;
    bool no_pca, expdiag;
    const double *A, *mu, *scale, *C0;
    __device__ __forceinline__ ObsModel(int P_, int M_, int mode, const double* A_, const double* mu_, const double* scale_,
                                        const double* C0_)
        : P(P_), M(M_), no_pca(mode == GPB_MODE_NO_PCA || mode == GPB_MODE_NO_PCA_EXPDIAG),
          expdiag(mode == GPB_MODE_EXPDIAG || mode == GPB_MODE_NO_PCA_EXPDIAG), A(A_), mu(mu_), scale(scale_), C0(C0_) {}
    // (zm, zv, mo: anything indexable — an array in LDS, or a view of one walker's column of the predict workspace)
    template <class ZM>
    __device__ __forceinline__ double mean(const ZM& zm, int m) const {
        double v;
        if (!no_pca) {
            v = 0.0;
            for (int p = 0; p < P; ++p) v = fma(zm[p], A[p * M + m], v);   // src/emulator.py:559-561, 373-374
            v += mu[m];
        } else {
            v = zm[m] * scale[m] + mu[m];                                    // :563-565
        }
        if (expdiag) v = exp(v);                                             // :567-568
        return v;
    }
    template <class ZV, class MO>
    __device__ __forceinline__ double cov(const ZV& zv, const MO& mo, int i, int j) const {
        double v;
        if (!no_pca) {
            if (expdiag && i != j) v = 0.0;
            else {
                v = 0.0;
                for (int p = 0; p < P; ++p) v = fma(zv[p] * A[p * M + i], A[p * M + j], v);   // :584-586
                v += C0[i * M + j];                                                            // :587
            }
        } else {
            v = (i == j) ? zv[i] : 0.0;                                                        // :590-592
        }
        if (expdiag && i == j) {
            const double f = sqrt(v) * mo[i];                                                  // :599-600
            v = f * f;
        }
        return v;
    }
};

// materialised: one workgroup per walker; writes mean[w][M] and (optionally) cov[w][M][M]
__global__ __launch_bounds__(256) void k_obs(const double* __restrict__ mean_pc, const double* __restrict__ var_pc,
                                             const double* __restrict__ estd, int64_t Wld, int P, int M, int mode,
                                             const double* __restrict__ A, const double* __restrict__ mu,
                                             const double* __restrict__ scale, const double* __restrict__ C0,
                                             double* __restrict__ mean_out, double* __restrict__ cov_out) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* zm = sm;            // [P]
    double* zv = sm + P;        // [P]
    double* mo = sm + 2 * P;    // [M]
    const int64_t w = blockIdx.x;
    const int tid = threadIdx.x;
    const ObsModel obs(P, M, mode, A, mu, scale, C0);
    const double e = estd ? estd[w] : 0.0;
    for (int p = tid; p < P; p += 256) {
        zm[p] = mean_pc[(int64_t)p * Wld + w];
        zv[p] = var_pc ? (var_pc[(int64_t)p * Wld + w] + e * e) : 0.0;     // src/emulator.py:578-579
    }
    __syncthreads();
    for (int m = tid; m < M; m += 256) {
        const double v = obs.mean(zm, m);
        mo[m] = v;
        mean_out[w * M + m] = v;
    }
    if (!cov_out) return;
    __syncthreads();
    double* co = cov_out + w * (int64_t)M * M;
    for (int e2 = tid; e2 < M * M; e2 += 256) co[e2] = obs.cov(zv, mo, e2 / M, e2 % M);
}

int launch_obs(gpb_ctx* ctx, int64_t W, const double* estd_dev, double* mean_dev, double* cov_dev) {
    const size_t sh = (2 * ctx->P + ctx->M) * sizeof(double);
    hipLaunchKernelGGL(k_obs, dim3((unsigned)W), dim3(256), sh, ctx->stream, ctx->mean_pc,
                       cov_dev ? ctx->var_pc : nullptr, estd_dev, ctx->Wld, (int)ctx->P, (int)ctx->M, ctx->mode,
                       ctx->A, ctx->mu, ctx->scale, ctx->C0, mean_dev, cov_dev);
    GPB_HIP(hipGetLastError());
    return 0;
}

// One walker's column of the predict workspace [P][Wld] as ObsModel sees k_obs's LDS copies: zm[p], zv[p] (+ extra_std^2)
struct PcMeanCol {
    const double* col;
    int64_t Wld;
    __device__ __forceinline__ double operator[](int p) const { return col[(int64_t)p * Wld]; }
};
struct PcVarCol {
    const double* col;
    int64_t Wld;
    double e2;        // fl(extra_std^2), rounded on its own as k_obs forms it (__dmul_rn: never contracted into the sum)
    __device__ __forceinline__ double operator[](int p) const { return col[(int64_t)p * Wld] + e2; }        // src/emulator.py:578-579
};
struct OneValue {
    double v;
    __device__ __forceinline__ double operator[](int) const { return v; }
};

// diagonal only, observable-major (gpb_emu_predict_diag): thread (lane = walker, y = observable) forms mean_T[m][w] = k_obs's
// mean[w][m] and var_T[m][w] = its cov[w][m][m] by the same ObsModel calls.  Walkers on the lanes: the reads of mean_pc / var_pc
// [P][Wld] and the writes of the [M][ld] outputs are contiguous per wave; nothing of size M x M is formed.
constexpr int DIAG_ROWS = 4;
__global__ __launch_bounds__(64 * DIAG_ROWS) void k_obs_diag(const double* __restrict__ mean_pc, const double* __restrict__ var_pc,
                                                             const double* __restrict__ estd, int64_t W, int64_t Wld, int P, int M,
                                                             int mode, const double* __restrict__ A, const double* __restrict__ mu,
                                                             const double* __restrict__ scale, const double* __restrict__ C0,
                                                             double* __restrict__ mean_T, double* __restrict__ var_T, int64_t ld) {
    const int64_t w = blockIdx.x * (int64_t)64 + threadIdx.x;
    const int m = blockIdx.y * DIAG_ROWS + threadIdx.y;
    if (w >= W || m >= M) return;
    const ObsModel obs(P, M, mode, A, mu, scale, C0);
    const double v = obs.mean(PcMeanCol{mean_pc + w, Wld}, m);
    mean_T[(int64_t)m * ld + w] = v;
    if (!var_T) return;
    const double e = estd ? estd[w] : 0.0;
    var_T[(int64_t)m * ld + w] = obs.cov(PcVarCol{var_pc + w, Wld, __dmul_rn(e, e)}, OneValue{v}, m, m);
}

int launch_obs_diag(gpb_ctx* ctx, int64_t W, const double* estd_dev, double* mean_T, double* var_T, int64_t ld) {
    const int64_t gy = (ctx->M + DIAG_ROWS - 1) / DIAG_ROWS;
    if (gy > 65535) GPB_FAIL(GPB_E_ARG, "gpb_emu_predict_diag: more than 262140 observables");
    hipLaunchKernelGGL(k_obs_diag, dim3((unsigned)((W + 63) / 64), (unsigned)gy), dim3(64, DIAG_ROWS), 0, ctx->stream, ctx->mean_pc,
                       var_T ? ctx->var_pc : nullptr, estd_dev, W, ctx->Wld, (int)ctx->P, (int)ctx->M, ctx->mode, ctx->A, ctx->mu,
                       ctx->scale, ctx->C0, mean_T, var_T, ld);
    GPB_HIP(hipGetLastError());
    return 0;
}

// Right-looking Cholesky of the augmented (M+1) x M lower matrix held at c (LDS or global slab),
// then ll[w] = -1/2 |v|^2 - sum log L_jj with v = last row.  Non-PD -> NaN and a counted status.
__device__ __forceinline__ void chol_aug_finish(double* c, int ld, int M, double* dg, double* __restrict__ ll,
                                                int64_t w, int accumulate, int* __restrict__ notpd) {
    const int tid = threadIdx.x;
    const int ty = tid >> 4, tx = tid & 15;
    bool bad = false;
    for (int j = 0; j < M; ++j) {
        const double ajj = c[j * ld + j];
        if (!(ajj > 0.0)) bad = true;
        const double dd = sqrt(ajj);
        __syncthreads();
        for (int i = j + 1 + tid; i <= M; i += 256) c[i * ld + j] = c[i * ld + j] / dd;
        if (tid == 0) dg[j] = dd;
        __syncthreads();
        for (int i = j + 1 + ty; i <= M; i += 16) {
            const double lij = c[i * ld + j];
            const int kmax = (i < M) ? i : (M - 1);
            for (int k = j + 1 + tx; k <= kmax; k += 16) c[i * ld + k] = fma(-lij, c[k * ld + j], c[i * ld + k]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        double q = 0.0, ld_sum = 0.0;
        for (int j = 0; j < M; ++j) {
            const double v = c[M * ld + j];
            q = fma(v, v, q);
            ld_sum += log(dg[j]);
        }
        double r = -0.5 * q - ld_sum;
        if (bad) {
            r = nan("");
            atomicAdd(notpd, 1);
        }
        ll[w] = accumulate ? (ll[w] + r) : r;
    }
}

// Generic batched mvn_loglike(y, cov) (src/mcmc.py:23-65) on caller-provided dY[W,M], cov[W,M,M].
template <bool GWS>
__global__ __launch_bounds__(256) void k_mvn(const double* __restrict__ dY, const double* __restrict__ cov, int M,
                                             double* __restrict__ gws, double* __restrict__ ll,
                                             int* __restrict__ notpd) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int64_t w = blockIdx.x;
    const int tid = threadIdx.x, ld = M + 1;
    double* dg = sm;
    double* c;
    if (GWS) c = gws + w * (int64_t)(M + 1) * ld;      // separate instantiations keep LDS accesses as ds_* ops
    else     c = sm + M;
    const double* cw = cov + w * (int64_t)M * M;
    for (int e2 = tid; e2 < M * M; e2 += 256) {
        const int i = e2 / M, j = e2 % M;
        if (j <= i) c[i * ld + j] = cw[e2];
    }
    for (int m = tid; m < M; m += 256) c[M * ld + m] = dY[w * M + m];
    __syncthreads();
    chol_aug_finish(c, ld, M, dg, ll, w, 0, notpd);
}

// ------------------------------------------------------------------ fused block log-likelihood
// One workgroup per walker.  Builds dY = mean - y_exp and C = cov_model + cov_exp directly in LDS
// (or in a global scratch slab when M > 128), then factorises the augmented matrix
//        [ C   . ]            [ L    0 ]
//        [ dY^T . ]   ->      [ v^T  . ]     with  L v = dY,
// so that  -1/2 dY^T C^-1 dY - sum log L_ii = -1/2 |v|^2 - sum log L_ii   (src/mcmc.py:42-65).
template <bool GWS>
__global__ __launch_bounds__(256) void k_loglike(const double* __restrict__ mean_pc,
                                                 const double* __restrict__ var_pc, int64_t Wld, int P, int M,
                                                 int mode, const double* __restrict__ A,
                                                 const double* __restrict__ mu, const double* __restrict__ scale,
                                                 const double* __restrict__ C0, const double* __restrict__ yexp,
                                                 const double* __restrict__ Cexp, double* __restrict__ gws,
                                                 double* __restrict__ ll, int accumulate, int* __restrict__ notpd) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int64_t w = blockIdx.x;
    const int tid = threadIdx.x;
    const int ld = M + 1;
    double* zm = sm;                 // [P]
    double* zv = sm + P;             // [P]
    double* mo = sm + 2 * P;         // [M]
    double* dg = sm + 2 * P + M;     // [M] pivots
    double* c;                       // [(M+1)][ld]
    if (GWS) c = gws + w * (int64_t)(M + 1) * ld;
    else     c = sm + 2 * P + 2 * M;
    const ObsModel obs(P, M, mode, A, mu, scale, C0);
    for (int p = tid; p < P; p += 256) {
        zm[p] = mean_pc[(int64_t)p * Wld + w];
        zv[p] = var_pc[(int64_t)p * Wld + w];       // extra_std == 0 on this path (src/mcmc.py:205,281)
    }
    __syncthreads();
    for (int m = tid; m < M; m += 256) {
        const double v = obs.mean(zm, m);
        mo[m] = v;
        c[M * ld + m] = v - yexp[m];                // dY (src/mcmc.py:288)
    }
    __syncthreads();
    for (int e2 = tid; e2 < M * M; e2 += 256) {
        const int i = e2 / M, j = e2 % M;
        if (j > i) continue;
        c[i * ld + j] = obs.cov(zv, mo, i, j) + Cexp[i * M + j];        // src/mcmc.py:290
    }
    __syncthreads();
    chol_aug_finish(c, ld, M, dg, ll, w, accumulate, notpd);
}

// ------------------------------------------------------------------ fused block log-likelihood, register-resident
// Fast path for the PCA mode with M <= 64 (every emulator of the reference's analyses): ONE WAVE per
// walker, lane i owns row i of C = sum_p var_p A_p^T A_p + C_trunc + C_exp in VGPRs.  Right-looking
// Cholesky fully unrolled: pivots and column entries are broadcast with v_readlane (-> SGPR operands of
// the v_fma_f64), no LDS traffic and no barriers inside the factorisation; the forward solve L v = dY is
// folded into the same sweep.  Rows >= M are padded with the identity (log 1 = 0, v = 0).
__device__ __forceinline__ double readlane_f64(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// Optional fused prior box (src/mcmc.py:194-198,275-276,296-297): X == nullptr -> plain block log-likelihood.
struct BoxArgs {
    const double* X;      // [W][d] walker positions
    const double* lo;     // [d]
    const double* hi;     // [d]
    int d;
    double outside;       // -inf or -1e300
    double inside_const;  // 2 log(1e-16)
    // compacted batch (launch_compact): X == nullptr, the box is already applied; workspace row w is row cmp[4 + w] of
    // the output, rows w >= cmp[0] do not exist (their numbers are stale workspace contents and are discarded)
    const int* cmp;
};

// Optional fused k_finalize: mpart != nullptr -> the kernel sums the per-chunk mean partials and the per-row-block
// sum-of-squares partials of its walker itself, in k_finalize's order (same bits), instead of reading mean_pc / var_pc.
// One launch and one dependent pass over HBM less per log-probability batch; needs P <= 32.
struct PartArgs {
    const double* mpart;  // [nchunk][P][Wld]
    const double* spart;  // [nI64][P][Wld]
    const double* amp;    // [P]
    const double* noise;  // [P]
    int nchunk, nI64;
};

// The end of a dense block log-likelihood kernel, by the one lane that writes row w's result -1/2 q - logdet (formed here,
// behind the load of the scatter index: handed over finished, k_loglike_reg<64> spills 12 more scalar registers): NaN and a
// counted status when the block is not positive definite inside the box, the emulators' blocks added up, the box's constant
// or `outside`, and the scatter through cmp for a compacted batch.
__device__ __forceinline__ void loglike_finish(const BoxArgs& box, int64_t w, double q, double logdet, bool bad, bool inside,
                                               int accumulate, double* ll, int* notpd) {
    const int64_t wo = box.cmp ? box.cmp[4 + w] : w;
    double r = -0.5 * q - logdet;
    if (bad && inside) {
        r = nan("");
        atomicAdd(notpd, 1);
    }
    r = accumulate ? (ll[wo] + r) : r;
    if (box.X) r = inside ? (r + box.inside_const) : box.outside;
    else if (box.cmp) r += box.inside_const;
    ll[wo] = r;
}

template <int MP>
__global__ __launch_bounds__(256) void k_loglike_reg(const double* __restrict__ mean_pc,
                                                     const double* __restrict__ var_pc, int64_t Wld, int64_t W, int P,
                                                     int M, const double* __restrict__ A,
                                                     const double* __restrict__ mu, const double* __restrict__ C0,
                                                     const double* __restrict__ yexp, const double* __restrict__ Cexp,
                                                     double* __restrict__ ll, int accumulate, int* __restrict__ notpd,
                                                     BoxArgs box, PartArgs part) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* sC = sm;                         // [64][MP+1]  C_trunc + C_exp, identity padded
    double* sA = sm + 64 * (MP + 1);         // [P][64]     A, zero padded
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int e = tid; e < 64 * MP; e += 256) {
        const int i = e / MP, k = e % MP;
        double v = (i == k) ? 1.0 : 0.0;
        if (i < M && k < M) v = C0[i * M + k] + Cexp[i * M + k];
        sC[i * (MP + 1) + k] = v;
    }
    for (int e = tid; e < P * 64; e += 256) {
        const int p = e >> 6, i = e & 63;
        sA[e] = (i < M) ? A[p * M + i] : 0.0;
    }
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * 4 + wave;
    if (w >= W) return;                      // wave-uniform
    double a[MP];
#pragma unroll
    for (int k = 0; k < MP; ++k) a[k] = sC[lane * (MP + 1) + k];
    double y = (lane < M) ? (mu[lane] - yexp[lane]) : 0.0;
    double zmv = 0.0;                        // fused finalize: lane p = mean of GP p, lane 32 + p = its variance
    if (part.mpart) {
        const int pl = lane & 31;
        if (pl < P) {
            if (lane < 32) {
                double m = 0.0;
#pragma unroll 8
                for (int c = 0; c < part.nchunk; ++c) m += part.mpart[((int64_t)c * P + pl) * Wld + w];
                zmv = m;
            } else {
                double s = 0.0;
#pragma unroll 8
                for (int i = 0; i < part.nI64; ++i) s += part.spart[((int64_t)i * P + pl) * Wld + w];
                zmv = (part.amp[pl] + part.noise[pl]) - s;
            }
        }
    }
    for (int p = 0; p < P; ++p) {
        // wave-uniform; extra_std == 0 on this path
        const double zm = part.mpart ? readlane_f64(zmv, p) : mean_pc[(int64_t)p * Wld + w];
        const double zv = part.mpart ? readlane_f64(zmv, 32 + p) : var_pc[(int64_t)p * Wld + w];
        const double ai = sA[p * 64 + lane];
        y = fma(zm, ai, y);                                       // dY_i (src/emulator.py:559-561, src/mcmc.py:288)
        const double t = zv * ai;
#pragma unroll
        for (int k = 0; k < MP; ++k) a[k] = fma(t, sA[p * 64 + k], a[k]);   // src/emulator.py:584-587
    }
    bool bad = false;
    double q = 0.0, prod = 1.0;
    double gprod = 1.0;                               // lane g keeps the product of pivot group g (4 pivots each)
#pragma unroll
    for (int j = 0; j < MP; ++j) {
        const double ajj = readlane_f64(a[j], j);
        bad = bad || !(ajj > 0.0);
        const double rinv = rsqrt(ajj);               // 1 / L_jj
        const double lj = a[j] * rinv;                // column j of L for the lanes i > j
        const double vj = readlane_f64(y, j) * rinv;  // forward solve: v_j
        q = fma(vj, vj, q);
        prod *= ajj;                                  // log det: sum log L_jj = 1/2 log prod a_jj, 4 pivots per log
        if ((j & 3) == 3) { gprod = (lane == (j >> 2)) ? prod : gprod; prod = 1.0; }
        y = fma(-lj, vj, y);                          // meaningful for lanes i > j
#pragma unroll
        for (int k = j + 1; k < MP; ++k) {
            const double lkj = readlane_f64(lj, k);
            a[k] = fma(-lj, lkj, a[k]);               // meaningful for lanes i >= k
            if (((k - j) & 7) == 0) __builtin_amdgcn_sched_barrier(0);   // keep the SGPR broadcasts from piling up
        }
    }
    const double glog = log(gprod);                   // the MP/4 logarithms in parallel, one per lane, off the chain
    double logdet = 0.0;
#pragma unroll
    for (int g = 0; g < MP / 4; ++g) logdet = fma(0.5, readlane_f64(glog, g), logdet);   // fixed order
    bool inside = true;
    if (box.X) {                                      // strict box over the d parameters, one per lane
        bool ok = true;
        for (int k0 = 0; k0 < box.d; k0 += 64) {
            const int k = k0 + lane;
            if (k < box.d) {
                const double x = box.X[w * box.d + k];
                ok = ok && (x > box.lo[k]) && (x < box.hi[k]);
            }
        }
        inside = __all(ok);
    }
    if (lane == 0 && (!box.cmp || w < box.cmp[0])) loglike_finish(box, w, q, logdet, bad, inside, accumulate, ll, notpd);
}

template <int MP>
static int launch_loglike_reg(gpb_ctx* ctx, int64_t W, double* ll_dev, bool accumulate, const BoxArgs& box,
                              const PartArgs& part) {
    const size_t sh = (64 * (MP + 1) + (size_t)ctx->P * 64) * sizeof(double);
    hipLaunchKernelGGL(k_loglike_reg<MP>, dim3((unsigned)((W + 3) / 4)), dim3(256), sh, ctx->stream, ctx->mean_pc,
                       ctx->var_pc, ctx->Wld, W, (int)ctx->P, (int)ctx->M, ctx->A, ctx->mu, ctx->C0, ctx->yexp,
                       ctx->Cexp, ll_dev, accumulate ? 1 : 0, ctx->notpd, box, part);
    GPB_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ fused block log-likelihood, one workgroup per walker
// Low-latency variant of k_loglike_reg<64> for small walker batches (a rank's shard under 8-way sharding):
// the one-wave kernel is a single dependent instruction stream of ~80 KB of straight-line code (larger than
// the instruction cache) and takes ~50 us however few walkers there are.  Here 256 threads share one
// walker: thread (ty, tx) owns the elements (ty + 16a, tx + 16b), a >= b, of the lower triangle in VGPRs
// (2-D cyclic, so all threads stay busy to the last column); per column the owners publish the column and
// y_j through a double-buffered LDS line, one barrier per column.  Every element sees exactly the same
// sequence of operations as in k_loglike_reg (same build order over p, same rsqrt, same fma operands, same
// grouping of the log-determinant), so the two kernels are bit-identical and the choice by batch size
// never changes a result.
__global__ __launch_bounds__(256) void k_loglike_wg(const double* __restrict__ mean_pc,
                                                    const double* __restrict__ var_pc, int64_t Wld, int64_t W, int P,
                                                    int M, const double* __restrict__ A,
                                                    const double* __restrict__ mu, const double* __restrict__ C0,
                                                    const double* __restrict__ yexp, const double* __restrict__ Cexp,
                                                    double* __restrict__ ll, int accumulate, int* __restrict__ notpd,
                                                    BoxArgs box, PartArgs part) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* sA = sm;                         // [P][64]  A, zero padded
    double* col = sm + (size_t)P * 64;       // [2][66]  column j of the trailing matrix (unscaled), y_j at [64]
    double* zl = col + 2 * 66;               // [2P]     fused finalize: mean, variance of GP p at [2p], [2p+1]
    __shared__ int s_outside;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t w = blockIdx.x;
    for (int e = tid; e < P * 64; e += 256) {
        const int p = e >> 6, i = e & 63;
        sA[e] = (i < M) ? A[p * M + i] : 0.0;
    }
    if (part.mpart) {                        // k_finalize's sums for this walker, same order; means on wave 0, variances on wave 1
        const int pl = tid & 63;
        if (tid < 64 && pl < P) {
            double m = 0.0;
#pragma unroll 8
            for (int c = 0; c < part.nchunk; ++c) m += part.mpart[((int64_t)c * P + pl) * Wld + w];
            zl[2 * pl] = m;
        } else if (tid >= 64 && tid < 128 && pl < P) {
            double s = 0.0;
#pragma unroll 8
            for (int i = 0; i < part.nI64; ++i) s += part.spart[((int64_t)i * P + pl) * Wld + w];
            zl[2 * pl + 1] = (part.amp[pl] + part.noise[pl]) - s;
        }
    }
    if (tid == 0) s_outside = 0;
    __syncthreads();
    if (box.X) {                             // strict box over the d parameters
        bool ok = true;
        for (int k = tid; k < box.d; k += 256) {
            const double x = box.X[w * box.d + k];
            ok = ok && (x > box.lo[k]) && (x < box.hi[k]);
        }
        if (!ok) s_outside = 1;              // all writers store the same value
    }
    double c[4][4];                          // c[a][b], b <= a: element (ty + 16a, tx + 16b)
    double y[4];                             // dY rows ty + 16a (meaningful on the tx == 0 threads)
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = ty + 16 * a;
        y[a] = (i < M) ? (mu[i] - yexp[i]) : 0.0;
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            const int k = tx + 16 * b;
            double v = (i == k) ? 1.0 : 0.0;
            if (i < M && k < M) v = C0[i * M + k] + Cexp[i * M + k];
            c[a][b] = v;
        }
    }
    for (int p = 0; p < P; ++p) {
        // uniform; extra_std == 0 on this path
        const double zm = part.mpart ? zl[2 * p] : mean_pc[(int64_t)p * Wld + w];
        const double zv = part.mpart ? zl[2 * p + 1] : var_pc[(int64_t)p * Wld + w];
        double ak[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) ak[b] = sA[p * 64 + tx + 16 * b];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double ai = sA[p * 64 + ty + 16 * a];
            y[a] = fma(zm, ai, y[a]);                             // dY_i (src/emulator.py:559-561, src/mcmc.py:288)
            const double t = zv * ai;
#pragma unroll
            for (int b = 0; b <= a; ++b) c[a][b] = fma(t, ak[b], c[a][b]);   // src/emulator.py:584-587
        }
    }
    bool bad = false;
    double q = 0.0, prod = 1.0;
    double gprod = 1.0;                      // thread g keeps the product of pivot group g (4 pivots each)
    const int nblk = (M + 15) >> 4;          // identity-padded columns beyond M change nothing (pivot 1, v = 0)
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
        if (jb < nblk) {
            for (int jj = 0; jj < 16; ++jj) {
                const int j = 16 * jb + jj;
                double* buf = col + (j & 1) * 66;
                if (tx == jj) {
#pragma unroll
                    for (int a = jb; a < 4; ++a) buf[ty + 16 * a] = c[a][jb];
                }
                if (tx == 0 && ty == jj) buf[64] = y[jb];
                __syncthreads();             // one barrier per column: the line of column j-1 is not rewritten before j+1
                const double ajj = buf[j];
                bad = bad || !(ajj > 0.0);
                const double rinv = rsqrt(ajj);                   // 1 / L_jj
                const double vj = buf[64] * rinv;                 // forward solve: v_j
                q = fma(vj, vj, q);
                prod *= ajj;                                      // sum log L_jj = 1/2 log prod a_jj, 4 pivots per log
                if ((j & 3) == 3) { gprod = (tid == (j >> 2)) ? prod : gprod; prod = 1.0; }
                double lk[4];
#pragma unroll
                for (int b = jb; b < 4; ++b) lk[b] = buf[tx + 16 * b] * rinv;
#pragma unroll
                for (int a = jb; a < 4; ++a) {
                    const double li = buf[ty + 16 * a] * rinv;    // L_ij for this thread's rows
                    y[a] = fma(-li, vj, y[a]);
#pragma unroll
                    for (int b = jb; b <= a; ++b) c[a][b] = fma(-li, lk[b], c[a][b]);
                }
            }
        }
    }
    __syncthreads();                         // the column lines are free: reuse them for the 16 group logarithms
    if (tid < 16) col[tid] = log(gprod);     // in parallel, off the factorisation's dependency chain
    __syncthreads();
    if (tid == 0) {
        double logdet = 0.0;
        for (int g = 0; g < 16; ++g) logdet = fma(0.5, col[g], logdet);      // fixed order (as k_loglike_reg)
        if (!box.cmp || w < box.cmp[0]) loglike_finish(box, w, q, logdet, bad, !s_outside, accumulate, ll, notpd);
    }
}

static int launch_loglike_wg(gpb_ctx* ctx, int64_t W, double* ll_dev, bool accumulate, const BoxArgs& box,
                             const PartArgs& part) {
    const size_t sh = ((size_t)ctx->P * 64 + 2 * 66 + 2 * (size_t)ctx->P) * sizeof(double);
    hipLaunchKernelGGL(k_loglike_wg, dim3((unsigned)W), dim3(256), sh, ctx->stream, ctx->mean_pc, ctx->var_pc,
                       ctx->Wld, W, (int)ctx->P, (int)ctx->M, ctx->A, ctx->mu, ctx->C0, ctx->yexp, ctx->Cexp, ll_dev,
                       accumulate ? 1 : 0, ctx->notpd, box, part);
    GPB_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ low-rank block log-likelihood, one lane per walker
// C_w = C0 + A^T diag(var_w) A with the same C0 for every walker (lowrank_setup.h has the algebra):
//     loglike_w = -1/2 (c_perp + v^T S^-1 v) - 1/2 (log det C0 + log det S),   S = I + R diag(var_w) R^T,  v = R m_w + v0
// a PP x PP Cholesky in one lane's registers instead of the M x M one (M = 64: 90 k flops and a 64-column
// dependency chain per walker; here ~1 k flops).  R is upper triangular, so row i of R touches p >= i only.
// Same conventions as the dense kernels: a non-positive pivot inside the box gives NaN and counts in notpd; the
// fused k_finalize sums (part) use k_finalize's order.
// k_finalize's sums for the 64 walkers of a workgroup, in its order (same bits): sum (GP p, mean or variance) is one chain of
// additions over the row chunks; the 2 P sums are dealt to the workgroup's eight waves, each with up to 32 partials in flight
// per round trip to L2.  (Four waves with 16 + 16 in flight walked three GPs x two round trips each: most of the kernel's
// 11 us at 256 walkers; with 8 of one kind a 64-walker workgroup spent 20 us waiting.)
// (13-16 GPs: the per-walker algebra needs more than the 256 registers an eight-wave workgroup leaves a wave: four waves)
template <int PP> constexpr int lr_threads() { return PP > 12 ? 256 : 512; }
template <int PP>
__device__ __forceinline__ void partial_sums(double (*smg)[PP][64], const double* __restrict__ mpart,
                                             const double* __restrict__ spart, const double* __restrict__ amp,
                                             const double* __restrict__ noise, int P, int nchunk, int nI64, int64_t Wld,
                                             int64_t w, int lane, int grp) {
    const int64_t st = (int64_t)P * Wld;
    for (int u = grp; u < 2 * P; u += lr_threads<PP>() / 64) {
        const int p = u >> 1, kind = u & 1;
        const double* src = (kind ? spart : mpart) + (int64_t)p * Wld + w;
        const int n = kind ? nI64 : nchunk;
        double a = 0.0;
        int c = 0;
        for (; c + 32 <= n; c += 32) {
            double v[32];
#pragma unroll
            for (int t = 0; t < 32; ++t) v[t] = src[(c + t) * st];
#pragma unroll
            for (int t = 0; t < 32; ++t) a += v[t];
        }
        for (; c + 8 <= n; c += 8) {
            double v[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = src[(c + t) * st];
#pragma unroll
            for (int t = 0; t < 8; ++t) a += v[t];
        }
        for (; c < n; ++c) a += src[c * st];
        smg[kind][p][lane] = kind ? (amp[p] + noise[p]) - a : a;
    }
}

template <int PP>
__global__ __launch_bounds__(lr_threads<PP>()) void k_loglike_lowrank(const double* __restrict__ mean_pc,
                                                        const double* __restrict__ var_pc, int64_t Wld, int64_t W,
                                                        int P, const double* __restrict__ Rg,
                                                        const double* __restrict__ v0g, double cperp, double logdet0,
                                                        double* __restrict__ ll, int accumulate,
                                                        int* __restrict__ notpd, BoxArgs box, PartArgs part) {
    // 256 threads serve 64 walkers: the four waves share the fused k_finalize sums (wave q: GPs q, q+4, ...; the
    // loads are coalesced along the walkers), wave 0 then does the per-walker algebra.
    __shared__ double sR[PP][PP + 1];
    __shared__ double sv0[PP];
    __shared__ double smg[2][PP][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < PP * PP; e += lr_threads<PP>()) sR[e / PP][e % PP] = Rg[(e / PP) * 16 + (e % PP)];
    if (threadIdx.x < PP) sv0[threadIdx.x] = v0g[threadIdx.x];
    const int64_t w = (int64_t)blockIdx.x * 64 + lane;
    if (part.mpart && w < W && (!box.cmp || w < box.cmp[0]))
        partial_sums<PP>(smg, part.mpart, part.spart, part.amp, part.noise, P, part.nchunk, part.nI64, Wld, w, lane, grp);
    __syncthreads();
    if (grp != 0 || w >= W || (box.cmp && w >= box.cmp[0])) return;
    const int64_t wo = box.cmp ? box.cmp[4 + w] : w;
    double m[PP], g[PP];
#pragma unroll
    for (int p = 0; p < PP; ++p) {
        m[p] = 0.0; g[p] = 0.0;
        if (p < P) {
            if (part.mpart) {
                m[p] = smg[0][p][lane];
                g[p] = smg[1][p][lane];
            } else {
                m[p] = mean_pc[(int64_t)p * Wld + w];
                g[p] = var_pc[(int64_t)p * Wld + w];
            }
        }
    }
    bool inside = true;
    if (box.X) {
        for (int k = 0; k < box.d; ++k) {
            const double x = box.X[w * box.d + k];
            inside = inside && (x > box.lo[k]) && (x < box.hi[k]);
        }
    }
    // S (lower triangle, registers) and v
    double S[PP][PP], v[PP];
#pragma unroll
    for (int i = 0; i < PP; ++i) {
        double vi = sv0[i];
#pragma unroll
        for (int p = i; p < PP; ++p) vi = fma(sR[i][p], m[p], vi);
        v[i] = vi;
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double sij = (i == j) ? 1.0 : 0.0;
#pragma unroll
            for (int p = i; p < PP; ++p) sij = fma(sR[i][p] * g[p], sR[j][p], sij);
            S[i][j] = sij;
        }
    }
    // Cholesky + forward solve, column by column
    // log det S = sum of log pivots, four pivots per logarithm like the dense kernels (S >= I, so the pivots are >= 1
    // and a product cannot underflow; four of them overflow only beyond 1e77 each, i.e. never for a C0 that factorises
    // in fp64, whereas all PP <= 16 in one product overflowed from 1e19 per pivot: C0 ~ 1e-20 * I)
    double q = 0.0, prod = 1.0, logsum = 0.0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < PP; ++j) {
        const double ajj = S[j][j];
        bad = bad || !(ajj > 0.0);
        const double rinv = rsqrt(ajj);
        const double zj = v[j] * rinv;
        q = fma(zj, zj, q);
        prod *= ajj;
        if ((j & 3) == 3 || j == PP - 1) { logsum += log(prod); prod = 1.0; }
#pragma unroll
        for (int i = j + 1; i < PP; ++i) {
            const double lij = S[i][j] * rinv;
            v[i] = fma(-lij, zj, v[i]);
#pragma unroll
            for (int k = j + 1; k <= i; ++k) S[i][k] = fma(-lij, S[k][j] * rinv, S[i][k]);
        }
    }
    double r = -0.5 * (cperp + q) - 0.5 * (logdet0 + logsum);
    bad = bad || !(logsum < INFINITY);       // an overflowing pivot product is a failure, not a silent -inf
    // loglike_finish, written out: through the helper the forms of 11 GPs and more take up to 82 more registers and the one
    // of 13 GPs loses a wave per SIMD (the scatter index wo has to be loaded up here, ahead of the algebra)
    if (bad && inside) {
        r = nan("");
        atomicAdd(notpd, 1);
    }
    r = accumulate ? (ll[wo] + r) : r;
    if (box.X) r = inside ? (r + box.inside_const) : box.outside;
    else if (box.cmp) r += box.inside_const;
    ll[wo] = r;
}

static bool lowrank_applies(const gpb_ctx* ctx) {
    return ctx->lowrank && ctx->lr_ok && ctx->mode == GPB_MODE_PCA && ctx->P <= 16 && !ctx->force_generic_mvn;
}

static int launch_loglike_lowrank(gpb_ctx* ctx, int64_t W, double* ll_dev, bool accumulate, const BoxArgs& box,
                                  const PartArgs& part) {
    const dim3 grid((unsigned)((W + 63) / 64));
    // exact sizes: the work per walker grows with PP^3
    const int rc = with_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(ctx->P, [&](auto N) {
        constexpr int PP = decltype(N)::value;
        hipLaunchKernelGGL(k_loglike_lowrank<PP>, grid, dim3(lr_threads<PP>()), 0, ctx->stream, ctx->mean_pc, ctx->var_pc, ctx->Wld,
                           W, (int)ctx->P, ctx->lr_R, ctx->lr_v0, ctx->lr_cperp, ctx->lr_logdet0, ll_dev, accumulate ? 1 : 0,
                           ctx->notpd, box, part);
        return 0;
    });
    if (rc) return dispatched(ctx, rc, "k_loglike_lowrank");
    GPB_HIP(hipGetLastError());
    return 0;
}

// ---- the low-rank block log-likelihoods of ALL emulators of a chain in one launch (round 3) --------------------------------
// gpb_chain_logpost / gpb_chain_emcee_run end a batch with one k_loglike_lowrank per emulator, each adding its block onto the
// row's log-probability: 32 workgroups (2048 rows) of latency-bound work per launch, nine launches in a row for the
// reference's nine emulators.  Here a workgroup walks the emulators itself, in emuList order — the same sequence of
// additions per row as the separate launches.  PP = the largest number of GPs of any emulator of the chain (rounded up to a
// multiple of 4); an emulator with fewer runs with identity padding: its R and v0 are zero beyond P (lr_R / lr_v0 are zero
// padded), so the padded rows of S are unit rows, their pivots 1, their v 0 — every product, sum and logarithm of the exact-size
// kernel is reproduced bit for bit (x * 1 = x, x + 0 = x, log 1 = 0; the groups of four pivots per logarithm start at the same
// places).  Compacted batches only (the chain calls): rows w >= cmp[0] do not exist.
constexpr int MAX_LR_CTX = 24;
struct LrCtx {
    const double *mpart, *spart, *amp, *noise, *R, *v0;
    int* notpd;
    double cperp, logdet0;
    int P, nchunk, nI64;
};
struct LrTable { LrCtx c[MAX_LR_CTX]; int E; };

// Round 5: with `blocks` set the grid is (walker tiles, emulators): workgroup (t, e) computes emulator e's block alone and leaves
// it in blocks[e][w]; k_lowrank_sum then adds a row's blocks in emuList order — the same additions as the walk below, which ran
// nine latency-bound bodies one after the other in each of only W / 64 workgroups (57 us for nine emulators at 2048 rows).
template <int PP>
__global__ __launch_bounds__(lr_threads<PP>()) void k_loglike_lowrank_multi(const LrTable tab, int64_t Wld, int64_t W,
                                                              double* __restrict__ ll, const int* __restrict__ cmp,
                                                              double inside_const, double* __restrict__ blocks) {
    __shared__ double sR[PP][PP + 1];
    __shared__ double sv0[PP];
    __shared__ double smg[2][PP][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * 64 + lane;
    const bool live = w < W && w < cmp[0];
    double total = 0.0;
    const int e_begin = blocks ? (int)blockIdx.y : 0, e_end = blocks ? (int)blockIdx.y + 1 : tab.E;
    for (int e = e_begin; e < e_end; ++e) {
        const LrCtx& c = tab.c[e];
        const int P = c.P;
        if (e > e_begin) __syncthreads();              // wave 0 is done with the previous emulator's tables
        for (int i = threadIdx.x; i < PP * PP; i += lr_threads<PP>()) sR[i / PP][i % PP] = c.R[(i / PP) * 16 + (i % PP)];
        if (threadIdx.x < PP) sv0[threadIdx.x] = c.v0[threadIdx.x];
        if (live)                                      // k_finalize's sums, in its order (as k_loglike_lowrank)
            partial_sums<PP>(smg, c.mpart, c.spart, c.amp, c.noise, P, c.nchunk, c.nI64, Wld, w, lane, grp);
        __syncthreads();
        if (grp != 0 || !live) continue;               // (uniform per wave; every wave still reaches the barriers above)
        // From here to `bad` a copy of k_loglike_lowrank's algebra on purpose: a shared force-inlined body made every form
        // spill (up to 1.7 KB of scratch at 16 GPs).
        double m[PP], g[PP];
#pragma unroll
        for (int p = 0; p < PP; ++p) {
            m[p] = 0.0; g[p] = 0.0;
            if (p < P) { m[p] = smg[0][p][lane]; g[p] = smg[1][p][lane]; }
        }
        double S[PP][PP], v[PP];
#pragma unroll
        for (int i = 0; i < PP; ++i) {
            double vi = sv0[i];
#pragma unroll
            for (int p = i; p < PP; ++p) vi = fma(sR[i][p], m[p], vi);
            v[i] = vi;
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double sij = (i == j) ? 1.0 : 0.0;
#pragma unroll
                for (int p = i; p < PP; ++p) sij = fma(sR[i][p] * g[p], sR[j][p], sij);
                S[i][j] = sij;
            }
        }
        double q = 0.0, prod = 1.0, logsum = 0.0;
        bool bad = false;
#pragma unroll
        for (int j = 0; j < PP; ++j) {
            const double ajj = S[j][j];
            bad = bad || !(ajj > 0.0);
            const double rinv = rsqrt(ajj);
            const double zj = v[j] * rinv;
            q = fma(zj, zj, q);
            prod *= ajj;
            if ((j & 3) == 3 || j == PP - 1) { logsum += log(prod); prod = 1.0; }
#pragma unroll
            for (int i = j + 1; i < PP; ++i) {
                const double lij = S[i][j] * rinv;
                v[i] = fma(-lij, zj, v[i]);
#pragma unroll
                for (int k = j + 1; k <= i; ++k) S[i][k] = fma(-lij, S[k][j] * rinv, S[i][k]);
            }
        }
        double r = -0.5 * (c.cperp + q) - 0.5 * (c.logdet0 + logsum);
        bad = bad || !(logsum < INFINITY);
        if (bad) {
            r = nan("");
            atomicAdd(c.notpd, 1);
        }
        if (blocks) { blocks[(int64_t)e * Wld + w] = r; return; }      // (grp 0, live: the ordered sum follows in k_lowrank_sum)
        total = e ? (total + r) : r;                   // ll = r0; ll = ll + r1; ... as the separate launches accumulate
    }
    if (grp == 0 && live && !blocks) ll[cmp[4 + w]] = total + inside_const;
}

// a row's log-likelihood = its emulators' blocks added in emuList order (ll = r0; ll = ll + r1; ...), + the constant
__global__ __launch_bounds__(256) void k_lowrank_sum(const double* __restrict__ blocks, int E, int64_t Wld, int64_t W,
                                                     double* __restrict__ ll, const int* __restrict__ cmp, double inside_const) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= W || w >= cmp[0]) return;
    double total = blocks[w];
    for (int e = 1; e < E; ++e) total = total + blocks[(int64_t)e * Wld + w];
    ll[cmp[4 + w]] = total + inside_const;
}

// the per-emulator blocks of a chain's log-likelihood, [E][Wcap] in the chain's first context (k_loglike_lowrank_multi / k_lowrank_sum)
int ensure_lr_blocks(gpb_ctx* ctx, int E) {
    if (E < 2 || !ctx->lr_split) return 0;
    return ctx_grow(ctx, ctx->lr_blocks, (int64_t)E * ctx->Wcap);
}

// The block log-likelihoods of a chain's compacted batch, added up in emuList order, when every block takes the low-rank
// kernel: one launch that walks the emulators (or one workgroup per (walker tile, emulator) and the ordered sum).  *taken =
// false: not this chain, nothing was launched, and the caller runs one launch_loglike per emulator.
int launch_loglike_lowrank_chain(gpb_ctx* const* ctxs, int E, int64_t W, double* ll_dev, const int* cmpv, double inside_const,
                                 bool* taken) {
    gpb_ctx* ctx = ctxs[0];
    *taken = ctx->chain_batch && E > 1 && E <= MAX_LR_CTX;
    int64_t pmax = 0;
    for (int e = 0; e < E && *taken; ++e) {
        *taken = lowrank_applies(ctxs[e]) && ctxs[e]->fuse_finalize && ctxs[e]->Wld == ctx->Wld;
        pmax = ctxs[e]->P > pmax ? ctxs[e]->P : pmax;
    }
    if (!*taken) return 0;
    LrTable tab;
    for (int e = 0; e < E; ++e) {
        const gpb_ctx* c = ctxs[e];
        tab.c[e] = LrCtx{c->mpart, c->spart, c->amp, c->noise, c->lr_R, c->lr_v0, c->notpd, c->lr_cperp, c->lr_logdet0,
                         (int)c->P, (int)((c->Np + KX_CHUNK - 1) / KX_CHUNK), (int)(c->Np / 64)};
    }
    tab.E = E;
    // one workgroup per (walker tile, emulator) + the ordered sum, when the blocks' buffer is there (ensure_lr_blocks;
    // option key 49 = 0: the one-launch walk — the A/B, and the bit-identity test)
    double* blocks = (ctx->lr_split && ctx->lr_blocks.cap >= (int64_t)E * ctx->Wld) ? ctx->lr_blocks : nullptr;
    const dim3 grid((unsigned)((W + 63) / 64), blocks ? (unsigned)E : 1u);
    const int rc = with_int<4, 8, 12, 16>(round_up(pmax, 4), [&](auto N) {
        constexpr int PP = decltype(N)::value;
        hipLaunchKernelGGL(k_loglike_lowrank_multi<PP>, grid, dim3(lr_threads<PP>()), 0, ctx->stream, tab, ctx->Wld, W, ll_dev, cmpv,
                           inside_const, blocks);
        return 0;
    });
    if (rc) return dispatched(ctx, rc, "k_loglike_lowrank_multi");
    if (blocks)
        hipLaunchKernelGGL(k_lowrank_sum, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, ctx->stream, blocks, E, ctx->Wld, W,
                           ll_dev, cmpv, inside_const);
    if (hipGetLastError() != hipSuccess) GPB_FAIL(GPB_E_HIP, "gpb: k_loglike_lowrank_multi launch failed");
    return 0;
}

// ---- rows that belong to DIFFERENT data sets (a closure study: K ensembles, one per pseudo-experiment) ----------------------
// The data enter the low-rank form through v0 and c_perp alone (lowrank_setup.h); R, log det C0 and the whole per-row S do
// not depend on them.  k_loglike_lowrank_multi with a row's own v0[set][.] and cperp[set] from the tables of
// gpb_chain_like_sets: set = (the row's ORIGINAL index, cmp[4 + w]) / rows_per_set.  The rows of a 64-row tile belong to
// arbitrary sets (the gather order is arbitrary), so v0 is no per-workgroup vector: all waves stage the tile's 64 vectors in
// LDS (sv0[i][lane], read back like smg: an LDS read where the twin has one, no table value is held in a register across
// the algebra; all four forms build with zero scratch).  Given the same v0 every operation is the one the single-set kernels
// do, in their order, so a row of set k gets the bits of gpb_chain_logpost with data set k installed; an emulator with fewer
// than PP GPs runs with identity padding as in k_loglike_lowrank_multi (the tables are zero beyond P like lr_v0), which
// also serves E = 1 (k_loglike_lowrank<P>: same products, sums and logarithms).
struct LrSets {
    const double* v0[MAX_LR_CTX];      // [K][16] per emulator
    const double* cperp[MAX_LR_CTX];   // [K]
    int rows_per_set, K;
};

template <int PP>
__global__ __launch_bounds__(lr_threads<PP>()) void k_loglike_lowrank_sets(const LrTable tab, const LrSets sets, int64_t Wld,
                                                             int64_t W, double* __restrict__ ll,
                                                             const int* __restrict__ cmp, double inside_const,
                                                             double* __restrict__ blocks) {
    __shared__ double sR[PP][PP + 1];
    __shared__ double sv0[PP][64];
    __shared__ double smg[2][PP][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * 64 + lane;
    const bool live = w < W && w < cmp[0];
    // the set of this lane's row; a set index beyond the tables cannot happen (the host checks W / rows_per_set <= K): min
    // keeps the read inside them whatever the index list holds
    const int set = live ? max(min(cmp[4 + w] / sets.rows_per_set, sets.K - 1), 0) : 0;
    double total = 0.0;
    const int e_begin = blocks ? (int)blockIdx.y : 0, e_end = blocks ? (int)blockIdx.y + 1 : tab.E;
    for (int e = e_begin; e < e_end; ++e) {
        const LrCtx& c = tab.c[e];
        const int P = c.P;
        if (e > e_begin) __syncthreads();              // wave 0 is done with the previous emulator's tables
        for (int i = threadIdx.x; i < PP * PP; i += lr_threads<PP>()) sR[i / PP][i % PP] = c.R[(i / PP) * 16 + (i % PP)];
        if (live) {
            const double* v0s = sets.v0[e] + (int64_t)set * 16;
            for (int i = grp; i < PP; i += lr_threads<PP>() / 64) sv0[i][lane] = v0s[i];
            partial_sums<PP>(smg, c.mpart, c.spart, c.amp, c.noise, P, c.nchunk, c.nI64, Wld, w, lane, grp);
        }
        __syncthreads();
        if (grp != 0 || !live) continue;               // (uniform per wave; every wave still reaches the barriers above)
        // From here to `bad` a copy of k_loglike_lowrank's algebra on purpose (see k_loglike_lowrank_multi)
        double m[PP], g[PP];
#pragma unroll
        for (int p = 0; p < PP; ++p) {
            m[p] = 0.0; g[p] = 0.0;
            if (p < P) { m[p] = smg[0][p][lane]; g[p] = smg[1][p][lane]; }
        }
        double S[PP][PP], v[PP];
#pragma unroll
        for (int i = 0; i < PP; ++i) {
            double vi = sv0[i][lane];
#pragma unroll
            for (int p = i; p < PP; ++p) vi = fma(sR[i][p], m[p], vi);
            v[i] = vi;
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double sij = (i == j) ? 1.0 : 0.0;
#pragma unroll
                for (int p = i; p < PP; ++p) sij = fma(sR[i][p] * g[p], sR[j][p], sij);
                S[i][j] = sij;
            }
        }
        double q = 0.0, prod = 1.0, logsum = 0.0;
        bool bad = false;
#pragma unroll
        for (int j = 0; j < PP; ++j) {
            const double ajj = S[j][j];
            bad = bad || !(ajj > 0.0);
            const double rinv = rsqrt(ajj);
            const double zj = v[j] * rinv;
            q = fma(zj, zj, q);
            prod *= ajj;
            if ((j & 3) == 3 || j == PP - 1) { logsum += log(prod); prod = 1.0; }
#pragma unroll
            for (int i = j + 1; i < PP; ++i) {
                const double lij = S[i][j] * rinv;
                v[i] = fma(-lij, zj, v[i]);
#pragma unroll
                for (int k = j + 1; k <= i; ++k) S[i][k] = fma(-lij, S[k][j] * rinv, S[i][k]);
            }
        }
        double r = -0.5 * (sets.cperp[e][set] + q) - 0.5 * (c.logdet0 + logsum);
        bad = bad || !(logsum < INFINITY);
        if (bad) {
            r = nan("");
            atomicAdd(c.notpd, 1);
        }
        if (blocks) { blocks[(int64_t)e * Wld + w] = r; return; }      // (grp 0, live: the ordered sum follows in k_lowrank_sum)
        total = e ? (total + r) : r;                   // ll = r0; ll = ll + r1; ... as the separate launches accumulate
    }
    if (grp == 0 && live && !blocks) ll[cmp[4 + w]] = total + inside_const;
}

int lowrank_sets_check(gpb_ctx* const* ctxs, int E, const char* who) {
    gpb_ctx* ctx = ctxs[0];
    if (coupling_installed(ctx))
        GPB_FAIL(GPB_E_STATE, std::string(who) + ": a coupled chain likelihood is installed (per-set tables are those of the "
                                                 "emulators' own blocks)");
    if (E > MAX_LR_CTX) GPB_FAIL(GPB_E_STATE, std::string(who) + ": more than 24 emulators");
    for (int e = 0; e < E; ++e)
        if (!lowrank_applies(ctxs[e]) || !ctxs[e]->fuse_finalize || !ctxs[e]->lr_fac.ok)
            GPB_FAIL(GPB_E_STATE, std::string(who) + ": needs the low-rank likelihood kernel with its fused sums for every "
                                                     "emulator (PCA mode, at most 16 GPs, C0 positive definite, option "
                                                     "keys 11, 23 and 43 at their defaults)");
    return 0;
}

int launch_loglike_lowrank_sets(gpb_ctx* const* ctxs, int E, int64_t W, int64_t rows_per_set, double* ll_dev, const int* cmpv,
                                double inside_const) {
    gpb_ctx* ctx = ctxs[0];
    LrTable tab;
    LrSets sets;
    int64_t pmax = 0;
    for (int e = 0; e < E; ++e) {
        const gpb_ctx* c = ctxs[e];
        if (c->Wld != ctx->Wld || c->lrs_K != ctx->lrs_K || c->lrs_K < 1)
            GPB_FAIL(GPB_E_STATE, "gpb: internal: the emulators of a data-set batch disagree on its workspaces or tables");
        pmax = c->P > pmax ? c->P : pmax;
        tab.c[e] = LrCtx{c->mpart, c->spart, c->amp, c->noise, c->lr_R, c->lr_v0, c->notpd, c->lr_cperp, c->lr_logdet0,
                         (int)c->P, (int)((c->Np + KX_CHUNK - 1) / KX_CHUNK), (int)(c->Np / 64)};
        sets.v0[e] = c->lrs_v0;
        sets.cperp[e] = c->lrs_cperp;
    }
    tab.E = E;
    sets.rows_per_set = (int)rows_per_set;
    sets.K = (int)ctx->lrs_K;
    if (rows_per_set < 1 || rows_per_set >= (1ll << 31) || (W + rows_per_set - 1) / rows_per_set > ctx->lrs_K)
        GPB_FAIL(GPB_E_STATE, "gpb: internal: a data-set batch beyond the tables");
    double* blocks = (E > 1 && ctx->lr_split && ctx->lr_blocks.cap >= (int64_t)E * ctx->Wld) ? ctx->lr_blocks : nullptr;
    const dim3 grid((unsigned)((W + 63) / 64), blocks ? (unsigned)E : 1u);
    const int rc = with_int<4, 8, 12, 16>(round_up(pmax, 4), [&](auto N) {
        constexpr int PP = decltype(N)::value;
        hipLaunchKernelGGL(k_loglike_lowrank_sets<PP>, grid, dim3(lr_threads<PP>()), 0, ctx->stream, tab, sets, ctx->Wld, W, ll_dev,
                           cmpv, inside_const, blocks);
        return 0;
    });
    if (rc) return dispatched(ctx, rc, "k_loglike_lowrank_sets");
    if (blocks)
        hipLaunchKernelGGL(k_lowrank_sum, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, ctx->stream, blocks, E, ctx->Wld, W,
                           ll_dev, cmpv, inside_const);
    if (hipGetLastError() != hipSuccess) GPB_FAIL(GPB_E_HIP, "gpb: k_loglike_lowrank_sets launch failed");
    return 0;
}

// ------------------------------------------------------------------ prior box
__global__ void k_box(const double* __restrict__ X, int64_t W, int d, const double* __restrict__ lo,
                      const double* __restrict__ hi, double outside, double inside_const,
                      double* __restrict__ ll) {
    const int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (w >= W) return;
    bool in = true;
    for (int k = 0; k < d; ++k) {
        const double x = X[w * d + k];
        in = in && (x > lo[k]) && (x < hi[k]);      // strict (src/mcmc.py:275)
    }
    ll[w] = in ? (ll[w] + inside_const) : outside;
}

static bool block_kernels_apply(const gpb_ctx* ctx) {
    return ctx->mode == GPB_MODE_PCA && ctx->M <= 64 && ctx->P <= 96 && !ctx->force_generic_mvn;
}

// Small batches only: there the saved launch and dependent pass matter (a rank's shard), while at thousands of
// walkers the per-walker strided reads of the partials cost more than the coalesced k_finalize they replace
// (measured: +25 us on k_loglike_reg<64> at 2048 walkers against a 6.6 us kernel).
bool loglike_fuses_finalize(const gpb_ctx* ctx, int64_t W) {
    if (lowrank_applies(ctx)) return ctx->fuse_finalize != 0;     // the kernel's four waves share k_finalize's sums
    return block_kernels_apply(ctx) && ctx->P <= 32 && ctx->fuse_finalize && W <= ctx->mvn_wg_switch;
}

// Where the generic kernels keep a walker's augmented (M + 1) x (M + 1) matrix: in LDS behind the `small` bytes of their
// vectors, or (M > ~135) in a slab of ctx->mvn_ws, grown here.  Out: gws (null: LDS) and the dynamic LDS bytes sh.
static int mvn_storage(gpb_ctx* ctx, int64_t W, int64_t M, size_t small, double** gws, size_t* sh) {
    *gws = nullptr;
    *sh = small + (size_t)(M + 1) * (M + 1) * sizeof(double);
    if (*sh <= 150 * 1024) return 0;
    int rc = ctx_grow(ctx, ctx->mvn_ws, W * (M + 1) * (M + 1));
    if (rc) return rc;
    *gws = ctx->mvn_ws;
    *sh = small;
    return 0;
}

// box_* optional (X_box == nullptr: no prior box).  The register-resident kernel applies the box itself;
// the generic kernels are followed by k_box.
int launch_loglike(gpb_ctx* ctx, int64_t W, double* ll_dev, bool accumulate, bool from_partials, const double* X_box,
                   const double* lo_dev, const double* hi_dev, double outside, double inside_const, const int* cmp_dev) {
    const int64_t M = ctx->M, P = ctx->P;
    const BoxArgs box{X_box, lo_dev, hi_dev, (int)ctx->d, outside, inside_const, cmp_dev};
    if (cmp_dev && !(lowrank_applies(ctx) || block_kernels_apply(ctx)))
        GPB_FAIL(GPB_E_STATE, "gpb: internal: compacted batch without a block likelihood kernel");
    if (from_partials && !loglike_fuses_finalize(ctx, W)) GPB_FAIL(GPB_E_STATE, "gpb: internal: partials without a fused consumer");
    if (lowrank_applies(ctx) || block_kernels_apply(ctx)) {
        PartArgs part{nullptr, nullptr, nullptr, nullptr, 0, 0};
        if (from_partials)
            part = PartArgs{ctx->mpart, ctx->spart, ctx->amp, ctx->noise,
                            (int)((ctx->Np + KX_CHUNK - 1) / KX_CHUNK), (int)(ctx->Np / 64)};
        if (lowrank_applies(ctx)) return launch_loglike_lowrank(ctx, W, ll_dev, accumulate, box, part);
        if (M <= 8) return launch_loglike_reg<8>(ctx, W, ll_dev, accumulate, box, part);
        if (M <= 16) return launch_loglike_reg<16>(ctx, W, ll_dev, accumulate, box, part);
        if (M <= 32) return launch_loglike_reg<32>(ctx, W, ll_dev, accumulate, box, part);
        if (W <= ctx->mvn_wg_switch) return launch_loglike_wg(ctx, W, ll_dev, accumulate, box, part);   // same bits, lower latency
        return launch_loglike_reg<64>(ctx, W, ll_dev, accumulate, box, part);
    }
    double* gws;
    size_t sh;
    int rc = mvn_storage(ctx, W, M, (2 * P + 2 * M) * sizeof(double), &gws, &sh);
    if (rc) return rc;
    if (sh > 64 * 1024) {
        GPB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_loglike<false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    }
    if (gws)
        hipLaunchKernelGGL(k_loglike<true>, dim3((unsigned)W), dim3(256), sh, ctx->stream, ctx->mean_pc, ctx->var_pc,
                           ctx->Wld, (int)P, (int)M, ctx->mode, ctx->A, ctx->mu, ctx->scale, ctx->C0, ctx->yexp,
                           ctx->Cexp, gws, ll_dev, accumulate ? 1 : 0, ctx->notpd);
    else
        hipLaunchKernelGGL(k_loglike<false>, dim3((unsigned)W), dim3(256), sh, ctx->stream, ctx->mean_pc, ctx->var_pc,
                           ctx->Wld, (int)P, (int)M, ctx->mode, ctx->A, ctx->mu, ctx->scale, ctx->C0, ctx->yexp,
                           ctx->Cexp, gws, ll_dev, accumulate ? 1 : 0, ctx->notpd);
    if (X_box)
        hipLaunchKernelGGL(k_box, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, ctx->stream, X_box, W, (int)ctx->d,
                           lo_dev, hi_dev, outside, inside_const, ll_dev);
    GPB_HIP(hipGetLastError());
    return 0;
}

int launch_mvn(gpb_ctx* ctx, const double* dY_dev, const double* cov_dev, int64_t W, int64_t M, double* ll_dev) {
    double* gws;
    size_t sh;
    int rc = mvn_storage(ctx, W, M, M * sizeof(double), &gws, &sh);
    if (rc) return rc;
    if (sh > 64 * 1024) {
        GPB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_mvn<false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    }
    if (gws)
        hipLaunchKernelGGL(k_mvn<true>, dim3((unsigned)W), dim3(256), sh, ctx->stream, dY_dev, cov_dev, (int)M, gws,
                           ll_dev, ctx->notpd);
    else
        hipLaunchKernelGGL(k_mvn<false>, dim3((unsigned)W), dim3(256), sh, ctx->stream, dY_dev, cov_dev, (int)M, gws,
                           ll_dev, ctx->notpd);
    GPB_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ compaction to the rows inside the prior box
// The reference evaluates the emulators for the rows inside the box only (src/mcmc.py:194-203, 275-283) and an
// all-outside batch costs it nothing (:278-279).  Here: ONE workgroup marks the rows (strict inequalities), writes
// `outside` for those outside, and gathers the others — in order — into Xc with their indices and count in cmp
// ([0] = count, [4..] = indices).  The count stays on the device: the kernels that follow are launched for the whole
// batch and those of their workgroups that find no row leave at once.  From uniform starting positions more than half of
// a stretch move's proposals (z > 1) leave a 20-dimensional box; a burnt-in ensemble hardly ever does.
// Pass 1: 256 rows per workgroup, staged through LDS with coalesced loads (a lane reading its own row touches 64
// different cache lines per instruction).  rank[w] = position of row w among the live rows of its workgroup (-1: outside),
// blockcnt[b] = live rows of workgroup b.
__global__ __launch_bounds__(256) void k_compact_mark(const double* __restrict__ X, int64_t W, int d,
                                                      const double* __restrict__ lo, const double* __restrict__ hi,
                                                      double outside, double* __restrict__ ll, int* __restrict__ rank,
                                                      int* __restrict__ blockcnt) {
    extern __shared__ double srow[];                   // [256][dt + 1], dt = min(d, 64): the columns go through in tiles
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dt = d < 64 ? d : 64, ldr = dt + 1;
    const int64_t w0 = (int64_t)blockIdx.x * 256, nrow = imin64(256, W - w0);
    const bool have = tid < nrow;
    int ok = have ? 1 : 0;
    for (int k0 = 0; k0 < d; k0 += dt) {
        const int kn = (d - k0 < dt) ? d - k0 : dt;
        if (k0) __syncthreads();
        for (int64_t e = tid; e < nrow * kn; e += 256) srow[(e / kn) * ldr + (e % kn)] = X[(w0 + e / kn) * d + k0 + (e % kn)];
        __syncthreads();
        if (have)
            for (int k = 0; k < kn; ++k) {
                const double x = srow[tid * ldr + k];
                ok &= (int)(x > lo[k0 + k]) & (int)(x < hi[k0 + k]);      // strict (src/mcmc.py:275); no short circuit
            }
    }
    const bool in = ok != 0;
    if (have && !in) ll[w0 + tid] = outside;
    const unsigned long long m = __ballot(in);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = 0;
    for (int i = 0; i < wave; ++i) off += wsum[i];
    if (have) rank[w0 + tid] = in ? off + __popcll(m & ((1ull << lane) - 1ull)) : -1;
    if (tid == 0) blockcnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Pass 2: the live rows of workgroup b go to slots base_b + rank, base_b = live rows of the workgroups before it (the
// order of the rows is kept); cmp[0] = total, cmp[4 + slot] = row.
__global__ __launch_bounds__(256) void k_compact_gather(const double* __restrict__ X, int64_t W, int d,
                                                        const int* __restrict__ rank, const int* __restrict__ blockcnt,
                                                        double* __restrict__ Xc, int* __restrict__ cmp,
                                                        unsigned long long* __restrict__ rows_live,
                                                        unsigned long long* __restrict__ hint) {
    __shared__ int s_base, s_cnt;
    __shared__ int row_of[256];
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * 256, nrow = imin64(256, W - w0);
    int r;
    if (blockcnt) {
        if (tid < 64) {                                // fixed-order sum of the counts before this workgroup
            int s = 0;
            for (int b = lane; b < (int)blockIdx.x; b += 64) s += blockcnt[b];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) { s_base = s; s_cnt = blockcnt[blockIdx.x]; }
        }
        r = tid < nrow ? rank[w0 + tid] : -1;
    } else {
        // rank[] holds 0/1 flags (written by k_propose; batches of a few thousand rows): the live rows before this
        // workgroup are counted from the flags themselves (integers: any order), the rank inside it by ballots
        int s = 0;
        for (int64_t w = tid; w < w0; w += 256) s += rank[w];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const bool in = tid < nrow && rank[w0 + tid] != 0;
        const unsigned long long m = __ballot(in);
        __syncthreads();                               // (wsum is free: first use)
        if (lane == 0) { wsum[wave] = __popcll(m); row_of[wave] = s; }     // row_of[0..3] borrowed for the partial sums
        __syncthreads();
        int off = 0;
        for (int i = 0; i < wave; ++i) off += wsum[i];
        r = in ? off + __popcll(m & ((1ull << lane) - 1ull)) : -1;
        const int b4 = row_of[0] + row_of[1] + row_of[2] + row_of[3], c4 = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();                               // everyone has read row_of[0..3] before it is reused below
        if (tid == 0) { s_base = b4; s_cnt = c4; }
    }
    if (r >= 0) row_of[r] = tid;
    __syncthreads();
    const int base = s_base, cnt = s_cnt;
    if (r >= 0) cmp[4 + base + r] = (int)(w0 + tid);
    for (int64_t e = tid; e < (int64_t)cnt * d; e += 256) {
        const int s = (int)(e / d), k = (int)(e % d);
        Xc[((int64_t)base + s) * d + k] = X[(w0 + row_of[s]) * d + k];
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        cmp[0] = base + cnt;
        if (hint) __hip_atomic_store(hint, ((unsigned long long)W << 32) | (unsigned long long)(base + cnt), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_SYSTEM);        // for the host's tile-shape rule, read without a sync
        if (rows_live) atomicAdd(rows_live, (unsigned long long)(base + cnt));
    }
}

// X_dev [W][dx]: dx = the chain's number of parameters (the GP's d unless the emulator has a parameter map).  The
// gathered rows land in ctx->cmp_X (grown on demand), indices and count in ctx->cmp_idx.
int launch_compact(gpb_ctx* ctx, const double* X_dev, int64_t W, int64_t dx, const double* lo_dev, const double* hi_dev,
                   double outside, double* ll_dev, int premarked) {
    if (W > ctx->Wcap || W >= (1ll << 31)) GPB_FAIL(GPB_E_STATE, "gpb: internal: compaction beyond the workspace");
    int rc = ensure_cmp_rows(ctx, dx);
    if (rc) return rc;
    ctx->hint_from = ctx;
    if (premarked == 2) return 0;                      // k_propose has gathered the rows as well
    const unsigned nb = (unsigned)((W + 255) / 256);
    int* rank = ctx->cmp_idx + 4 + ctx->Wcap;          // [Wcap] ranks, then [Wcap / 256 + 1] workgroup counts
    int* blockcnt = rank + ctx->Wcap;
    const size_t sh = sizeof(double) * 256 * (size_t)((dx < 64 ? dx : 64) + 1);
    if (sh > 64 * 1024 && !premarked)
        GPB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_compact_mark), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    // premarked: k_propose has left 0/1 flags in rank[] and `outside` in ll (see there)
    if (!premarked)
        hipLaunchKernelGGL(k_compact_mark, dim3(nb), dim3(256), sh, ctx->stream, X_dev, W, (int)dx, lo_dev, hi_dev, outside,
                           ll_dev, rank, blockcnt);
    hipLaunchKernelGGL(k_compact_gather, dim3(nb), dim3(256), 0, ctx->stream, X_dev, W, (int)dx, rank,
                       premarked ? nullptr : blockcnt, ctx->cmp_X,
                       ctx->cmp_idx, ctx->profile ? ctx->rows_live : nullptr, ctx->live_hint);
    GPB_HIP(hipGetLastError());
    return 0;
}

// the buffer of gathered rows [Wcap][dx], grown on demand
int ensure_cmp_rows(gpb_ctx* ctx, int64_t dx) {
    if (ctx->cmp_X.cap >= ctx->Wcap * dx) return 0;    // (tested here as well: the memset below is for a NEW buffer only)
    int rc = ctx_grow(ctx, ctx->cmp_X, ctx->Wcap * dx);
    if (rc) return rc;
    GPB_HIP(hipMemsetAsync(ctx->cmp_X, 0, sizeof(double) * (size_t)(ctx->Wcap * dx), ctx->stream));   // rows past the count are read (not used) by the upper-bound launches
    return 0;
}

// true when gpb_logpost / gpb_emcee_run may evaluate the rows inside the box only (a block likelihood kernel follows)
bool compaction_applies(const gpb_ctx* ctx) {
    return ctx->compact && (lowrank_applies(ctx) || block_kernels_apply(ctx));
}

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_box_finish(gpb_ctx* ctx, const double* X_dev, int64_t W, int64_t d, const double* lo_dev,
                              const double* hi_dev, double outside_value, double inside_const,
                              double* ll_inout_dev) {
    if (!ctx || W < 0 || d < 1 || !X_dev || !lo_dev || !hi_dev || !ll_inout_dev) return GPB_E_ARG;
    if (W == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_box, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, ctx->stream, X_dev, W, (int)d,
                       lo_dev, hi_dev, outside_value, inside_const, ll_inout_dev);
    GPB_HIP(hipGetLastError());
    return 0;
}
