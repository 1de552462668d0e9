// gpb_sens.hip — response matrix and Fisher information of a set of posterior rows (gpb_sens_accumulate): what
// examples/SensitivityAnalysis.ipynb builds at one design point from 2 d finite-difference predictions, reduced over all rows of a
// chain, and the quantity that weighs the response by the uncertainties, J^T C^-1 J with the covariance the likelihood uses
// (src/mcmc.py:288-290).  Per row w, with Cw = C[w] + Cadd = L L^T:
//   k_sens_row    one workgroup per row: Cw -> L (left-looking Cholesky), U = L^-1 J by forward substitution, F_w = U^T U (upper
//                 triangle computed, mirrored: the triangles hold the same bits).  The dot products of the factorisation and of the
//                 substitution are carried in two doubles (dot2_sub): the bar on F is a small multiple of LAPACK's error on the
//                 host, and a plain fp64 elimination in another order misses it on one ill-conditioned case in a few.  Cw and U
//                 live in LDS while M (M | 1) + M d <= SENS_LDS_DOUBLES: the leading dimension M | 1 is odd, so the reads of the
//                 factorisation (lane i at row i, 8 (M | 1) bytes apart) fall on 32 different 8-byte bank pairs per half wave.
//                 Larger rows are factorised in place in their own slab of C_dev, with U in the workspace.  The row leaves F_w
//                 [d, d], the diagonal of Cw [M] and a flag (a non-positive pivot) in the workspace.
//   k_sens_chunk  one thread per entry and chunk of 256 consecutive rows: the chunk's sum of wt * term by ONE tree — sixteen runs of
//                 sixteen rows, each run summed in order, then the runs in order.  R = (x_j J_mj) / y_m and I = (J_mj J_mj) / Cw_mm are
//                 formed here from the inputs, every operation rounded on its own.  A row with wt == 0 or a raised flag is skipped by
//                 a branch: nothing of it is read into a sum.
//   k_sens_add    one thread per entry adds the chunk sums to acc in chunk order.
// No floating-point atomics; the only atomic is the integer count of bad rows.  A call must start on a chunk boundary (cnt[0] a
// multiple of 256), so any split of the rows into slabs that are multiples of 256 (the last one free) forms the same chunks, the
// same trees and the same order of additions as one call on all rows.
#include "gpb_internal.h"
#include <math.h>

// Nothing in this file may be contracted: dot2_sub is an error-free transformation only if its products, sums and differences
// are rounded one by one, and k_sens_chunk promises the host formulas' bits.  build.py compiles THIS file with -ffp-contract=off
// (SOURCE_FLAGS).  hipcc's default is -ffp-contract=fast, under which the backend fuses whatever it finds: the __d*_rn
// intrinsics are plain operators in this toolchain and `#pragma clang fp contract(off)` does not reach the backend — both were
// tried and the emitted loops read.  The fused operations that are meant are written as fma().

namespace gpb {

namespace {

constexpr int SENS_THREADS = 256;
constexpr int SENS_CHUNK = 256;                  // rows per tree
constexpr int SENS_RUN = 16;                     // rows per run of the tree (SENS_CHUNK / SENS_RUN runs)
constexpr int64_t SENS_LDS_DOUBLES = GPB_SENS_LDS_DOUBLES;
static_assert(SENS_CHUNK == SENS_RUN * SENS_RUN, "the tree is SENS_RUN runs of SENS_RUN rows");
static_assert(SENS_LDS_DOUBLES * 8 <= 64 * 1024, "the row kernel's dynamic LDS stays within the 64 KiB a launch may ask for unannounced");

__host__ __device__ inline int64_t sens_ld(int64_t M) { return M | 1; }
inline bool sens_in_lds(int64_t M, int64_t d) { return M * sens_ld(M) + M * d <= SENS_LDS_DOUBLES; }

// (hi, lo) -= x y without rounding the product or the difference away (Ogita, Rump, Oishi: Dot2): TwoProduct by fma, TwoSum,
// the two errors added to lo.  Holds only uncontracted (the note above); the emitted loop was read: one v_mul_f64, one
// v_fma_f64 (the product's error), eight v_add_f64 per term.
__device__ __forceinline__ void dot2_sub(double& hi, double& lo, double x, double y) {
    const double p = -__dmul_rn(x, y);
    const double pe = -fma(x, y, p);                 // x y = -(p + pe) exactly
    const double s = __dadd_rn(hi, p);
    const double bb = __dsub_rn(s, hi);
    const double se = __dadd_rn(__dsub_rn(hi, __dsub_rn(s, bb)), __dsub_rn(p, bb));
    hi = s;
    lo = __dadd_rn(lo, __dadd_rn(se, pe));
}

// Fw [W][d d], dg [W][M], flag [W], Ug [W][M d] (the global path) of the workspace
__global__ __launch_bounds__(SENS_THREADS) void k_sens_row(const double* __restrict__ J, double* Cg, const double* __restrict__ Cadd,
                                                           const double* __restrict__ wt, int M, int d, int in_lds,
                                                           double* __restrict__ Fw, double* __restrict__ dg, int* __restrict__ flag,
                                                           double* Ug, unsigned long long* nbad) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int64_t w = blockIdx.x;
    const int t = threadIdx.x;
    if (wt && wt[w] == 0.0) {                    // (uniform: the whole workgroup leaves)
        if (t == 0) flag[w] = 0;
        return;
    }
    const int ld = in_lds ? (int)sens_ld(M) : M;
    double* C = in_lds ? sm : Cg + w * (int64_t)M * M;
    double* U = in_lds ? sm + (int64_t)M * ld : Ug + w * (int64_t)M * d;
    const double* Cw = Cg + w * (int64_t)M * M;
    const double* Jw = J + w * (int64_t)M * d;
    for (int64_t e = t; e < (int64_t)M * M; e += SENS_THREADS) {
        const int i = (int)(e / M), k = (int)(e - (int64_t)i * M);
        const double v = Cadd ? Cw[e] + Cadd[e] : Cw[e];
        C[(int64_t)i * ld + k] = v;
        if (i == k) dg[w * M + i] = v;
    }
    for (int64_t e = t; e < (int64_t)M * d; e += SENS_THREADS) U[e] = Jw[e];
    __syncthreads();
    // left-looking Cholesky, lower triangle: column j's entries are C_ij - sum_{k<j} L_ik L_jk with the sum carried in two doubles
    // (dot2), so an entry of L carries one rounding of its own, not one per term.  Every thread reads the same pivot after the
    // barrier: the exit is uniform.
    bool bad = false;
    for (int j = 0; j < M; ++j) {
        const double* Lj = C + (int64_t)j * ld;
        for (int i = j + t; i < M; i += SENS_THREADS) {
            const double* Li = C + (int64_t)i * ld;
            double hi = Li[j], lo = 0.0;
            for (int k = 0; k < j; ++k) dot2_sub(hi, lo, Li[k], Lj[k]);
            C[(int64_t)i * ld + j] = __dadd_rn(hi, lo);
        }
        __syncthreads();
        const double ajj = C[(int64_t)j * ld + j];
        if (!(ajj > 0.0)) {
            bad = true;
            break;
        }
        const double dd = sqrt(ajj);
        __syncthreads();
        for (int i = j + 1 + t; i < M; i += SENS_THREADS) C[(int64_t)i * ld + j] = C[(int64_t)i * ld + j] / dd;
        if (t == 0) C[(int64_t)j * ld + j] = dd;
        __syncthreads();
    }
    if (bad) {
        if (t == 0) {
            flag[w] = 1;
            atomicAdd(nbad, 1ull);
        }
        return;
    }
    // U <- L^-1 J, row by row: U_kc = (J_kc - sum_{i<k} L_ki U_ic) / L_kk, the sum again in two doubles; one thread per column
    for (int k = 0; k < M; ++k) {
        const double* Lk = C + (int64_t)k * ld;
        for (int cc = t; cc < d; cc += SENS_THREADS) {
            double hi = U[(int64_t)k * d + cc], lo = 0.0;
            for (int i = 0; i < k; ++i) dot2_sub(hi, lo, Lk[i], U[(int64_t)i * d + cc]);
            U[(int64_t)k * d + cc] = __dadd_rn(hi, lo) / Lk[k];
        }
        __syncthreads();
    }
    // F = U^T U: pair p of the upper triangle, row a: pairs a (2 d - a + 1) / 2 .. ; both triangles get the one value
    const int npair = d * (d + 1) / 2;
    for (int p = t; p < npair; p += SENS_THREADS) {
        int a = 0, rem = p;
        while (rem >= d - a) {
            rem -= d - a;
            ++a;
        }
        const int b = a + rem;
        double s = 0.0;
        for (int i = 0; i < M; ++i) s = fma(U[(int64_t)i * d + a], U[(int64_t)i * d + b], s);
        Fw[w * (int64_t)d * d + a * d + b] = s;
        Fw[w * (int64_t)d * d + b * d + a] = s;
    }
    if (t == 0) flag[w] = 0;
}

// entry e of a chunk's sums: 0 the weights, 1 .. d d the Fisher matrix, then one thread per (m, j) for R, R^2 and I
__global__ __launch_bounds__(SENS_THREADS) void k_sens_chunk(const double* __restrict__ J, const double* __restrict__ y,
                                                             const double* __restrict__ x, const double* __restrict__ wt, int64_t W,
                                                             int M, int d, const double* __restrict__ Fw, const double* __restrict__ dg,
                                                             const int* __restrict__ flag, double* __restrict__ part, int64_t nacc) {
    const int64_t c = blockIdx.x;
    const int64_t e = (int64_t)blockIdx.y * SENS_THREADS + threadIdx.x;
    const int64_t dd = (int64_t)d * d, Md = (int64_t)M * d;
    if (e >= 1 + dd + Md) return;
    const int kind = e == 0 ? 0 : (e < 1 + dd ? 1 : 2);
    const int64_t q = kind == 2 ? e - 1 - dd : e - 1;       // (m, j) flattened, or the entry of F
    const int m = kind == 2 ? (int)(q / d) : 0, j = kind == 2 ? (int)(q - (int64_t)m * d) : 0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int g = 0; g < SENS_RUN; ++g) {
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;
        for (int k = 0; k < SENS_RUN; ++k) {
            const int64_t w = c * SENS_CHUNK + g * SENS_RUN + k;
            double t0 = 0.0, t1 = 0.0, t2 = 0.0;
            if (w < W && flag[w] == 0) {
                const double a = wt ? wt[w] : 1.0;
                if (a != 0.0) {
                    if (kind == 0) t0 = a;
                    else if (kind == 1) t0 = __dmul_rn(a, Fw[w * dd + q]);
                    else {
                        const double jm = J[w * Md + q];
                        const double R = __dmul_rn(x[w * d + j], jm) / y[w * M + m];
                        const double I = __dmul_rn(jm, jm) / dg[w * M + m];
                        t0 = __dmul_rn(a, R);
                        t1 = __dmul_rn(a, __dmul_rn(R, R));
                        t2 = __dmul_rn(a, I);
                    }
                }
            }
            r0 = __dadd_rn(r0, t0);
            r1 = __dadd_rn(r1, t1);
            r2 = __dadd_rn(r2, t2);
        }
        s0 = __dadd_rn(s0, r0);
        s1 = __dadd_rn(s1, r1);
        s2 = __dadd_rn(s2, r2);
    }
    double* out = part + c * nacc;
    if (kind != 2) out[e] = s0;
    else {
        out[1 + dd + q] = s0;
        out[1 + dd + Md + q] = s1;
        out[1 + dd + 2 * Md + q] = s2;
    }
}

__global__ __launch_bounds__(SENS_THREADS) void k_sens_add(const double* __restrict__ part, int64_t nchunks, int64_t nacc,
                                                           double* __restrict__ acc, long long* cnt, int64_t W) {
    const int64_t e = (int64_t)blockIdx.x * SENS_THREADS + threadIdx.x;
    if (e == 0) cnt[0] += W;
    if (e >= nacc) return;
    double a = acc[e];
    for (int64_t c = 0; c < nchunks; ++c) a = __dadd_rn(a, part[c * nacc + e]);
    acc[e] = a;
}

}  // namespace

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_sens_accumulate(gpb_ctx* ctx, int64_t W, int64_t M, int64_t d, const double* J_dev, const double* y_dev,
                                   double* C_dev, const double* Cadd_dev, const double* x_dev, const double* wt_dev, double* acc_dev,
                                   int64_t* cnt_dev) {
    if (!ctx || !J_dev || !y_dev || !C_dev || !x_dev || !acc_dev || !cnt_dev) return GPB_E_ARG;
    if (W < 0 || M < 1 || d < 1) GPB_FAIL(GPB_E_ARG, "gpb_sens_accumulate: need W >= 0, M >= 1 and d >= 1");
    if (M > GPB_SENS_MAX_M || d > GPB_SENS_MAX_D) GPB_FAIL(GPB_E_ARG, "gpb_sens_accumulate: M above 2048 or d above 64");
    if (W > 0x7fffffffLL) GPB_FAIL(GPB_E_ARG, "gpb_sens_accumulate: more than 2^31 - 1 rows in one call");
    if (W == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    long long seen = 0;
    GPB_HIP(hipMemcpyAsync(&seen, cnt_dev, sizeof(seen), hipMemcpyDeviceToHost, ctx->stream));
    GPB_HIP(hipStreamSynchronize(ctx->stream));
    if (seen < 0 || seen % SENS_CHUNK != 0)
        GPB_FAIL(GPB_E_STATE, "gpb_sens_accumulate: the rows seen so far are not a multiple of 256 (only the last slab may be ragged)");
    const bool in_lds = sens_in_lds(M, d);
    const int64_t nacc = GPB_SENS_ACC_DOUBLES(M, d), nchunks = (W + SENS_CHUNK - 1) / SENS_CHUNK;
    double *Fw, *dg, *Ug, *part;
    int* flag;
    if (const int rc = ctx_carve(ctx, ctx->sens_ws, [&](Carver<double>& c) {
            Fw = c.take<double>(W * d * d);
            dg = c.take<double>(W * M);
            Ug = c.take<double>(in_lds ? 0 : W * M * d);
            part = c.take<double>(nchunks * nacc);
            flag = c.take<int>(W);
        }))
        return rc;
    const size_t lds = in_lds ? sizeof(double) * (size_t)(M * sens_ld(M) + M * d) : 0;
    hipLaunchKernelGGL(k_sens_row, dim3((unsigned)W), dim3(SENS_THREADS), lds, ctx->stream, J_dev, C_dev, Cadd_dev, wt_dev, (int)M,
                       (int)d, in_lds ? 1 : 0, Fw, dg, flag, Ug, reinterpret_cast<unsigned long long*>(cnt_dev + 1));
    const int64_t nthr = 1 + d * d + M * d;
    hipLaunchKernelGGL(k_sens_chunk, dim3((unsigned)nchunks, (unsigned)((nthr + SENS_THREADS - 1) / SENS_THREADS)), dim3(SENS_THREADS), 0,
                       ctx->stream, J_dev, y_dev, x_dev, wt_dev, W, (int)M, (int)d, Fw, dg, flag, part, nacc);
    hipLaunchKernelGGL(k_sens_add, dim3((unsigned)((nacc + SENS_THREADS - 1) / SENS_THREADS)), dim3(SENS_THREADS), 0, ctx->stream, part,
                       nchunks, nacc, acc_dev, reinterpret_cast<long long*>(cnt_dev), W);
    GPB_HIP(hipGetLastError());
    return 0;
}
