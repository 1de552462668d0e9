// gpb_loo.hip — the pointwise leave-one-out conditionals of a Gaussian likelihood that does not factorise (Buerkner, Gabry, Vehtari,
// Comput. Stat. 2021): per row w, with dY = y[w] - yexp, Cw = C[w] + Cadd = L L^T, P = Cw^-1 and g = P dY, for every observable m
//     ll_T[m, w] = ln p(y_m | y_-m, theta_w) = -1/2 ln(2 pi / P_mm) - 1/2 g_m^2 / P_mm
//     zc_T[m, w] = g_m / sqrt(P_mm)            the standardised conditional residual (y_m - E[y_m | y_-m]) / sd[y_m | y_-m]
// (the conditional of observable m given all others has variance 1 / P_mm and mean y_m - g_m / P_mm).
//   k_loo_row   one workgroup per row, built like k_gof_row of gpb_gof.hip: dY is appended to Cw as row M and the left-looking
//               Cholesky runs over the M + 1 rows with its dot products in two doubles (dot2_sub), so that row M of the factor is
//               z = L^-1 dY.  Then L is inverted in place, row by row from the top: row k of X = L^-1 is
//               X_km = (delta_km - sum_{j = m}^{k - 1} L_kj X_jm) / L_kk, which reads row k of L (copied aside first, for the row is
//               overwritten) and the rows of X above it; the sums again in two doubles.  Then one thread per observable:
//               P_mm = sum_{k >= m} X_km^2 and g_m = sum_{k >= m} X_km z_k, in ascending k.
//               The M + 1 rows and the copy live in LDS while (M + 1) (M | 1) <= GPB_GOF_LDS_DOUBLES (M <= 89, gpb_gof's rule);
//               larger rows are worked in place in their slab of C_dev with z and the copy in the workspace.
// A row with a non-positive pivot raises flag[w] and leaves NaN in its column of both outputs.  A row's bits depend on the row
// alone; there is no atomic.
#include "gpb_internal.h"
#include <math.h>

// Nothing in this file may be contracted (build.py compiles it with -ffp-contract=off, as it compiles gpb_gof.hip): dot2_sub is
// error free only when every operation is rounded on its own.

namespace gpb {

namespace {

constexpr int LOO_THREADS = 256;
constexpr int64_t LOO_LDS_DOUBLES = GPB_GOF_LDS_DOUBLES;
// (M + 1) (M | 1) <= 8064 means M <= 89: the M + 1 rows and the copy of one row take at most 8064 + 89 doubles
static_assert((LOO_LDS_DOUBLES + 128) * 8 <= 64 * 1024, "the row kernel's dynamic LDS stays within the 64 KiB a launch may ask for unannounced");

__host__ __device__ inline int64_t loo_ld(int64_t M) { return M | 1; }
inline bool loo_in_lds(int64_t M) { return (M + 1) * loo_ld(M) <= LOO_LDS_DOUBLES; }

// k_gof_row's (hi, lo) -= x y; a copy, so that gpb_gof.hip and the bits of its tests stay as they are
__device__ __forceinline__ void dot2_sub(double& hi, double& lo, double x, double y) {
    const double p = -__dmul_rn(x, y);
    const double pe = -fma(x, y, p);
    const double s = __dadd_rn(hi, p);
    const double bb = __dsub_rn(s, hi);
    const double se = __dadd_rn(__dsub_rn(hi, __dsub_rn(s, bb)), __dsub_rn(p, bb));
    hi = s;
    lo = __dadd_rn(lo, __dadd_rn(se, pe));
}

// zw [W][M], rw [W][M] of the workspace (rows that do not fit in LDS)
__global__ __launch_bounds__(LOO_THREADS) void k_loo_row(const double* __restrict__ y, double* Cg, const double* __restrict__ yexp,
                                                         const double* __restrict__ Cadd, int M, int in_lds, double* __restrict__ ll_T,
                                                         double* __restrict__ zc_T, int64_t ldo, unsigned char* __restrict__ flag,
                                                         double* zw, double* rw) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int64_t w = blockIdx.x;
    const int t = threadIdx.x;
    const int ld = in_lds ? (int)loo_ld(M) : M;
    double* C = in_lds ? sm : Cg + w * (int64_t)M * M;
    double* zr = in_lds ? sm + (int64_t)M * ld : zw + w * (int64_t)M;      // row M of the augmented matrix
    double* cp = in_lds ? sm + (int64_t)(M + 1) * ld : rw + w * (int64_t)M;  // the copy of the row being inverted
    const double* Cw = Cg + w * (int64_t)M * M;
    const double* yw = y + w * (int64_t)M;
    for (int64_t e = t; e < (int64_t)M * M; e += LOO_THREADS) {
        const int i = (int)(e / M), k = (int)(e - (int64_t)i * M);
        const double v = Cadd ? Cw[e] + Cadd[e] : Cw[e];
        C[(int64_t)i * ld + k] = v;
    }
    for (int m = t; m < M; m += LOO_THREADS) zr[m] = __dsub_rn(yw[m], yexp[m]);
    __syncthreads();
    // left-looking Cholesky over rows j .. M (row M: dY, becoming z).  Every thread reads the same pivot after the barrier: the
    // exit is uniform.
    bool bad = false;
    for (int j = 0; j < M; ++j) {
        const double* Lj = C + (int64_t)j * ld;
        for (int i = j + t; i <= M; i += LOO_THREADS) {
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
        for (int i = j + 1 + t; i <= M; i += LOO_THREADS) {
            double* Li = i < M ? C + (int64_t)i * ld : zr;
            Li[j] = Li[j] / dd;
        }
        if (t == 0) C[(int64_t)j * ld + j] = dd;
        __syncthreads();
    }
    if (bad) {
        for (int m = t; m < M; m += LOO_THREADS) {
            ll_T[m * ldo + w] = NAN;
            if (zc_T) zc_T[m * ldo + w] = NAN;
        }
        if (t == 0) flag[w] = 1;
        return;
    }
    // X = L^-1 in place, row by row: rows above k hold X already, row k of L is read from its copy
    for (int k = 0; k < M; ++k) {
        double* Lk = C + (int64_t)k * ld;
        for (int j = t; j <= k; j += LOO_THREADS) cp[j] = Lk[j];
        __syncthreads();
        const double dk = cp[k];
        for (int m = t; m <= k; m += LOO_THREADS) {
            double hi = m == k ? 1.0 : 0.0, lo = 0.0;
            for (int j = m; j < k; ++j) dot2_sub(hi, lo, cp[j], C[(int64_t)j * ld + m]);
            Lk[m] = __dadd_rn(hi, lo) / dk;
        }
        __syncthreads();
    }
    for (int m = t; m < M; m += LOO_THREADS) {
        double pmm = 0.0, gm = 0.0;
        for (int k = m; k < M; ++k) {
            const double x = C[(int64_t)k * ld + m];
            pmm = __dadd_rn(pmm, __dmul_rn(x, x));
            gm = __dadd_rn(gm, __dmul_rn(x, zr[k]));
        }
        ll_T[m * ldo + w] = __dsub_rn(__dmul_rn(-0.5, log(6.283185307179586477 / pmm)), __dmul_rn(0.5, __dmul_rn(gm, gm) / pmm));
        if (zc_T) zc_T[m * ldo + w] = gm / sqrt(pmm);
    }
    if (t == 0) flag[w] = 0;
}

}  // namespace

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_loo_pointwise(gpb_ctx* ctx, int64_t W, int64_t M, const double* y_dev, double* C_dev, const double* yexp_dev,
                                 const double* Cadd_dev, double* ll_T, double* zc_T, int64_t ld, unsigned char* flag_dev) {
    if (!ctx || !y_dev || !C_dev || !yexp_dev || !ll_T || !flag_dev) return GPB_E_ARG;
    if (W < 0 || M < 1) GPB_FAIL(GPB_E_ARG, "gpb_loo_pointwise: need W >= 0 and M >= 1");
    if (M > GPB_GOF_MAX_M) GPB_FAIL(GPB_E_ARG, "gpb_loo_pointwise: M above 2048");
    if (W > 0x7fffffffLL || ld < W) GPB_FAIL(GPB_E_ARG, "gpb_loo_pointwise: need W <= 2^31 - 1 and ld >= W");
    if (W == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    const bool in_lds = loo_in_lds(M);
    double *zw = nullptr, *rw = nullptr;
    if (!in_lds)
        if (const int rc = ctx_carve(ctx, ctx->loo_ws, [&](Carver<double>& c) {
                zw = c.take<double>(W * M);
                rw = c.take<double>(W * M);
            }))
            return rc;
    const size_t lds = in_lds ? sizeof(double) * (size_t)((M + 1) * loo_ld(M) + M) : 0;
    hipLaunchKernelGGL(k_loo_row, dim3((unsigned)W), dim3(LOO_THREADS), lds, ctx->stream, y_dev, C_dev, yexp_dev, Cadd_dev, (int)M,
                       in_lds ? 1 : 0, ll_T, zc_T, ld, flag_dev, zw, rw);
    GPB_HIP(hipGetLastError());
    return 0;
}
