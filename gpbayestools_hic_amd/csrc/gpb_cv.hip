// gpb_cv.hip — closed-form leave-one-out / leave-k-out cross-validation of the factored GPs (gpb_gp_cv, gpb_emu_cv).
//
// With Ky = K + sigma_n^2 I + diag(t) = L L^T, t_i = alpha_reg + s_i (s: the per-point simulation noise of gpb_gp_set_point_noise, zero
// when none is installed), and a fold F of k design points (Rasmussen & Williams, section 5.4.2, for blocks):
//     G_F = (Ky^-1)_FF = (L^-1[:, F])^T (L^-1[:, F])                  a k x k Gram matrix over rows of L^-1
//     mean of the GP refitted without F (same theta) at X_F           = z_F - G_F^-1 alpha_F
//     its GPR.predict(X_F, return_cov=True)                           = G_F^-1 - diag(t_F)
// (sklearn's predictive prior carries the White noise but not `alpha`, scalar or per point: sk:_gpr.py:441-469).  Nothing of size N is factored: L^-1
// and alpha stay resident after gpb_gp_factor.  Design point i lives at stored row / column pad_front(Np, N) + i.
//
// General path (k_cv_fold): one workgroup per (fold, GP) walks the rows of L^-1 from the fold's smallest stored column down in 64-row
//   slabs, gathers the fold's columns of a slab into LDS (the next slab's are in flight in registers meanwhile) and accumulates G with
//   v_mfma_f64_16x16x4_f64 (mma_nt_64); G, padded to 64 with a unit diagonal, is factored and inverted in LDS (potf2_inv_64).
// Leave-one-out path (k_cv_colsq + k_cv_loo): G is the sum of squares of one column: one coalesced pass over the lower block triangle
//   of L^-1, column blocks x 64-row chunks, and the chunk partials of a column summed in order.
// Every sum has a fixed order and no floating-point atomics: a fold's bits do not depend on the folds or GPs that share the call.
// Elements above the diagonal of L^-1 are never read (they are zeros where the factorisation wrote them, nothing where it did not).
#include "gpb_internal.h"
#include "chol_block.h"
#include <math.h>

namespace gpb {

namespace {

constexpr int CV_MAX_FOLD = 64;

// element (GP p, position q of idx) of mean / var sits at out[p * sp + q * si]: [n_idx][P] for the callers of gpb_gp_cv (sp = 1,
// si = P), the predict workspace [P][Wld] in front of the observable transform (sp = Wld, si = 1)
struct CvOut {
    double* mean;
    double* var;
    int64_t sp, si;
    double* cov;          // [P][nf][kmax][kmax] or nullptr
    int kmax;
};

__global__ __launch_bounds__(CHOL_THREADS) void k_cv_fold(const double* __restrict__ Linv, const double* __restrict__ alpha,
                                                          const double* __restrict__ Z, const int* __restrict__ idx,
                                                          const int* __restrict__ fold_ptr, int64_t Np, int pad, double alpha_reg,
                                                          const double* __restrict__ pnoise, int nf, CvOut out,
                                                          int* __restrict__ notpd) {
    __shared__ CholLds s;
    __shared__ int scol[64];
    __shared__ double sa[64], sz[64], su[64], st[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f = blockIdx.x, p = blockIdx.y;
    const int q0 = fold_ptr[f], k = fold_ptr[f + 1] - q0;         // 1 <= k <= 64 (checked on the host)
    if (tid < 64) {
        const int c = tid < k ? pad + idx[q0 + tid] : (int)Np;     // a column past the matrix: never read
        scol[tid] = c;
        sa[tid] = tid < k ? alpha[(int64_t)p * Np + c] : 0.0;
        sz[tid] = tid < k ? Z[(int64_t)p * Np + c] : 0.0;
        st[tid] = (tid < k && pnoise) ? alpha_reg + pnoise[(int64_t)p * Np + c] : alpha_reg;      // t_i: alpha + s_i first (k_kmat)
    }
    __syncthreads();
    int cmin = (int)Np;
    for (int j = 0; j < k; ++j) cmin = min(cmin, scol[j]);
    const double* Lp = Linv + (int64_t)p * Np * Np;
    // the gather of one slab: thread (j = fold column, rows rr0, rr0 + 8, ...): consecutive lanes read one row of L^-1 (adjacent
    // addresses for a contiguous fold) and store LDS addresses 65 doubles apart (no bank conflict)
    const int gj = tid & 63, rr0 = tid >> 6;
    const int gc = scol[gj];
    double v[8];
    auto gather = [&](int64_t r) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t row = r + rr0 + 8 * e;
            v[e] = row >= gc ? Lp[row * Np + gc] : 0.0;          // (gc = Np for the padding columns: always zero)
        }
    };
    d4 acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    const int64_t rbeg = (cmin / 64) * 64;
    gather(rbeg);
    for (int64_t r = rbeg; r < Np; r += 64) {
        __syncthreads();                               // the previous slab's product is done reading s.a
#pragma unroll
        for (int e = 0; e < 8; ++e) s.a[gj][rr0 + 8 * e] = v[e];
        __syncthreads();
        if (r + 64 < Np) gather(r + 64);
        mma_nt_64(s.a, s.a, acc, wave, lane);          // G[i][j] += sum_rows L^-1[row][c_i] L^-1[row][c_j]
    }
    __syncthreads();                                   // s.a is free: G goes there, padded with a unit diagonal
    {
        const int m0 = (wave >> 2) * 32, n0 = (wave & 3) * 16, lr = lane & 15, lk = lane >> 4;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = m0 + 16 * t + lk + 4 * r, j = n0 + lr;
                s.a[i][j] = (i == j && i >= k) ? 1.0 : acc[t][r];
            }
    }
    potf2_inv_64(s);                                   // opens and ends with a barrier: s.x = L_G^-1 (zeros above the diagonal)
    const bool bad = s.bad >= 0 && s.bad < k;
    // G^-1 = X^T X with X = L_G^-1:  u = X alpha_F,  w = X^T u = G^-1 alpha_F,  diag(G^-1)_i = sum_m X_mi^2
    if (tid < 64) {
        double u = 0.0;
        for (int i = 0; i <= tid; ++i) u = fma(s.x[tid][i], sa[i], u);
        su[tid] = u;
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    if (tid < k) {
        double w = 0.0, g = 0.0;
        for (int m = tid; m < 64; ++m) {
            const double x = s.x[m][tid];
            w = fma(x, su[m], w);
            g = fma(x, x, g);
        }
        const int64_t o = (int64_t)p * out.sp + (int64_t)(q0 + tid) * out.si;
        out.mean[o] = bad ? nan : sz[tid] - w;
        if (out.var) out.var[o] = bad ? nan : g - st[tid];
    }
    if (out.cov) {
        const int km = out.kmax;
        double* C = out.cov + ((int64_t)p * nf + f) * km * km;
        for (int e = tid; e < km * km; e += CHOL_THREADS) {
            const int i = e / km, j = e % km;
            double g = 0.0;
            if (i < k && j < k) {
                for (int m = max(i, j); m < 64; ++m) g = fma(s.x[m][i], s.x[m][j], g);
                g = bad ? nan : (i == j ? g - st[i] : g);
            }
            C[e] = g;
        }
    }
    if (bad && tid == 0) atomicAdd(notpd, 1);
}

// part[p][rc][col] = sum over the rows of 64-row chunk rc of L^-1[row][col]^2, for the chunks at or below column block cb
__global__ __launch_bounds__(256) void k_cv_colsq(const double* __restrict__ Linv, double* __restrict__ part, int64_t Np, int nI) {
    __shared__ double sh[4][64];
    const int cb = blockIdx.x, rc = blockIdx.y, p = blockIdx.z;
    if (rc < cb) return;                               // above the diagonal: zeros, never read back
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t col = (int64_t)cb * 64 + lane;
    const double* Lp = Linv + (int64_t)p * Np * Np;
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int64_t row = (int64_t)rc * 64 + w + 4 * e;
        const double x = row >= col ? Lp[row * Np + col] : 0.0;
        acc = fma(x, x, acc);
    }
    sh[w][lane] = acc;
    __syncthreads();
    if (w == 0) part[((int64_t)p * nI + rc) * Np + col] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

__global__ __launch_bounds__(256) void k_cv_loo(const double* __restrict__ part, const double* __restrict__ alpha,
                                                const double* __restrict__ Z, const int* __restrict__ idx, int64_t n_idx,
                                                int64_t Np, int nI, int pad, double alpha_reg,
                                                const double* __restrict__ pnoise, CvOut out, int* __restrict__ notpd) {
    const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int p = blockIdx.y;
    if (q >= n_idx) return;
    const int64_t col = pad + (idx ? (int64_t)idx[q] : q);
    double g = 0.0;
    for (int rc = (int)(col / 64); rc < nI; ++rc) g += part[((int64_t)p * nI + rc) * Np + col];
    const bool bad = !(g > 0.0);
    const double nan = __builtin_nan("");
    const double ginv = 1.0 / g;
    const int64_t o = (int64_t)p * out.sp + q * out.si;
    const double var = bad ? nan : ginv - (pnoise ? alpha_reg + pnoise[(int64_t)p * Np + col] : alpha_reg);
    out.mean[o] = bad ? nan : Z[(int64_t)p * Np + col] - alpha[(int64_t)p * Np + col] * ginv;
    if (out.var) out.var[o] = var;
    if (out.cov) out.cov[(int64_t)p * n_idx + q] = var;           // kmax = 1, nf = n_idx
    if (bad) atomicAdd(notpd, 1);
}

// the pieces of cv_ws for the planned call (CvWs, ws_layout.h): its folds, if it has a list of them, and the leave-one-out partials
void cv_lay(const gpb_ctx* ctx, Carver<int>& c, CvWs& ws) {
    ws.lay(c, ctx->cv_has_idx ? ctx->cv_n + ctx->cv_nf + 1 : 0, ctx->cv_loo ? ctx->P * (ctx->Np / 64) * ctx->Np : 0);
}

}  // namespace

// Checks the folds of a cross-validation call and stores them in the context (device copy included); *kmax = the largest fold.
int cv_plan(gpb_ctx* ctx, const char* who, const int32_t* idx, int64_t n_idx, const int32_t* fold_ptr, int64_t nf, int64_t* kmax) {
    const std::string w(who);
    if (ctx->N == 0) GPB_FAIL(GPB_E_STATE, w + " before gpb_gp_set");
    if (ctx->multi) GPB_FAIL(GPB_E_STATE, w + ": a gpb_gp_set_multi context is fit-only (its GPs have different designs)");
    if (!ctx->factored) GPB_FAIL(GPB_E_STATE, w + " before gpb_gp_factor");
    const int64_t N = ctx->N;
    ctx->cv_loo = true;
    ctx->cv_has_idx = idx != nullptr;
    *kmax = 1;
    if (!idx) {                                        // leave-one-out over all N points in order
        if (n_idx != N || fold_ptr || nf != N) GPB_FAIL(GPB_E_ARG, w + ": idx == NULL means leave-one-out of all points: n_idx = nf = N, fold_ptr = NULL");
    } else {
        if (n_idx < 1 || n_idx > N || nf < 1 || nf > n_idx) GPB_FAIL(GPB_E_ARG, w + ": need 1 <= nf <= n_idx <= N");
        if (!fold_ptr && nf != n_idx) GPB_FAIL(GPB_E_ARG, w + ": fold_ptr == NULL means one point per fold: nf = n_idx");
        std::vector<char> seen((size_t)N, 0);
        for (int64_t q = 0; q < n_idx; ++q) {
            const int64_t i = idx[q];
            if (i < 0 || i >= N) GPB_FAIL(GPB_E_ARG, w + ": design-point index out of range [0, N)");
            if (seen[(size_t)i]) GPB_FAIL(GPB_E_ARG, w + ": a design point appears twice (folds must be disjoint)");
            seen[(size_t)i] = 1;
        }
        if (fold_ptr) {
            if (fold_ptr[0] != 0 || fold_ptr[nf] != n_idx) GPB_FAIL(GPB_E_ARG, w + ": fold_ptr must run from 0 to n_idx");
            for (int64_t f = 0; f < nf; ++f) {
                const int64_t k = (int64_t)fold_ptr[f + 1] - fold_ptr[f];
                if (k < 1) GPB_FAIL(GPB_E_ARG, w + ": empty fold (fold_ptr must increase)");
                if (k > CV_MAX_FOLD) GPB_FAIL(GPB_E_ARG, w + ": a fold has more than 64 points (the closed form is for folds of 1 to 64; refit for larger ones)");
                if (k > *kmax) *kmax = k;
            }
        }
        ctx->cv_loo = *kmax == 1;
    }
    ctx->cv_n = n_idx; ctx->cv_nf = nf; ctx->cv_kmax = *kmax;
    GPB_HIP(hipSetDevice(ctx->device));
    CvWs ws;
    if (const int rc = ctx_carve(ctx, ctx->cv_ws, [&](Carver<int>& c) { cv_lay(ctx, c, ws); })) return rc;
    if (idx) {
        // the host copy lives in the context: the previous call's upload must have left it before it is overwritten
        GPB_HIP(hipStreamSynchronize(ctx->stream));
        ctx->h_cv.assign(idx, idx + n_idx);
        for (int64_t f = 0; f <= nf; ++f) ctx->h_cv.push_back(fold_ptr ? fold_ptr[f] : (int)f);
        GPB_HIP(hipMemcpyAsync(ws.folds, ctx->h_cv.data(), sizeof(int) * ctx->h_cv.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    return 0;
}

// The planned cross-validation (cv_plan): mean / var at [p * sp + q * si], cov_dev [P][nf][kmax][kmax] or nullptr.
int launch_cv(gpb_ctx* ctx, double* mean_dev, double* var_dev, int64_t sp, int64_t si, double* cov_dev) {
    const int64_t Np = ctx->Np, P = ctx->P, n_idx = ctx->cv_n, nf = ctx->cv_nf;
    const int nI = (int)(Np / 64), pad = (int)pad_front(Np, ctx->N);
    CvWs ws;
    Carver<int> pieces(ctx->cv_ws.get());
    cv_lay(ctx, pieces, ws);
    const int* idx = ws.folds;
    const CvOut out{mean_dev, var_dev, sp, si, cov_dev, (int)ctx->cv_kmax};
    if (P > 65535 || nI > 65535) GPB_FAIL(GPB_E_ARG, "gpb: cross-validation of more than 65535 GPs or 4 million design points");
    if (ctx->cv_loo) {
        double* part = ws.part;
        hipLaunchKernelGGL(k_cv_colsq, dim3((unsigned)nI, (unsigned)nI, (unsigned)P), dim3(256), 0, ctx->stream, ctx->Linv, part, Np, nI);
        hipLaunchKernelGGL(k_cv_loo, dim3((unsigned)((n_idx + 255) / 256), (unsigned)P), dim3(256), 0, ctx->stream, part, ctx->alpha,
                           ctx->Z, idx, n_idx, Np, nI, pad, ctx->alpha_reg, ctx->pnoise, out, ctx->notpd);
    } else {
        hipLaunchKernelGGL(k_cv_fold, dim3((unsigned)nf, (unsigned)P), dim3(CHOL_THREADS), 0, ctx->stream, ctx->Linv, ctx->alpha,
                           ctx->Z, idx, idx + n_idx, Np, pad, ctx->alpha_reg, ctx->pnoise, (int)nf, out, ctx->notpd);
    }
    GPB_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpb
