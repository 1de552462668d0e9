// gpb_grad.hip — gradients of the emulator's predictions and of the chain's log-posterior with respect to the input.
//
// Per GP (theta = (c, l, sigma_n^2), scaled distance r = |(x - x_i) / l|) the derivative of the kernel is
//     dk(x, x_i)/dx_j = phi(r) (x_j - x_ij) / l_j^2,   phi(r) = (1/r) dk/dr:
//     RBF -c e^{-r^2/2};  Matern-3/2 -3c e^{-sqrt3 r};  Matern-5/2 -(5/3) c (1 + sqrt5 r) e^{-sqrt5 r}
// (all finite at r = 0; the White term is constant), so that
//     dmu/dx_j  = sum_i alpha_i dk_i/dx_j                      (alpha = K^-1 z,  sk:_gpr.py:364,443)
//     dvar/dx_j = -2 sum_i beta_i dk_i/dx_j,  beta = K^-1 k*   (var = k** - k*^T K^-1 k*,  sk:_gpr.py:454-460)
// Kernels:
//   k_betaT     beta^T = V^T L^-1 with V = L^-1 K*^T (k_vmat, gpb_cov.hip): one MFMA GEMM per GP over the k >= n triangle
//   k_gp_grad   the contraction over the design points for every (walker, GP): r and phi recomputed per pair as k_kcross
//               does, the sum formed from the differences (x_j - x_ij) directly, in a fixed order per row (no dependence on
//               the batch, the walker's place in it, or the tiles)
//   k_like_w    d lp / d mu_k and d lp / d var_k of one emulator's likelihood block, all four transform modes
//               (oracle/gp_oracle.py emulator_predict + mvn_loglike restated for the derivative)
//   k_pmap_jac  the Jacobian of the parameterTrafoPCA map (gpb_pmap.hip)
//   k_grad_fold / k_emu_jac / k_grad_finish   chain rule into the chain's parameters, the observable-space Jacobian, box
#include "gpb_internal.h"
#include "gemm_tile.h"
#include <math.h>

namespace gpb {

// beta^T[p][w][n] = sum_{k >= n} V[p][k][w] Linv[p][k][n]   (L^-1 lower: rows k < n of column n are zero)
__global__ __launch_bounds__(256, 2) void k_betaT(const double* __restrict__ V, const double* __restrict__ Linv,
                                                  double* __restrict__ BT, int64_t Np, int64_t Wld) {
    __shared__ TileLds<128> lds;
    const int p = blockIdx.z;
    const int64_t mb = (int64_t)blockIdx.y * 128, nb = (int64_t)blockIdx.x * 128;
    const int n_ext = (int)imin64(128, Np - nb);
    Acc<128> acc;
    acc_zero<128>(acc);
    gemm_tile_loop<128, true, false>(V + (int64_t)p * Np * Wld, Wld, Linv + (int64_t)p * Np * Np, Np, mb, nb, 128, n_ext, nb,
                                     Np, lds, acc);
    tile_store<128>(BT + (int64_t)p * Wld * Np, Np, mb, nb, 128, n_ext, 1.0, false, acc);
}

template <int KIND>
__device__ __forceinline__ double phi_of(double r2, double c) {
    if (KIND == GPB_KERNEL_RBF) return -c * exp(-0.5 * r2);
    if (KIND == GPB_KERNEL_MATERN15) return -3.0 * c * exp(-1.7320508075688772 * sqrt(r2));
    const double t = 2.23606797749979 * sqrt(r2);
    return -(5.0 / 3.0) * c * (1.0 + t) * exp(-t);
}

constexpr int GG_CHUNK = 512;     // design points staged per pass

// One workgroup per (walker w, GP p).  dmean[w][p][j] and (BT != null) dvar[w][p][j], j < d.
// Phase 1: thread per design point i: r^2 from the differences, phi, the two weights phi alpha_i and phi beta_i into LDS.
// Phase 2: thread (j, g) for g < G = 256 / d sums design points g, g + G, ... of the chunk for coordinate j; the G partials
// are added in g order at the end.  Every order depends on d alone.
template <int KIND>
__global__ __launch_bounds__(256) void k_gp_grad(const double* __restrict__ Xq, int64_t ldq, const double* __restrict__ X,
                                                 int dpad, const double* __restrict__ ls, const double* __restrict__ amp,
                                                 const double* __restrict__ alpha, const double* __restrict__ BT,
                                                 int64_t Np, int64_t pad, int64_t N, int d, int P, int64_t Wld,
                                                 double* __restrict__ dmean, double* __restrict__ dvar) {
    __shared__ double xq[MAX_D], il[MAX_D];
    __shared__ double wa[GG_CHUNK], wb[GG_CHUNK];
    __shared__ double ra[256], rb[256];
    const int64_t w = blockIdx.x;
    const int p = blockIdx.y, t = threadIdx.x;
    if (t < d) {
        xq[t] = Xq[w * ldq + t];
        il[t] = 1.0 / ls[(int64_t)p * dpad + t];
    }
    __syncthreads();
    const double c = amp[p];
    const double* al = alpha + (int64_t)p * Np + pad;
    const double* bt = BT ? BT + ((int64_t)p * Wld + w) * Np + pad : nullptr;
    const double* Xd = X + pad * dpad;
    const int G = 256 / d, j = t % d, g = t / d;
    const bool act = g < G;
    double sa = 0.0, sb = 0.0;
    for (int64_t c0 = 0; c0 < N; c0 += GG_CHUNK) {
        const int n = (int)imin64(GG_CHUNK, N - c0);
        for (int i = t; i < n; i += 256) {
            const double* xi = Xd + (c0 + i) * dpad;
            double r2 = 0.0;
            for (int k = 0; k < d; ++k) {
                const double df = (xq[k] - xi[k]) * il[k];
                r2 = fma(df, df, r2);
            }
            const double ph = phi_of<KIND>(r2, c);
            wa[i] = ph * al[c0 + i];
            wb[i] = bt ? ph * bt[c0 + i] : 0.0;
        }
        __syncthreads();
        if (act) {
            const double xj = xq[j];
            for (int i = g; i < n; i += G) {
                const double df = xj - Xd[(c0 + i) * dpad + j];
                sa = fma(wa[i], df, sa);
                sb = fma(wb[i], df, sb);
            }
        }
        __syncthreads();
    }
    ra[t] = sa;
    rb[t] = sb;
    __syncthreads();
    if (t < d) {
        double a = 0.0, b = 0.0;
        for (int q = 0; q < G; ++q) {
            a += ra[q * d + t];
            b += rb[q * d + t];
        }
        const double s = il[t] * il[t];
        dmean[(w * P + p) * d + t] = a * s;
        if (dvar) dvar[(w * P + p) * d + t] = -2.0 * b * s;
    }
}

// d lp / d mu_k and d lp / d var_k (wmu / wv [W][P]) of lp = -1/2 dY^T C^-1 dY - 1/2 log det C, dY = y - yexp, C = C_model
// + C_exp, for one row per workgroup.  With u = C^-1 dY and G = dlp/dC = 1/2 (u u^T - C^-1):
//   PCA             y = A^T mu + m0, C_model = sum_k var_k a_k a_k^T + C_trunc:  wmu_k = -a_k.u,  wv_k = a_k^T G a_k
//   NO_PCA          y_i = s_i mu_i + m0_i, C_model = diag(var):                 wmu_i = -s_i u_i,  wv_i = G_ii
//   EXPDIAG         y = exp(A^T mu + m0), C_model = diag(F_i y_i^2), F = diag(sum_k var_k a_k a_k^T + C_trunc):
//                   h_i = y_i (2 G_ii F_i y_i - u_i):  wmu_k = sum_i A_ki h_i,  wv_k = sum_i A_ki^2 G_ii y_i^2
//   NO_PCA_EXPDIAG  y_i = exp(s_i mu_i + m0_i), C_model = diag(var_i y_i^2):  wmu_i = s_i y_i (2 G_ii var_i y_i - u_i),  wv_i = G_ii y_i^2
// C = L L^T in place; the right-hand sides B = [a_0 .. a_{P-1} | dY] (PCA) or [e_0 .. e_{M-1} | dY] are solved as L^-1 B, so that
// with z = L^-1 dY:  s_c = (L^-1 B_c).z  (= a_k.u, or u_i) and q_c = |L^-1 B_c|^2  (= a_k^T C^-1 a_k, or (C^-1)_ii).
// A block that is not positive definite gives NaN weights.  ws: LDS (ws_g null) or a per-row slab of ws_g.
__global__ __launch_bounds__(256) void k_like_w(const double* __restrict__ mean_pc, const double* __restrict__ var_pc, int64_t Wld,
                                                int P, int M, int mode, const double* __restrict__ A, const double* __restrict__ mu,
                                                const double* __restrict__ scale, const double* __restrict__ C0,
                                                const double* __restrict__ yexp, const double* __restrict__ Cexp,
                                                double* __restrict__ wmu, double* __restrict__ wv, double* ws_g, int64_t ws_row) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ int bad;
    const int64_t w = blockIdx.x;
    const int t = threadIdx.x;
    const bool no_pca = (mode == GPB_MODE_NO_PCA || mode == GPB_MODE_NO_PCA_EXPDIAG);
    const bool expdiag = (mode == GPB_MODE_EXPDIAG || mode == GPB_MODE_NO_PCA_EXPDIAG);
    const int ncol = (mode == GPB_MODE_PCA) ? P + 1 : M + 1;
    double* ws = ws_g ? ws_g + w * ws_row : sm;
    double* C = ws;                       // [M][M]
    double* B = C + (int64_t)M * M;       // [M][ncol]
    double* y = B + (int64_t)M * ncol;    // [M]
    double* F = y + M;                    // [M]
    double* h = F + M;                    // [M]
    double* g2 = h + M;                   // [M]
    double* zm = g2 + M;                  // [P]
    double* zv = zm + P;                  // [P]
    double* s = zv + P;                   // [ncol]
    double* q = s + ncol;                 // [ncol]
    if (t == 0) bad = 0;
    for (int k = t; k < P; k += 256) {
        zm[k] = mean_pc[(int64_t)k * Wld + w];
        zv[k] = var_pc[(int64_t)k * Wld + w];
    }
    __syncthreads();
    for (int i = t; i < M; i += 256) {
        double v, f = 0.0;
        if (!no_pca) {
            v = 0.0;
            for (int k = 0; k < P; ++k) {
                v = fma(zm[k], A[k * M + i], v);
                f = fma(zv[k] * A[k * M + i], A[k * M + i], f);
            }
            v += mu[i];
            f += C0[i * M + i];
        } else {
            v = zm[i] * scale[i] + mu[i];
            f = zv[i];
        }
        if (expdiag) v = exp(v);
        y[i] = v;
        F[i] = f;
    }
    __syncthreads();
    for (int e = t; e < M * M; e += 256) {
        const int i = e / M, j = e - i * M;
        double v;
        if (mode == GPB_MODE_PCA) {
            v = 0.0;
            for (int k = 0; k < P; ++k) v = fma(zv[k] * A[k * M + i], A[k * M + j], v);
            v += C0[e];
        } else {
            v = (i == j) ? (expdiag ? F[i] * y[i] * y[i] : F[i]) : 0.0;
        }
        C[e] = v + Cexp[e];
    }
    for (int e = t; e < M * ncol; e += 256) {
        const int i = e / ncol, cc = e - i * ncol;
        double v;
        if (cc == ncol - 1) v = y[i] - yexp[i];
        else if (mode == GPB_MODE_PCA) v = A[cc * M + i];
        else v = (i == cc) ? 1.0 : 0.0;
        B[e] = v;
    }
    __syncthreads();
    // right-looking Cholesky, lower triangle
    const int ty = t >> 4, tx = t & 15;
    for (int j = 0; j < M; ++j) {
        const double ajj = C[j * M + j];
        if (!(ajj > 0.0)) { if (t == 0) bad = 1; }
        const double dd = sqrt(ajj);
        __syncthreads();
        for (int i = j + 1 + t; i < M; i += 256) C[i * M + j] = C[i * M + j] / dd;
        if (t == 0) C[j * M + j] = dd;
        __syncthreads();
        for (int i = j + 1 + ty; i < M; i += 16) {
            const double lij = C[i * M + j];
            for (int k = j + 1 + tx; k <= i; k += 16) C[i * M + k] = fma(-lij, C[k * M + j], C[i * M + k]);
        }
        __syncthreads();
    }
    // B <- L^-1 B, column-oriented forward substitution
    for (int k = 0; k < M; ++k) {
        const double lkk = C[k * M + k];
        for (int cc = t; cc < ncol; cc += 256) B[k * ncol + cc] = B[k * ncol + cc] / lkk;
        __syncthreads();
        const int rows = M - k - 1;
        for (int e = t; e < rows * ncol; e += 256) {
            const int i = k + 1 + e / ncol, cc = e % ncol;
            B[i * ncol + cc] = fma(-C[i * M + k], B[k * ncol + cc], B[i * ncol + cc]);
        }
        __syncthreads();
    }
    for (int cc = t; cc < ncol - 1; cc += 256) {
        double a = 0.0, b = 0.0;
        for (int i = 0; i < M; ++i) {
            const double v = B[i * ncol + cc];
            a = fma(v, B[i * ncol + ncol - 1], a);
            b = fma(v, v, b);
        }
        s[cc] = a;
        q[cc] = b;
    }
    __syncthreads();
    const double nanv = nan("");
    if (mode == GPB_MODE_EXPDIAG) {
        for (int i = t; i < M; i += 256) {
            const double Gi = 0.5 * (s[i] * s[i] - q[i]);
            h[i] = y[i] * (2.0 * Gi * F[i] * y[i] - s[i]);
            g2[i] = Gi * y[i] * y[i];
        }
        __syncthreads();
        for (int k = t; k < P; k += 256) {
            double a = 0.0, b = 0.0;
            for (int i = 0; i < M; ++i) {
                const double aki = A[k * M + i];
                a = fma(aki, h[i], a);
                b = fma(aki * aki, g2[i], b);
            }
            wmu[w * P + k] = bad ? nanv : a;
            wv[w * P + k] = bad ? nanv : b;
        }
        return;
    }
    for (int k = t; k < P; k += 256) {
        double gm, gv;
        const double Gk = 0.5 * (s[k] * s[k] - q[k]);
        if (mode == GPB_MODE_PCA) {
            gm = -s[k];
            gv = Gk;
        } else if (mode == GPB_MODE_NO_PCA) {
            gm = -scale[k] * s[k];
            gv = Gk;
        } else {
            gm = scale[k] * y[k] * (2.0 * Gk * zv[k] * y[k] - s[k]);
            gv = Gk * y[k] * y[k];
        }
        wmu[w * P + k] = bad ? nanv : gm;
        wv[w * P + k] = bad ? nanv : gv;
    }
}

int64_t like_w_doubles(const gpb_ctx* c) {
    const int64_t M = c->M, P = c->P, ncol = (c->mode == GPB_MODE_PCA) ? P + 1 : M + 1;
    return M * M + M * ncol + 4 * M + 2 * P + 2 * ncol;
}
constexpr int64_t LIKE_W_LDS = 6144;   // doubles (48 KiB): larger blocks work in a per-row slab of global memory

// ---- the parameterTrafoPCA map (gpb_pmap.hip): J[w][j][q] = d out_j / d x_q
// d pmap_fn(fn, par, g) / d par[0..3]; the switch of the zeta/s width at g = T0 is ignored (measure zero)
__device__ __forceinline__ void pmap_fn_grad(int fn, const double* par, double g, double* dp) {
    dp[0] = dp[1] = dp[2] = dp[3] = 0.0;
    if (fn == 0) {
        const double zmax = par[0], T0 = par[1], sp = par[2], sm = par[3];
        const bool lo = g < T0;
        const double sig = lo ? sm : sp;
        const double dT = g - T0;
        const double e = exp(-(dT * dT) / (2.0 * (sig * sig)));
        dp[0] = e;
        dp[1] = zmax * e * dT / (sig * sig);
        dp[lo ? 3 : 2] = zmax * e * dT * dT / (sig * sig * sig);
    } else if (fn == 1) {
        if (0.0 < g && g <= 0.2) { dp[0] = 1.0 - g / 0.2; dp[1] = g / 0.2; }
        else if (0.2 < g && g < 0.4) { const double u = (g - 0.2) / 0.2; dp[1] = 1.0 - u; dp[2] = u; }
        else dp[2] = 1.0;
    } else {
        if (0.0 < g && g <= 2.0) dp[0] = g / 2.0;
        else if (2.0 < g && g < 4.0) { const double u = (g - 2.0) / 2.0; dp[0] = 1.0 - u; dp[1] = u; }
        else { const double u = (g - 4.0) / 2.0; dp[1] = 1.0 - u; dp[2] = u; }
    }
}

// one thread per (row, output column j): J[w][j][0 .. d_in)
__global__ __launch_bounds__(256) void k_pmap_jac(const double* __restrict__ X, int64_t W, int d_in, int d_out,
                                                  const int* __restrict__ col_src, int maxpc, const int* __restrict__ desc,
                                                  const double* __restrict__ tab, double* __restrict__ J) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= W * d_out) return;
    const int64_t w = it / d_out;
    const int j = (int)(it - w * d_out);
    const double* x = X + w * d_in;
    double* Jr = J + it * d_in;
    for (int q = 0; q < d_in; ++q) Jr[q] = 0.0;
    const int src = col_src[j];
    if (src >= 0) {
        Jr[src] = 1.0;
        return;
    }
    const int code = -1 - src, g = code / maxpc, c = code - g * maxpc;
    const int* dg = desc + 6 * g;
    const double* tg = tab + (size_t)g * (4 + maxpc) * 100;
    const double* comp = tg + (size_t)(4 + c) * 100;
    double par[4], acc[4] = {0.0, 0.0, 0.0, 0.0}, dp[4];
    for (int k = 0; k < 4; ++k) par[k] = (dg[1 + k] >= 0) ? x[dg[1 + k]] : 0.0;
    for (int k = 0; k < 100; ++k) {
        pmap_fn_grad(dg[0], par, tg[k], dp);
        const double f = comp[k] / tg[200 + k];          // d u_k / d f_k = 1 / scaler scale_k
        for (int m = 0; m < 4; ++m) acc[m] = fma(f, dp[m], acc[m]);
    }
    for (int m = 0; m < 4; ++m)
        if (dg[1 + m] >= 0) Jr[dg[1 + m]] += acc[m];
}

// grad[w][q] (+)= sum_j (sum_p wmu[w][p] dmean[w][p][j] + wv[w][p] dvar[w][p][j]) J[w][j][q]   (J = identity: no map)
__global__ __launch_bounds__(256) void k_grad_fold(const double* __restrict__ wmu, const double* __restrict__ wv,
                                                   const double* __restrict__ dm, const double* __restrict__ dv, int P, int d,
                                                   const double* __restrict__ J, int nd, int64_t W, double* __restrict__ grad,
                                                   int accumulate) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= W * nd) return;
    const int64_t w = it / nd;
    const int q = (int)(it - w * nd);
    const double* a = wmu + w * P;
    const double* b = wv + w * P;
    double r = 0.0;
    for (int j = 0; j < d; ++j) {
        if (!J && j != q) continue;
        double gj = 0.0;
        for (int p = 0; p < P; ++p) {
            const int64_t o = (w * P + p) * d + j;
            gj = fma(a[p], dm[o], gj);
            gj = fma(b[p], dv[o], gj);
        }
        r = J ? fma(gj, J[(w * d + j) * nd + q], r) : gj;
    }
    grad[it] = accumulate ? grad[it] + r : r;
}

// jac[w][i][q] = sum_j (sum_p dy_i/dmu_p dmean[w][p][j]) J[w][j][q]; dy_i/dmu_p = A_pi (PCA), s_i [i = p] (no PCA), times y_i
// under the EXPDIAG modes
__global__ __launch_bounds__(256) void k_emu_jac(const double* __restrict__ mean_pc, int64_t Wld, const double* __restrict__ dm,
                                                 int P, int d, int M, int mode, const double* __restrict__ A,
                                                 const double* __restrict__ mu, const double* __restrict__ scale,
                                                 const double* __restrict__ J, int nd, int64_t W, double* __restrict__ jac) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= W * M * nd) return;
    const int64_t w = it / ((int64_t)M * nd);
    const int rem = (int)(it - w * M * nd), i = rem / nd, q = rem - i * nd;
    const bool no_pca = (mode == GPB_MODE_NO_PCA || mode == GPB_MODE_NO_PCA_EXPDIAG);
    const bool expdiag = (mode == GPB_MODE_EXPDIAG || mode == GPB_MODE_NO_PCA_EXPDIAG);
    double f = 1.0;
    if (expdiag) {
        double v;
        if (!no_pca) {
            v = 0.0;
            for (int p = 0; p < P; ++p) v = fma(mean_pc[(int64_t)p * Wld + w], A[p * M + i], v);
            v += mu[i];
        } else {
            v = mean_pc[(int64_t)i * Wld + w] * scale[i] + mu[i];
        }
        f = exp(v);
    }
    double r = 0.0;
    for (int j = 0; j < d; ++j) {
        if (!J && j != q) continue;
        double gj;
        if (!no_pca) {
            gj = 0.0;
            for (int p = 0; p < P; ++p) gj = fma(A[p * M + i], dm[(w * P + p) * d + j], gj);
        } else {
            gj = scale[i] * dm[(w * P + i) * d + j];
        }
        r = J ? fma(gj, J[(w * d + j) * nd + q], r) : gj;
    }
    jac[it] = f * r;
}

// rows outside the open box: zero gradient; rows whose log-posterior is NaN (a block not positive definite): NaN
__global__ void k_grad_finish(const double* __restrict__ X, int64_t W, int nd, const double* __restrict__ lo,
                              const double* __restrict__ hi, const double* __restrict__ ll, double* __restrict__ grad) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    bool inside = true;
    for (int q = 0; q < nd; ++q) {
        const double x = X[w * nd + q];
        inside = inside && (x > lo[q]) && (x < hi[q]);
    }
    const bool nanrow = isnan(ll[w]);
    for (int q = 0; q < nd; ++q) {
        double* g = grad + w * nd + q;
        if (!inside) *g = 0.0;
        else if (nanrow) *g = nan("");
    }
}

namespace {

// the pieces of one gradient evaluation of W rows, carved out of ctx->gbuf (GradWs, ws_layout.h)
int grad_ws(gpb_ctx* ctx, int64_t W, bool need_beta, bool need_like, int64_t n_out, GradWs& g) {
    const bool lw_global = need_like && like_w_doubles(ctx) > LIKE_W_LDS;
    return ctx_carve(ctx, ctx->gbuf, [&](Carver<double>& c) {
        g.lay(c, need_beta, ctx->P, round_up(W, WPAD), ctx->Np, W, ctx->d, sampler_ndim(ctx), ctx->pmap_d_in > 0,
              lw_global ? W * like_w_doubles(ctx) : 0, n_out);
    });
}

// K*^T (fp64) of the rows Xg[W][d], optionally the per-GP means / variances, then beta^T (need_beta) and the contraction into
// dmean / dvar [W][P][d]
int gp_grad_rows(gpb_ctx* ctx, const double* Xg, int64_t W, bool need_var, bool need_mv, double* bt, double* dmean, double* dvar) {
    int rc;
    ctx->want_kst = true;                       // the fp64 K*^T itself, whatever predict arithmetic the context has selected
    rc = need_mv ? launch_predict(ctx, Xg, W, true) : launch_kcross(ctx, Xg, W, nullptr, false);
    ctx->want_kst = false;
    if (rc) return rc;
    const int64_t Wld = ctx->Wld, Np = ctx->Np;
    if (need_var) {
        if ((rc = launch_vmat(ctx))) return rc;
        hipLaunchKernelGGL(k_betaT, dim3((unsigned)((Np + 127) / 128), (unsigned)(Wld / 128), (unsigned)ctx->P), dim3(256), 0,
                           ctx->stream, ctx->vbuf, ctx->Linv, bt, Np, Wld);
    }
    const dim3 grid((unsigned)W, (unsigned)ctx->P);
    const int64_t pad = pad_front(Np, ctx->N);
    rc = with_kind(ctx->kind, [&](auto K) {
        hipLaunchKernelGGL(k_gp_grad<decltype(K)::value>, grid, dim3(256), 0, ctx->stream, Xg, ctx->d, ctx->X, (int)ctx->dpad, ctx->ls,
                           ctx->amp, ctx->alpha, need_var ? bt : nullptr, Np, pad, ctx->N, (int)ctx->d, (int)ctx->P, Wld, dmean,
                           need_var ? dvar : nullptr);
        return 0;
    });
    if (rc) return dispatched(ctx, rc, "k_gp_grad");
    GPB_HIP(hipGetLastError());
    return 0;
}

int launch_pmap_jac(gpb_ctx* ctx, const double* X, int64_t W, double* J) {
    const int64_t n = W * ctx->pmap_d_out;
    hipLaunchKernelGGL(k_pmap_jac, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, X, W, (int)ctx->pmap_d_in,
                       (int)ctx->pmap_d_out, ctx->pmap_int, ctx->pmap_maxpc, ctx->pmap_int + ctx->pmap_d_out, ctx->pmap_tab, J);
    GPB_HIP(hipGetLastError());
    return 0;
}

int grad_state_check(gpb_ctx* ctx, const char* who) {
    if (ctx->multi) GPB_FAIL(GPB_E_STATE, std::string(who) + ": a gpb_gp_set_multi context is fit-only");
    if (!ctx->factored) GPB_FAIL(GPB_E_STATE, std::string(who) + " before gpb_gp_factor");
    if (ctx->d > MAX_D) GPB_FAIL(GPB_E_ARG, std::string(who) + ": more than 64 GP inputs");
    return 0;
}

}  // namespace
}  // namespace gpb

using namespace gpb;

extern "C" int gpb_gp_predict_grad(gpb_ctx* ctx, const double* Xs, int64_t W, int on_device, double* dmean, double* dvar) {
    if (!ctx || !Xs || !dmean || W < 0) return GPB_E_ARG;
    int rc = grad_state_check(ctx, "gpb_gp_predict_grad");
    if (rc) return rc;
    if (W == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    if ((rc = ensure_wcap(ctx, W))) return rc;
    const int64_t n = W * ctx->P * ctx->d;
    GradWs g;
    if ((rc = grad_ws(ctx, W, dvar != nullptr, false, on_device ? 0 : 2 * n, g))) return rc;
    HostOut so(ctx, on_device != 0);
    const double* X;
    if ((rc = so.in_at(X, Xs, g.xin, W * ctx->d))) return rc;
    double* om = so.at(dmean, g.out, n);
    double* ov = so.at(dvar, g.out ? g.out + n : nullptr, n);
    if ((rc = gp_grad_rows(ctx, X, W, dvar != nullptr, false, g.bt, om, ov))) return rc;
    return so.finish();
}

extern "C" int gpb_emu_predict_jac(gpb_ctx* ctx, const double* Xs, int64_t W, int on_device, double* jac) {
    if (!ctx || !Xs || !jac || W < 0) return GPB_E_ARG;
    int rc = grad_state_check(ctx, "gpb_emu_predict_jac");
    if (rc) return rc;
    if (!ctx->have_transform) GPB_FAIL(GPB_E_STATE, "gpb_emu_predict_jac before gpb_emu_set_transform");
    if (W == 0) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    if ((rc = ensure_wcap(ctx, W))) return rc;
    const int64_t din = sampler_ndim(ctx), n = W * ctx->M * din;
    GradWs g;
    if ((rc = grad_ws(ctx, W, false, false, on_device ? 0 : n, g))) return rc;
    HostOut so(ctx, on_device != 0);
    const double* X;
    if ((rc = so.in_at(X, Xs, g.xin, W * din))) return rc;
    const double* Xg = X;
    if (ctx->pmap_d_in > 0) {
        if ((rc = gpb_param_map(ctx, X, W, g.xg))) return rc;
        if ((rc = launch_pmap_jac(ctx, X, W, g.jm))) return rc;
        Xg = g.xg;
    }
    if ((rc = gp_grad_rows(ctx, Xg, W, false, true, nullptr, g.dm, nullptr))) return rc;
    double* o = so.at(jac, g.out, n);
    hipLaunchKernelGGL(k_emu_jac, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->mean_pc, ctx->Wld, g.dm,
                       (int)ctx->P, (int)ctx->d, (int)ctx->M, ctx->mode, ctx->A, ctx->mu, ctx->scale,
                       ctx->pmap_d_in > 0 ? g.jm : nullptr, (int)din, W, o);
    GPB_HIP(hipGetLastError());
    return so.finish();
}

extern "C" int gpb_chain_logpost_grad(gpb_ctx* const* ctxs, int E, const double* Xs_dev, int64_t W, double* ll_dev,
                                      double* grad_dev, const double* lo_dev, const double* hi_dev, double outside_value,
                                      double inside_const) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* c0 = ctxs[0];
    gpb_ctx* ctx = c0;                          // (the error macros report on it)
    if (!Xs_dev || !ll_dev || !grad_dev || !lo_dev || !hi_dev || W < 0)
        GPB_FAIL(GPB_E_ARG, "gpb_chain_logpost_grad: null pointer or negative size");
    int rc;
    for (int e = 0; e < E; ++e)                 // (first: a fit-only context has no likelihood either, and says which it is)
        if (ctxs[e] && (rc = grad_state_check(ctxs[e], "gpb_chain_logpost_grad"))) { c0->err = ctxs[e]->err; return rc; }
    if ((rc = chain_ctx_check(ctxs, E, "gpb_chain_logpost_grad"))) return rc;
    if (W == 0) return 0;
    GPB_HIP(hipSetDevice(c0->device));
    const int64_t nd = sampler_ndim(c0);
    GradWs ws[MAX_CHAIN_CTX];
    for (int e = 0; e < E; ++e) {
        if ((rc = ensure_wcap(ctxs[e], W)) || (rc = grad_ws(ctxs[e], W, true, true, 0, ws[e]))) {
            c0->err = ctxs[e]->err;
            return rc;
        }
    }
    // the log-posterior, as every sampler evaluates it
    if ((rc = chain_eval(ctxs, E, Xs_dev, W, ll_dev, lo_dev, hi_dev, outside_value, inside_const))) return rc;
    // A coupled chain (gpb_chain_like_set; chain_eval has checked the coupling): the likelihood's weights of all emulators come
    // from ONE factorisation per row, so first every emulator's GP derivatives, means and variances, then the joint launch, then
    // the folds in emuList order.
    if (coupling_installed(c0)) {
        double *wmu[MAX_CHAIN_CTX], *wv[MAX_CHAIN_CTX];
        for (int e = 0; e < E; ++e) {
            gpb_ctx* c = ctxs[e];
            GradWs& g = ws[e];
            const double* Xg = Xs_dev;
            if (c->pmap_d_in > 0) {
                if ((rc = gpb_param_map(c, Xs_dev, W, g.xg)) || (rc = launch_pmap_jac(c, Xs_dev, W, g.jm))) { c0->err = c->err; return rc; }
                Xg = g.xg;
            }
            if ((rc = gp_grad_rows(c, Xg, W, true, true, g.bt, g.dm, g.dv))) { c0->err = c->err; return rc; }
            wmu[e] = g.wmu;
            wv[e] = g.wv;
        }
        if ((rc = launch_like_w_coupled(ctxs, E, W, wmu, wv))) return rc;
        const int64_t n = W * nd;
        for (int e = 0; e < E; ++e) {
            gpb_ctx* c = ctxs[e];
            GradWs& g = ws[e];
            hipLaunchKernelGGL(k_grad_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, g.wmu, g.wv, g.dm, g.dv,
                               (int)c->P, (int)c->d, c->pmap_d_in > 0 ? g.jm : nullptr, (int)nd, W, grad_dev, e > 0 ? 1 : 0);
        }
        hipLaunchKernelGGL(k_grad_finish, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, c0->stream, Xs_dev, W, (int)nd, lo_dev,
                           hi_dev, ll_dev, grad_dev);
        GPB_HIP(hipGetLastError());
        return 0;
    }
    // the gradient, emulator after emulator (fp64 throughout), added up in emuList order
    for (int e = 0; e < E; ++e) {
        gpb_ctx* c = ctxs[e];
        GradWs& g = ws[e];
        const double* Xg = Xs_dev;
        const bool mapped = c->pmap_d_in > 0;
        if (mapped) {
            if ((rc = gpb_param_map(c, Xs_dev, W, g.xg)) || (rc = launch_pmap_jac(c, Xs_dev, W, g.jm))) { c0->err = c->err; return rc; }
            Xg = g.xg;
        }
        if ((rc = gp_grad_rows(c, Xg, W, true, true, g.bt, g.dm, g.dv))) { c0->err = c->err; return rc; }
        const int64_t nw = like_w_doubles(c);
        const bool glob = nw > LIKE_W_LDS;
        hipLaunchKernelGGL(k_like_w, dim3((unsigned)W), dim3(256), glob ? 0 : (size_t)nw * sizeof(double), c->stream, c->mean_pc,
                           c->var_pc, c->Wld, (int)c->P, (int)c->M, c->mode, c->A, c->mu, c->scale, c->C0, c->yexp, c->Cexp,
                           g.wmu, g.wv, glob ? g.lw : nullptr, nw);
        const int64_t n = W * nd;
        hipLaunchKernelGGL(k_grad_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, g.wmu, g.wv, g.dm, g.dv,
                           (int)c->P, (int)c->d, mapped ? g.jm : nullptr, (int)nd, W, grad_dev, e > 0 ? 1 : 0);
        if (hipGetLastError() != hipSuccess) GPB_FAIL(GPB_E_HIP, "gpb_chain_logpost_grad: kernel launch failed");
    }
    hipLaunchKernelGGL(k_grad_finish, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, c0->stream, Xs_dev, W, (int)nd, lo_dev,
                       hi_dev, ll_dev, grad_dev);
    GPB_HIP(hipGetLastError());
    return 0;
}
