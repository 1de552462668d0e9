// gpb_design.hip — variance-reduction sequential design (gpb_design_begin, gpb_chain_design_run, gpb_design_end): where the next
// model runs go, from what is already resident (X, theta, L^-1).  No training output enters.
//
// For GP p: v(a) = L^-1 k(X, a) and the posterior covariance of the latent function s(a, b) = c k(a, b) - v(a)^T v(b) (no White
// term).  A run at x, observed with the training runs' noise tau = sigma_n^2 + alpha — or, after gpb_design_set_noise, with candidate
// c's own tau_p(c) = sigma_n^2 + (alpha + s_c[p][c]), the sum alpha + s first as on the training diagonal — conditions every GP:
//     s'(a, b) = s(a, b) - s(a, x) s(x, b) / (s(x, x) + tau)
// and lowers the reference-averaged variance sum_p g_p sum_r w_r s_p(r, r) by
//     J(x) = sum_p g_p [sum_r w_r s_p(r, x)^2] / (s_p(x, x) + tau_p)                     (active learning Cohn; Seo et al. 2000)
// The greedy loop picks the eligible candidate with the largest J (lowest index on ties) and conditions on it, T times.
//
// gpb_design_begin, per context:
//   k_kcross + k_vmat (gpb_predict.hip, gpb_cov.hip)   V_c [P][Np][Cp] and V_r [P][Np][Rp], C and R padded to 128
//   k_design_kern   S[p][r][c] = c k(x_r, x_c), exact zeros in the padding
//   k_design_gemm   S[p] -= V_r^T V_c: fp64 MFMA TN product (gemm_tile.h) over the design's rows; the front padding rows are left
//                   out of the k range, the few behind are exact zeros of V
//   k_design_diag   s(c, c) = c - sum_n V_c[n][c]^2
// gpb_chain_design_run enqueues, per pick t, with no host synchronisation:
//   k_design_score    per context: one pass over S that applies the pending downdate S -= u_r u_c^T of pick t - 1 in place and leaves
//                     sum_r w_r S^2 per column and 128-row chunk
//   k_design_combine  per context: J_e[c] = sum_p g_p (chunks in order) / (s_p(c, c) + tau_p), GPs in index order
//   k_design_pick     one workgroup: J = J_1 + J_2 + ... in emuList order, eligibility, scores row, arg-max; the index stays on the device
//   k_design_ur       per context: u_r = S[:, c*] / sqrt(den), den = s(c*, c*) + tau (kept for k_design_row)
//   k_design_row      per context: the pick's covariance row c k(x_c*, x_c) - V_c[:, c*]^T V_c - sum_{i<t} u_i(c*) u_i against all
//                     candidates (a GEMV over Np plus the earlier picks), u_c = row / sqrt(den), s(c, c) -= u_c^2
// No floating-point atomics; every sum runs in an order fixed by the padded shapes (Np, Cp, Rp) alone; no [C, C] matrix exists.
#include "gpb_internal.h"
#include "gemm_tile.h"
#include <math.h>

namespace gpb {

namespace {

constexpr int64_t DS_MAX_POINTS = 8192;   // candidates / reference points of one call
constexpr int DS_MAX_CTX = 32;            // contexts of one chain call (k_design_pick's table is a kernel argument)
constexpr int DS_RCH = 128;               // reference rows per chunk partial of k_design_score

// squared scaled distance in the difference form sklearn's cdist takes (as k_kss)
__device__ __forceinline__ double design_r2(const double* __restrict__ xa, const double* __restrict__ xb, const double* __restrict__ l, int d) {
    double r2 = 0.0;
    for (int k = 0; k < d; ++k) {
        const double df = xa[k] / l[k] - xb[k] / l[k];
        r2 = fma(df, df, r2);
    }
    return r2;
}

// S[p][r][c] = c_p k_p(x_r, x_c) inside [R, C], 0 in the padding
template <int KIND>
__global__ __launch_bounds__(256) void k_design_kern(const double* __restrict__ Xr, int R, const double* __restrict__ Xc, int C, int d,
                                                     const double* __restrict__ ls, int dpad, const double* __restrict__ amp,
                                                     double* __restrict__ S, int64_t Rp, int64_t Cp) {
    const int p = blockIdx.z;
    const int64_t r = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4), c = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
    double v = 0.0;
    if (r < R && c < C) v = amp[p] * shape_fn<KIND>(design_r2(Xr + r * d, Xc + c * d, ls + p * dpad, d));
    S[((int64_t)p * Rp + r) * Cp + c] = v;
}

// S[p] -= V_r[p]^T V_c[p] over the rows [k0, Np) of V; only the [R, C] corner is written
__global__ __launch_bounds__(256, 2) void k_design_gemm(const double* __restrict__ Vr, const double* __restrict__ Vc,
                                                        double* __restrict__ S, int64_t Np, int64_t k0, int64_t Rp, int64_t Cp, int R,
                                                        int C) {
    __shared__ TileLds<128> lds;
    const int p = blockIdx.z;
    const int64_t mb = (int64_t)blockIdx.y * 128, nb = (int64_t)blockIdx.x * 128;
    Acc<128> acc;
    acc_zero<128>(acc);
    gemm_tile_loop<128, true, false>(Vr + (int64_t)p * Np * Rp, Rp, Vc + (int64_t)p * Np * Cp, Cp, mb, nb, 128, 128, k0, Np, lds, acc);
    tile_store<128>(S + (int64_t)p * Rp * Cp, Cp, mb, nb, (int)imin64(128, R - mb), (int)imin64(128, C - nb), -1.0, true, acc);
}

// sum_n V[n][cs] V[n][c] over the rows [k0, Np) for 64 columns c: the four waves take the rows n = k0 + wave (mod 4), their sums are
// added in wave order.  cs < 0: the column itself.  The result is valid in wave 0.
__device__ __forceinline__ double design_coldot(const double* __restrict__ V, int64_t ld, int64_t k0, int64_t k1, int64_t cs, int64_t c,
                                                double (*sh)[64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a = 0.0;
#pragma unroll 4
    for (int64_t n = k0 + wave; n < k1; n += 4) {
        const double x = V[n * ld + c];
        a = fma(cs < 0 ? x : V[n * ld + cs], x, a);
    }
    __syncthreads();                                   // (a previous use of sh is done)
    sh[wave][lane] = a;
    __syncthreads();
    return ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

// dg[p][c] = s_p(c, c) = c_p - sum_n V_c[n][c]^2   (1 in the padding)
__global__ __launch_bounds__(256) void k_design_diag(const double* __restrict__ Vc, const double* __restrict__ amp, double* __restrict__ dg,
                                                     int64_t Np, int64_t k0, int64_t Cp, int C) {
    __shared__ double sh[4][64];
    const int p = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const double s = design_coldot(Vc + (int64_t)p * Np * Cp, Cp, k0, Np, -1, c, sh);
    if (threadIdx.x < 64) dg[(int64_t)p * Cp + c] = c < C ? amp[p] - s : 1.0;
}

// One pass over S[p]: the pending downdate S -= u_r u_c^T (PENDING) in place, then part[p][chunk][c] = sum over the chunk's 128 rows
// of w_r S[r][c]^2 — thread = column, the two halves of the workgroup take 64 rows each, in row order, first half + second half.
// The padding of S, u_r, u_c and w is zeros: no bounds enter.
template <bool PENDING>
__global__ __launch_bounds__(256) void k_design_score(double* __restrict__ S, const double* __restrict__ ur, const double* __restrict__ uc,
                                                      const double* __restrict__ w, double* __restrict__ part, int64_t Rp, int64_t Cp) {
    __shared__ double sh[128];
    const int p = blockIdx.z, half = threadIdx.x >> 7;
    const int64_t c = (int64_t)blockIdx.x * 128 + (threadIdx.x & 127), r0 = (int64_t)blockIdx.y * DS_RCH + half * 64;
    double* Sp = S + ((int64_t)p * Rp + r0) * Cp + c;
    const double* urp = ur + (int64_t)p * Rp + r0;
    const double ucc = PENDING ? uc[(int64_t)p * Cp + c] : 0.0;
    double acc = 0.0;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
        double s = Sp[(int64_t)j * Cp];
        if (PENDING) {
            s = fma(-urp[j], ucc, s);
            Sp[(int64_t)j * Cp] = s;
        }
        acc = fma(w[r0 + j] * s, s, acc);
    }
    if (half) sh[threadIdx.x & 127] = acc;
    __syncthreads();
    if (!half) part[((int64_t)p * gridDim.y + blockIdx.y) * Cp + c] = acc + sh[threadIdx.x];
}

// J[c] = sum_p g_p [sum_chunks part[p][chunk][c]] / (dg[p][c] + tau_p): chunks, then GPs, in index order; a GP of weight 0 is left out.
// sc (gpb_design_set_noise, or nullptr): the candidates' simulation noise [P][Cp], tau_p(c) = sigma_n^2 + (alpha + sc[p][c]).
__global__ __launch_bounds__(256) void k_design_combine(const double* __restrict__ part, const double* __restrict__ dg,
                                                        const double* __restrict__ g, const double* __restrict__ noise, double alpha_reg,
                                                        const double* __restrict__ sc, int P, int nch, int64_t Cp, int C,
                                                        double* __restrict__ J) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= Cp) return;
    double j = 0.0;
    if (c < C) {
        for (int p = 0; p < P; ++p) {
            if (g[p] == 0.0) continue;
            double q = 0.0;
            for (int ch = 0; ch < nch; ++ch) q += part[((int64_t)p * nch + ch) * Cp + c];
            const double a = sc ? alpha_reg + sc[(int64_t)p * Cp + c] : alpha_reg;
            j += g[p] * (q / (dg[(int64_t)p * Cp + c] + (noise[p] + a)));
        }
    }
    J[c] = j;
}

struct DesignTab {
    const double* J[DS_MAX_CTX];
    int E;
};

// One workgroup: J = J_1 + J_2 + ... in table order, the scores row (-inf where ineligible), the eligible arg-max with the lowest
// index on ties (a NaN score ranks as -inf), then picks[t], gain[t], *pick and the cleared eligibility flag.  Nothing eligible:
// the pick is -1, the gain NaN, and the kernels behind leave a zero downdate.
__global__ __launch_bounds__(1024) void k_design_pick(const DesignTab tab, int C, uint8_t* __restrict__ elig, int t, int* __restrict__ pick,
                                                      int32_t* __restrict__ picks, double* __restrict__ gain, double* __restrict__ scores) {
    __shared__ double sv[1024], sk[1024];
    __shared__ int si[1024];
    const int tid = threadIdx.x;
    const double ninf = -__builtin_inf();
    double bk = ninf, bv = 0.0;
    int bi = -1;
    for (int c = tid; c < C; c += 1024) {
        double j = tab.J[0][c];
        for (int e = 1; e < tab.E; ++e) j += tab.J[e][c];
        const bool el = elig[c] != 0;
        if (scores) scores[(int64_t)t * C + c] = el ? j : ninf;
        const double key = j == j ? j : ninf;
        if (el && (bi < 0 || key > bk)) { bk = key; bv = j; bi = c; }
    }
    sk[tid] = bk; sv[tid] = bv; si[tid] = bi;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) {
            const int oi = si[tid + s];
            const double ok = sk[tid + s];
            // (indices of the upper half are not ordered against the lower half's: compare them)
            if (oi >= 0 && (si[tid] < 0 || ok > sk[tid] || (ok == sk[tid] && oi < si[tid]))) {
                sk[tid] = ok; sv[tid] = sv[tid + s]; si[tid] = oi;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int b = si[0];
        *pick = b;
        picks[t] = b;
        gain[t] = b >= 0 ? sv[0] : __builtin_nan("");
        if (b >= 0) elig[b] = 0;
    }
}

// u_r[p][r] = S[p][r][c*] / sqrt(den_p), den_p = s_p(c*, c*) + tau_p, kept in den[p] for k_design_row (which changes s(c*, c*))
__global__ __launch_bounds__(256) void k_design_ur(const double* __restrict__ S, const double* __restrict__ dg, const double* __restrict__ noise,
                                                   double alpha_reg, const double* __restrict__ sc, const int* __restrict__ pick,
                                                   int64_t Rp, int64_t Cp, int R, double* __restrict__ ur, double* __restrict__ den) {
    const int p = blockIdx.y, cs = *pick;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= Rp) return;
    double u = 0.0, dn = 1.0;
    if (cs >= 0) {
        const double a = sc ? alpha_reg + sc[(int64_t)p * Cp + cs] : alpha_reg;
        dn = dg[(int64_t)p * Cp + cs] + (noise[p] + a);
        if (r < R) u = S[((int64_t)p * Rp + r) * Cp + cs] / sqrt(dn);
    }
    ur[(int64_t)p * Rp + r] = u;
    if (r == 0) den[p] = dn;
}

// The pick's covariance row against 64 candidates per workgroup, scaled: U[t][p][c] = u_c = s^(t)(c*, c) / sqrt(den_p), and the
// diagonal's downdate s(c, c) -= u_c^2.  The sums over the design's rows and over the earlier picks each take design_coldot's order.
template <int KIND>
__global__ __launch_bounds__(256) void k_design_row(const double* __restrict__ Vc, double* __restrict__ U, const double* __restrict__ Xc,
                                                    const double* __restrict__ ls, const double* __restrict__ amp,
                                                    const double* __restrict__ den, const int* __restrict__ pick, double* __restrict__ dg,
                                                    int64_t Np, int64_t k0, int64_t Cp, int C, int d, int dpad, int P, int t) {
    __shared__ double sh[4][64];
    const int p = blockIdx.y, cs = *pick;
    const int64_t c = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    double* Ut = U + ((int64_t)t * P + p) * Cp;
    if (cs < 0) {
        if (threadIdx.x < 64) Ut[c] = 0.0;
        return;
    }
    const double sv = design_coldot(Vc + (int64_t)p * Np * Cp, Cp, k0, Np, cs, c, sh);
    // the earlier picks' rows: U[i][p][.] for i < t are Cp apart by P * Cp
    const double su = design_coldot(U + (int64_t)p * Cp, (int64_t)P * Cp, 0, t, cs, c, sh);
    if (threadIdx.x >= 64) return;
    double u = 0.0;
    if (c < C) {
        const double k = amp[p] * shape_fn<KIND>(design_r2(Xc + (int64_t)cs * d, Xc + c * d, ls + p * dpad, d));
        u = ((k - sv) - su) / sqrt(den[p]);
        dg[(int64_t)p * Cp + c] = fma(-u, u, dg[(int64_t)p * Cp + c]);
    }
    Ut[c] = u;
}

static_assert(WS_PAD == WPAD, "the design layouts pad to the walker-batch granule");
// the pieces of the begin block (DesignWs, ws_layout.h) in a context's design_ws as it stands
DesignWs design_layout(const gpb_ctx* ctx, int64_t C, int64_t R) {
    DesignWs L;
    Carver<double> c(ctx->design_ws.get());
    L.lay(c, C, R, ctx->d, ctx->P, ctx->Np);
    return L;
}

}  // namespace

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_design_begin(gpb_ctx* ctx, const double* Xc_dev, int64_t C, const double* Xr_dev, int64_t R, const double* w_dev,
                                const double* g_host) {
    if (!ctx) return GPB_E_ARG;
    ctx->design_ready = ctx->design_noise = false;
    if (ctx->N == 0) GPB_FAIL(GPB_E_STATE, "gpb_design_begin before gpb_gp_set");
    if (ctx->multi) GPB_FAIL(GPB_E_STATE, "gpb_design_begin: a gpb_gp_set_multi context is fit-only (its GPs have different designs)");
    if (!ctx->factored) GPB_FAIL(GPB_E_STATE, "gpb_design_begin before gpb_gp_factor");
    if (!Xc_dev || !Xr_dev || !w_dev || !g_host) GPB_FAIL(GPB_E_ARG, "gpb_design_begin: null pointer");
    if (C < 1 || R < 1 || C > DS_MAX_POINTS || R > DS_MAX_POINTS)
        GPB_FAIL(GPB_E_ARG, "gpb_design_begin: need 1 <= C, R <= 8192 candidates / reference points");
    const int64_t P = ctx->P, Np = ctx->Np, d = ctx->d;
    for (int64_t p = 0; p < P; ++p)
        if (!(g_host[p] >= 0.0)) GPB_FAIL(GPB_E_ARG, "gpb_design_begin: a GP weight g is negative (or NaN)");
    if (P > 65535) GPB_FAIL(GPB_E_ARG, "gpb_design_begin: more than 65535 GPs");
    GPB_HIP(hipSetDevice(ctx->device));
    DesignWs L;
    int rc;
    if ((rc = ctx_carve(ctx, ctx->design_ws, [&](Carver<double>& c) { L.lay(c, C, R, d, P, Np); }))) return rc;
    if ((rc = ensure_wcap(ctx, C > R ? C : R))) return rc;
    hipStream_t st = ctx->stream;
    GPB_HIP(hipMemcpyAsync(L.xc, Xc_dev, sizeof(double) * (size_t)(C * d), hipMemcpyDeviceToDevice, st));
    GPB_HIP(hipMemcpyAsync(L.xr, Xr_dev, sizeof(double) * (size_t)(R * d), hipMemcpyDeviceToDevice, st));
    GPB_HIP(hipMemsetAsync(L.w, 0, sizeof(double) * (size_t)L.Rp, st));
    GPB_HIP(hipMemcpyAsync(L.w, w_dev, sizeof(double) * (size_t)R, hipMemcpyDeviceToDevice, st));
    GPB_HIP(hipMemcpyAsync(L.g, g_host, sizeof(double) * (size_t)P, hipMemcpyHostToDevice, st));
    GPB_HIP(hipStreamSynchronize(st));                 // (g_host is the caller's)
    // V = L^-1 K*^T of the two point sets through the predict path's cross kernel (fp64 K*^T) and the joint covariance's k_vmat
    ctx->want_kst = true;
    rc = launch_kcross(ctx, L.xc, C, nullptr);
    if (!rc) rc = launch_vmat(ctx, L.vc);
    if (!rc) rc = launch_kcross(ctx, L.xr, R, nullptr);
    if (!rc) rc = launch_vmat(ctx, L.vr);
    ctx->want_kst = false;
    if (rc) return rc;
    const int64_t k0 = pad_front(Np, ctx->N);          // a multiple of the GEMM's K-step
    const dim3 gk((unsigned)(L.Cp / 16), (unsigned)(L.Rp / 16), (unsigned)P);
    rc = with_kind(ctx->kind, [&](auto K) {
        hipLaunchKernelGGL(k_design_kern<decltype(K)::value>, gk, dim3(256), 0, st, L.xr, (int)R, L.xc, (int)C, (int)d, ctx->ls,
                           (int)ctx->dpad, ctx->amp, L.s, L.Rp, L.Cp);
        return 0;
    });
    if (rc) return dispatched(ctx, rc, "k_design_kern");
    hipLaunchKernelGGL(k_design_gemm, dim3((unsigned)(L.Cp / 128), (unsigned)(L.Rp / 128), (unsigned)P), dim3(256), 0, st, L.vr,
                       L.vc, L.s, Np, k0, L.Rp, L.Cp, (int)R, (int)C);
    hipLaunchKernelGGL(k_design_diag, dim3((unsigned)(L.Cp / 64), (unsigned)P), dim3(256), 0, st, L.vc, ctx->amp, L.dg, Np, k0,
                       L.Cp, (int)C);
    GPB_HIP(hipGetLastError());
    ctx->design_C = C;
    ctx->design_R = R;
    ctx->design_ready = true;
    return 0;
}

extern "C" int gpb_design_set_noise(gpb_ctx* ctx, const double* s_c_dev) {
    if (!ctx) return GPB_E_ARG;
    if (!ctx->design_ready) GPB_FAIL(GPB_E_STATE, "gpb_design_set_noise before gpb_design_begin (or after the run that consumed it)");
    if (!s_c_dev) {                                    // back to the training runs' tau_p
        ctx->design_noise = false;
        return 0;
    }
    GPB_HIP(hipSetDevice(ctx->device));
    const int64_t C = ctx->design_C, P = ctx->P;
    const DesignWs L = design_layout(ctx, C, ctx->design_R);
    double* sc = L.sc;
    GPB_HIP(hipMemsetAsync(sc, 0, sizeof(double) * (size_t)(P * L.Cp), ctx->stream));
    GPB_HIP(hipMemcpy2DAsync(sc, sizeof(double) * (size_t)L.Cp, s_c_dev, sizeof(double) * (size_t)C, sizeof(double) * (size_t)C, (size_t)P,
                             hipMemcpyDeviceToDevice, ctx->stream));
    ctx->design_noise = true;
    return 0;
}

extern "C" int gpb_chain_design_run(gpb_ctx* const* ctxs, int E, int64_t T, uint8_t* eligible_dev, int32_t* picks_dev, double* gain_dev,
                                    double* scores_dev) {
    if (!ctxs || E < 1 || !ctxs[0]) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    if (E > DS_MAX_CTX) GPB_FAIL(GPB_E_ARG, "gpb_chain_design_run: more than 32 contexts");
    for (int e = 0; e < E; ++e) {
        const gpb_ctx* c = ctxs[e];
        if (!c) GPB_FAIL(GPB_E_ARG, "gpb_chain_design_run: null context");
        if (c->device != ctx->device || c->stream != ctx->stream)
            GPB_FAIL(GPB_E_ARG, "gpb_chain_design_run: the contexts must share one device and one stream");
        if (!c->factored) GPB_FAIL(GPB_E_STATE, "gpb_chain_design_run before gpb_gp_factor");
        if (!c->design_ready)
            GPB_FAIL(GPB_E_STATE, "gpb_chain_design_run before gpb_design_begin (a run conditions the workspace in place: begin again for another)");
        if (c->design_C != ctx->design_C || c->design_R != ctx->design_R)
            GPB_FAIL(GPB_E_STATE, "gpb_chain_design_run: the contexts were begun with different numbers of candidates or reference points");
    }
    const int64_t C = ctx->design_C, R = ctx->design_R;
    if (!picks_dev || !gain_dev) GPB_FAIL(GPB_E_ARG, "gpb_chain_design_run: null pointer");
    if (T < 1) GPB_FAIL(GPB_E_ARG, "gpb_chain_design_run: need T >= 1 picks");
    if (T > C) GPB_FAIL(GPB_E_ARG, "gpb_chain_design_run: more picks than candidates");
    GPB_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t Cp = round_up(C, WPAD), Rp = round_up(R, WPAD);
    const int nch = (int)(Rp / DS_RCH);
    DesignRun run[DS_MAX_CTX];      // per context (ws_layout.h); the first context's also holds the pick and the flags
    DesignTab tab;
    tab.E = E;
    for (int e = 0; e < E; ++e) {
        gpb_ctx* c = ctxs[e];
        if (const int rc = ctx_carve(c, c->design_run, [&](Carver<double>& cv) { run[e].lay(cv, T, c->P, Cp, Rp, nch, e == 0); })) {
            ctx->err = c->err;
            return rc;
        }
        tab.J[e] = run[e].J;
    }
    int* pick = run[0].pick;
    uint8_t* elig = eligible_dev;
    if (!elig) {
        elig = run[0].elig;
        GPB_HIP(hipMemsetAsync(elig, 1, (size_t)C, st));
    }
    for (int64_t t = 0; t < T; ++t) {
        for (int e = 0; e < E; ++e) {
            gpb_ctx* c = ctxs[e];
            const DesignWs L = design_layout(c, C, R);
            const int P = (int)c->P;
            const dim3 gs((unsigned)(Cp / 128), (unsigned)nch, (unsigned)P);
            if (t == 0)
                hipLaunchKernelGGL(k_design_score<false>, gs, dim3(256), 0, st, L.s, run[e].ur, run[e].U, L.w, run[e].part, Rp, Cp);
            else
                hipLaunchKernelGGL(k_design_score<true>, gs, dim3(256), 0, st, L.s, run[e].ur, run[e].U + (t - 1) * P * Cp, L.w,
                                   run[e].part, Rp, Cp);
            hipLaunchKernelGGL(k_design_combine, dim3((unsigned)((Cp + 255) / 256)), dim3(256), 0, st, run[e].part, L.dg, L.g,
                               c->noise, c->alpha_reg, c->design_noise ? L.sc : nullptr, P, nch, Cp, (int)C, run[e].J);
        }
        hipLaunchKernelGGL(k_design_pick, dim3(1), dim3(1024), 0, st, tab, (int)C, elig, (int)t, pick, picks_dev, gain_dev, scores_dev);
        if (t + 1 == T) break;                         // (nothing reads the last pick's downdate)
        for (int e = 0; e < E; ++e) {
            gpb_ctx* c = ctxs[e];
            const DesignWs L = design_layout(c, C, R);
            const int P = (int)c->P;
            const int64_t k0 = pad_front(c->Np, c->N);
            hipLaunchKernelGGL(k_design_ur, dim3((unsigned)((Rp + 255) / 256), (unsigned)P), dim3(256), 0, st, L.s, L.dg, c->noise,
                               c->alpha_reg, c->design_noise ? L.sc : nullptr, pick, Rp, Cp, (int)R, run[e].ur, run[e].den);
            const dim3 gr((unsigned)(Cp / 64), (unsigned)P);
            const int rc = with_kind(c->kind, [&](auto K) {
                hipLaunchKernelGGL(k_design_row<decltype(K)::value>, gr, dim3(256), 0, st, L.vc, run[e].U, L.xc, c->ls, c->amp,
                                   run[e].den, pick, L.dg, c->Np, k0, Cp, (int)C, (int)c->d, (int)c->dpad, P, (int)t);
                return 0;
            });
            if (rc) return dispatched(ctx, rc, "k_design_row");
        }
    }
    for (int e = 0; e < E; ++e) ctxs[e]->design_ready = false;     // S and s(c, c) are conditioned on the picks now
    GPB_HIP(hipGetLastError());
    return 0;
}

extern "C" int gpb_design_end(gpb_ctx* ctx) {
    if (!ctx) return GPB_E_ARG;
    ctx->design_ready = ctx->design_noise = false;
    ctx->design_C = ctx->design_R = 0;
    if (!ctx->design_ws && !ctx->design_run) return 0;
    GPB_HIP(hipSetDevice(ctx->device));
    GPB_HIP(hipStreamSynchronize(ctx->stream));
    ctx->design_ws.release();
    ctx->design_run.release();
    return 0;
}
