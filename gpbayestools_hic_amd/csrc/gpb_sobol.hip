// gpb_sobol.hip — closed-form Sobol sensitivity indices and main-effect curves of the posterior mean (gpb_gp_sobol, gpb_emu_sobol,
// gpb_emu_main_effect).  RBF kernel, uniform prior box [lo, hi], widths w = hi - lo (Oakley & O'Hagan 2004).
//
// GP p has the mean m_p(x) = c_p sum_i alpha_pi prod_l exp(-(x_l - x_il)^2 / 2 l_pl^2).  With a = x_il, b = x_i'l, l = l_pl, l' = l_ql:
//     I^p_l(a)     = l sqrt(pi/2) / w_l [erf((hi_l - a) / (sqrt2 l)) - erf((lo_l - a) / (sqrt2 l))]               the box average of one factor
//     Q^pq_l(a, b) = exp(-(a - b)^2 / 2(l^2 + l'^2)) sqrt(pi / 2s) / w_l [erf((hi_l - c) sqrt(s/2)) - erf((lo_l - c) sqrt(s/2))]
//                    s = 1/l^2 + 1/l'^2, c = (a/l^2 + b/l'^2) / s                                                  of a product of two
//     e_p    = c_p sum_i alpha_pi prod_l I^p_l(x_il)
//     H^pq_S = c_p c_q sum_ii' alpha_pi alpha_qi' prod_{l in S} Q^pq_l(x_il, x_i'l) prod_{l not in S} I^p_l(x_il) I^q_l(x_i'l)
// for the 2d + 1 subsets S = {j} (slot j), all \ {j} (slot d + j) and all (slot 2d).
//
// k_sobol_itab   I^p_l(x_il) and E^p_l(i) = prod_{m != l} I^p_m(x_im) for the N design rows, [P][N][dpad] each; chunk partials of e_p
// k_sobol_pairs  one workgroup per (64 x 64 tile of (i, i'), GP pair p <= q, window of NJ output dimensions): lane = i', a wave walks
//                16 rows i.  The factors of the window's dimensions stay in registers (q_l and prefix . u_l), the dimensions outside
//                it only enter a running product; a context with d above its window takes ceil(d / NJ) passes, each of which
//                recomputes the factors.  Products over l are prefix x suffix products, never quotients: a Q factor that underflows
//                to zero gives 0, not NaN.  The tile's 2d + 1 partials go to a workspace.
// k_sobol_sum    adds the tile partials of a (p, q, S) in tile order (row block, then column block; for p = q the lower block triangle
//                with the off-diagonal tiles doubled), the chunk partials of e_p in chunk order
// k_sobol_obs    V_S(m) = sum_pq A_pm A_qm (H^pq_S - e_p e_q) and the indices of observable m
// k_sobol_main_effect   E[f_m | x_j = t] on a grid, design rows summed in index order
// No floating-point atomics; a (p, q) block's bits do not depend on the other GPs of the call.  Only the N real rows are visited
// (design point i at stored row pad_front(Np, N) + i): nothing is assumed about alpha in the padding.
#include "gpb_internal.h"
#include <math.h>

namespace gpb {

namespace {

constexpr int SB_CST = 8;       // constants per dimension of a GP pair (k_sobol_pairs)

struct SobolBox {
    double lo[MAX_D], hi[MAX_D];
};


__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(64) void k_sobol_itab(const double* __restrict__ X, const double* __restrict__ ls,
                                                   const double* __restrict__ alpha, SobolBox box, int N, int64_t Np, int pad, int d,
                                                   int dpad, int nB, double* __restrict__ Itab, double* __restrict__ Etab,
                                                   double* __restrict__ epart) {
    const int lane = threadIdx.x, p = blockIdx.y;
    const int i = blockIdx.x * 64 + lane;
    double term = 0.0;
    if (i < N) {
        const double* x = X + (pad + (int64_t)i) * dpad;
        double* It = Itab + ((int64_t)p * N + i) * dpad;
        double* Et = Etab + ((int64_t)p * N + i) * dpad;
        double pre = 1.0;
        for (int l = 0; l < d; ++l) {
            const double len = ls[p * dpad + l], r = 0.7071067811865476 / len;
            const double v = len * 1.2533141373155003 / (box.hi[l] - box.lo[l]) * (erf((box.hi[l] - x[l]) * r) - erf((box.lo[l] - x[l]) * r));
            It[l] = v;
            Et[l] = pre;
            pre *= v;
        }
        double suf = 1.0;
        for (int l = d - 1; l >= 0; --l) {
            Et[l] *= suf;
            suf *= It[l];
        }
        for (int l = d; l < dpad; ++l) It[l] = Et[l] = 1.0;
        term = alpha[(int64_t)p * Np + pad + i] * pre;
    }
    term = wave_sum(term);
    if (lane == 0) epart[p * nB + blockIdx.x] = term;
}

// One Q factor (see the head of the file) from the row-side value a, the lane-side value b and the GP pair's constants of the
// dimension (c7 = 0 for a real dimension; c4 = 0, c7 = 1 for a padding one: exactly 1).  A call, not inlined: the ~60 fp64 coefficients of erf and
// exp are then materialised where they are used; inlined into the row loop they are hoisted out of it and spill.
__device__ __attribute__((noinline)) double sobol_factor(double a, double b, double c0, double c1, double c2, double c3, double c4,
                                                         double c5, double c6, double c7) {
    const double df = a - b, cc = c1 * a + c2 * b;
    return fma(exp(df * df * c0), c4 * (erf((c6 - cc) * c3) - erf((c5 - cc) * c3)), c7);
}

template <int NJ>
__global__ __launch_bounds__(256, NJ <= 20 ? 2 : 1) void k_sobol_pairs(const double* __restrict__ X, const double* __restrict__ Itab,
                                                     const double* __restrict__ Etab, const double* __restrict__ alpha,
                                                     const double* __restrict__ ls, SobolBox box, int N, int64_t Np, int pad, int d,
                                                     int dpad, int P, int nB, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* sb = sm;                     // [dpad][64] x_i'l of the lane side
    double* sI = sb + dpad * 64;         // [dpad][64] I^q_l(x_i'l)
    double* sE = sI + dpad * 64;         // [dpad][64] E^q_l(i')
    double* cst = sE + dpad * 64;        // [dpad][SB_CST]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* rw = cst + dpad * SB_CST + w * 3 * dpad;   // [3][dpad] of this wave: x_il, I^p_l(x_il), E^p_l(i) of its current row i, read as broadcasts
    int p = 0, q = (int)blockIdx.y;
    while (q >= P - p) { q -= P - p; ++p; }
    q += p;
    const int bi = blockIdx.x / nB, bj = blockIdx.x % nB;
    if (p == q && bj > bi) return;       // H^pp is symmetric in (i, i'): k_sobol_sum doubles the tiles below the diagonal
    const int j0 = blockIdx.z * NJ;
    // the padding dimensions d <= l < dpad take part as factors of exactly 1 (tables: 1; constants: q = 0 + 1), so that the window
    // loops below carry no conditions; their outputs are not written
    for (int e = tid; e < dpad * 64; e += 256) {
        const int l = e >> 6, ip = min(bj * 64 + (e & 63), N - 1);
        sb[e] = X[(pad + (int64_t)ip) * dpad + l];
        sI[e] = Itab[((int64_t)q * N + ip) * dpad + l];
        sE[e] = Etab[((int64_t)q * N + ip) * dpad + l];
    }
    if (tid < dpad) {
        const bool real = tid < d;
        const double lp = ls[p * dpad + tid], lq = ls[q * dpad + tid];
        const double ip2 = 1.0 / (lp * lp), iq2 = 1.0 / (lq * lq), s = ip2 + iq2;
        double* c = cst + tid * SB_CST;
        c[0] = -0.5 / (lp * lp + lq * lq);
        c[1] = ip2 / s;
        c[2] = iq2 / s;
        c[3] = sqrt(0.5 * s);
        c[4] = real ? sqrt(1.5707963267948966 / s) / (box.hi[tid] - box.lo[tid]) : 0.0;
        c[5] = real ? box.lo[tid] : 0.0;
        c[6] = real ? box.hi[tid] : 1.0;
        c[7] = real ? 0.0 : 1.0;
    }
    __syncthreads();
    const int il = bj * 64 + lane;
    const double wl = il < N ? alpha[(int64_t)q * Np + pad + il] : 0.0;
    double accF[NJ], accT[NJ], accA = 0.0;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) accF[jj] = accT[jj] = 0.0;
    const int i0 = bi * 64 + w * 16, nrow = max(0, min(16, N - i0));      // the same in every lane of the wave
    const int ll = min(lane, dpad - 1);
    // lane l < d fetches the row side of dimension l one row ahead; the wave's LDS operations execute in order, so the row's
    // values are in place for the broadcast reads that follow and are not overwritten before the last of them
    double nx = 0.0, nI = 0.0, nE = 0.0;
    auto fetch = [&](int i) {
        nx = X[(pad + (int64_t)i) * dpad + ll];
        nI = Itab[((int64_t)p * N + i) * dpad + ll];
        nE = Etab[((int64_t)p * N + i) * dpad + ll];
    };
    if (nrow > 0) fetch(i0);
    for (int r = 0; r < nrow; ++r) {
        if (lane < dpad) {
            rw[lane] = nx;
            rw[dpad + lane] = nI;
            rw[2 * dpad + lane] = nE;
        }
        __builtin_amdgcn_wave_barrier();
        const double ai = alpha[(int64_t)p * Np + pad + i0 + r];
        if (r + 1 < nrow) fetch(i0 + r + 1);
        // an offset of zero the compiler cannot see through: the lane side and the constants do not change from row to row, and
        // hoisted out of the row loop they would take 20 registers per dimension
        int z = 0;
        auto factor = [&](int l) {
            asm volatile("" : "+v"(z) : : "memory");              // (and one dimension's loads at a time)
            const double* c = cst + z + l * SB_CST;
            return sobol_factor(rw[l], sb[z + l * 64 + lane], c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]);
        };
        double qa[NJ], ya[NJ];
        double pre = 1.0;
        for (int l = 0; l < j0; ++l) pre *= factor(l);
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int l = j0 + jj;
            const double qv = factor(l);
            qa[jj] = qv;
            ya[jj] = pre * (rw[dpad + l] * sI[z + l * 64 + lane]);
            accF[jj] = fma(ai, qv * (rw[2 * dpad + l] * sE[z + l * 64 + lane]), accF[jj]);
            pre *= qv;
            // formed here, not after the last call: the scheduler would otherwise keep the four table values of every dimension
            // alive until then
            asm volatile("" : "+v"(ya[jj]), "+v"(accF[jj]), "+v"(pre));
        }
        double suf = 1.0;
        for (int l = j0 + NJ; l < dpad; ++l) suf *= factor(l);
        accA = fma(ai, pre * suf, accA);
#pragma unroll
        for (int jj = NJ - 1; jj >= 0; --jj) {
            accT[jj] = fma(ai, ya[jj] * suf, accT[jj]);
            suf *= qa[jj];
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();                                              // the lane-side tables are done with: sm takes the waves' sums
    double* red = sm;                                             // [4][2 NJ + 1]
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const double f = wave_sum(accF[jj] * wl), t = wave_sum(accT[jj] * wl);
        if (lane == 0) {
            red[w * (2 * NJ + 1) + jj] = f;
            red[w * (2 * NJ + 1) + NJ + jj] = t;
        }
    }
    {
        const double a = wave_sum(accA * wl);
        if (lane == 0) red[w * (2 * NJ + 1) + 2 * NJ] = a;
    }
    __syncthreads();
    if (tid < 2 * NJ + 1) {
        const double v = ((red[tid] + red[(2 * NJ + 1) + tid]) + red[2 * (2 * NJ + 1) + tid]) + red[3 * (2 * NJ + 1) + tid];
        const int ns = 2 * d + 1;
        double* out = part + (((int64_t)blockIdx.y * nB + bi) * nB + bj) * ns;
        if (tid == 2 * NJ) {
            if (j0 == 0) out[2 * d] = v;
        } else {
            const int j = j0 + (tid < NJ ? tid : tid - NJ);
            if (j < d) out[(tid < NJ ? 0 : d) + j] = v;
        }
    }
}

// block = GP pair p <= q, thread = subset slot; the diagonal pairs also sum their GP's e partials
__global__ __launch_bounds__(256) void k_sobol_sum(const double* __restrict__ part, const double* __restrict__ epart,
                                                   const double* __restrict__ amp, int d, int P, int nB, double* __restrict__ e_out,
                                                   double* __restrict__ H_out) {
    int p = 0, q = (int)blockIdx.x;
    while (q >= P - p) { q -= P - p; ++p; }
    q += p;
    const int ns = 2 * d + 1, S = threadIdx.x;
    if (S < ns) {
        const double* pp = part + (int64_t)blockIdx.x * nB * nB * ns + S;
        double sum = 0.0;
        for (int bi = 0; bi < nB; ++bi)
            for (int bj = 0; bj < (p == q ? bi + 1 : nB); ++bj) {
                const double v = pp[((int64_t)bi * nB + bj) * ns];
                sum += (p == q && bj < bi) ? 2.0 * v : v;
            }
        const double h = amp[p] * amp[q] * sum;
        H_out[((int64_t)p * P + q) * ns + S] = h;
        H_out[((int64_t)q * P + p) * ns + S] = h;
    }
    if (p == q && S == 0) {
        double sum = 0.0;
        for (int b = 0; b < nB; ++b) sum += epart[p * nB + b];
        e_out[p] = amp[p] * sum;
    }
}

// the linear map of observable m: f_m = mu_m + sum_p a_p z_p (PCA modes: column m of A; no-PCA modes: scale_m on GP m alone)
struct SobolLin {
    const double *A, *mu, *scale;
    int P, M;
    bool no_pca;
    __device__ __forceinline__ double a(int p, int m) const { return no_pca ? (p == m ? scale[m] : 0.0) : A[(int64_t)p * M + m]; }
    __device__ __forceinline__ int p0(int m) const { return no_pca ? m : 0; }
    __device__ __forceinline__ int p1(int m) const { return no_pca ? m + 1 : P; }
};

__global__ __launch_bounds__(256) void k_sobol_obs(const double* __restrict__ e, const double* __restrict__ H, SobolLin lin, int d,
                                                   double* __restrict__ mean, double* __restrict__ var, double* __restrict__ first,
                                                   double* __restrict__ total) {
    __shared__ double sV[2 * MAX_D + 1];
    const int m = blockIdx.x, S = threadIdx.x, ns = 2 * d + 1, P = lin.P;
    const int p0 = lin.p0(m), p1 = lin.p1(m);
    if (S < ns) {
        double v = 0.0;
        for (int p = p0; p < p1; ++p)
            for (int q = p0; q < p1; ++q) v = fma(lin.a(p, m) * lin.a(q, m), H[((int64_t)p * P + q) * ns + S] - e[p] * e[q], v);
        sV[S] = v;
    }
    __syncthreads();
    const double V = sV[2 * d];
    if (S < d) {
        first[(int64_t)m * d + S] = sV[S] / V;
        total[(int64_t)m * d + S] = 1.0 - sV[d + S] / V;
    }
    if (S == 0) {
        double v = 0.0;
        for (int p = p0; p < p1; ++p) v = fma(lin.a(p, m), e[p], v);
        mean[m] = lin.mu[m] + v;
        var[m] = V;
    }
}

// thread = grid point; zbuf [G][P] holds the per-GP conditional means of the thread's point between its two loops
__global__ __launch_bounds__(64) void k_sobol_main_effect(const double* __restrict__ X, const double* __restrict__ Etab,
                                                          const double* __restrict__ alpha, const double* __restrict__ ls,
                                                          const double* __restrict__ amp, const double* __restrict__ t, int G, int j,
                                                          int N, int64_t Np, int pad, int dpad, SobolLin lin, double* zbuf,
                                                          double* __restrict__ curve) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= G) return;
    const double tg = t[g];
    const int P = lin.P, M = lin.M;
    for (int p = 0; p < P; ++p) {
        const double len = ls[p * dpad + j], c = -0.5 / (len * len);
        double s = 0.0;
        for (int i = 0; i < N; ++i) {
            const double df = tg - X[(pad + (int64_t)i) * dpad + j];
            s = fma(alpha[(int64_t)p * Np + pad + i] * Etab[((int64_t)p * N + i) * dpad + j], exp(df * df * c), s);
        }
        zbuf[(int64_t)g * P + p] = amp[p] * s;
    }
    for (int m = 0; m < M; ++m) {
        double v = 0.0;
        for (int p = lin.p0(m); p < lin.p1(m); ++p) v = fma(lin.a(p, m), zbuf[(int64_t)g * P + p], v);
        curve[(int64_t)g * M + m] = lin.mu[m] + v;
    }
}

// output dimensions per pass of k_sobol_pairs: the context's padded width up to 32; two passes of 24 / 32 above
int sobol_window(int64_t dpad) { return dpad == 48 ? 24 : dpad == 64 ? 32 : (int)dpad; }

SobolBox sobol_box(const gpb_ctx* ctx) {
    SobolBox b;
    for (int l = 0; l < MAX_D; ++l) {
        b.lo[l] = l < ctx->d ? ctx->h_sobol_box[(size_t)l] : 0.0;
        b.hi[l] = l < ctx->d ? ctx->h_sobol_box[(size_t)(ctx->d + l)] : 1.0;
    }
    return b;
}

SobolLin sobol_lin(const gpb_ctx* ctx) {
    return SobolLin{ctx->A, ctx->mu, ctx->scale, (int)ctx->P, (int)ctx->M,
                    ctx->mode == GPB_MODE_NO_PCA || ctx->mode == GPB_MODE_NO_PCA_EXPDIAG};
}

// the front of the context's sobol_ws as it stands
SobolWs sobol_pieces(const gpb_ctx* ctx) {
    SobolWs ws;
    Carver<double> c(ctx->sobol_ws.get());
    sobol_lay(ctx, c, ws, true);
    return ws;
}

int launch_itab(gpb_ctx* ctx) {
    const int64_t N = ctx->N, Np = ctx->Np, P = ctx->P, dpad = ctx->dpad, nB = Np / 64;
    const SobolWs ws = sobol_pieces(ctx);
    double *Itab = ws.Itab, *Etab = ws.Etab, *epart = ws.epart;
    hipLaunchKernelGGL(k_sobol_itab, dim3((unsigned)nB, (unsigned)P), dim3(64), 0, ctx->stream, ctx->X, ctx->ls, ctx->alpha,
                       sobol_box(ctx), (int)N, Np, (int)pad_front(Np, N), (int)ctx->d, (int)dpad, (int)nB, Itab, Etab, epart);
    GPB_HIP(hipGetLastError());
    return 0;
}

template <int NJ>
int launch_pairs_t(gpb_ctx* ctx, double* part) {
    const int64_t N = ctx->N, Np = ctx->Np, P = ctx->P, d = ctx->d, dpad = ctx->dpad, nB = Np / 64;
    const SobolWs ws = sobol_pieces(ctx);
    const double *Itab = ws.Itab, *Etab = ws.Etab;
    const size_t red = sizeof(double) * 4 * (2 * NJ + 1), tab = sizeof(double) * (size_t)(3 * 64 * dpad + SB_CST * dpad + 4 * 3 * dpad);
    const size_t sh = tab > red ? tab : red;
    const dim3 grid((unsigned)(nB * nB), (unsigned)(P * (P + 1) / 2), (unsigned)(dpad / NJ));
    if (sh > 64 * 1024)
        GPB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sobol_pairs<NJ>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    hipLaunchKernelGGL(k_sobol_pairs<NJ>, grid, dim3(256), sh, ctx->stream, ctx->X, Itab, Etab, ctx->alpha, ctx->ls,
                       sobol_box(ctx), (int)N, Np, (int)pad_front(Np, N), (int)d, (int)dpad, (int)P, (int)nB, part);
    GPB_HIP(hipGetLastError());
    return 0;
}

}  // namespace

void sobol_lay(const gpb_ctx* ctx, Carver<double>& c, SobolWs& ws, bool with_part) {
    const int64_t P = ctx->P, nB = ctx->Np / 64;
    ws.lay(c, P, ctx->N, ctx->dpad, nB, with_part ? P * (P + 1) / 2 * nB * nB * (2 * ctx->d + 1) : 0);
}

// Checks the state and the box of a Sobol call (GPB_E_STATE / GPB_E_ARG), keeps the box and selects the device.
int sobol_plan(gpb_ctx* ctx, const char* who, const double* lo, const double* hi, bool need_transform) {
    const std::string w(who);
    if (ctx->N == 0) GPB_FAIL(GPB_E_STATE, w + " before gpb_gp_set");
    if (ctx->multi) GPB_FAIL(GPB_E_STATE, w + ": a gpb_gp_set_multi context is fit-only (its GPs have different designs)");
    if (!ctx->factored) GPB_FAIL(GPB_E_STATE, w + " before gpb_gp_factor");
    if (need_transform && !ctx->have_transform) GPB_FAIL(GPB_E_STATE, w + " before gpb_emu_set_transform");
    if (ctx->kind != GPB_KERNEL_RBF)
        GPB_FAIL(GPB_E_ARG, w + ": the closed form needs a kernel that is a product over the input dimensions (RBF); the Matern kernels are not");
    if (ctx->pmap_d_in > 0) GPB_FAIL(GPB_E_ARG, w + ": the context has a parameter map, which is not linear in the original parameters");
    if (!lo || !hi) GPB_FAIL(GPB_E_ARG, w + ": null box");
    for (int64_t l = 0; l < ctx->d; ++l)
        if (!(hi[l] > lo[l]) || !isfinite(lo[l]) || !isfinite(hi[l])) GPB_FAIL(GPB_E_ARG, w + ": the box needs finite lo < hi in every dimension");
    if (ctx->P * (ctx->P + 1) / 2 > 65535 || ctx->Np / 64 > 255) GPB_FAIL(GPB_E_ARG, w + ": more than 361 GPs or 16320 design points");
    ctx->h_sobol_box.assign(lo, lo + ctx->d);
    ctx->h_sobol_box.insert(ctx->h_sobol_box.end(), hi, hi + ctx->d);
    GPB_HIP(hipSetDevice(ctx->device));
    return 0;
}

// e_dev [P], H_dev [P][P][2d + 1] of the planned box (sobol_ws sized for sobol_lay with its partials)
int launch_sobol(gpb_ctx* ctx, double* e_dev, double* H_dev) {
    int rc = launch_itab(ctx);
    if (rc) return rc;
    const SobolWs ws = sobol_pieces(ctx);
    double* part = ws.part;
    rc = with_int<8, 16, 20, 24, 32>(sobol_window(ctx->dpad), [&](auto NJ) { return launch_pairs_t<decltype(NJ)::value>(ctx, part); });
    if (rc) return dispatched(ctx, rc, "k_sobol_pairs");
    const int64_t P = ctx->P, nB = ctx->Np / 64;
    const double* epart = ws.epart;
    hipLaunchKernelGGL(k_sobol_sum, dim3((unsigned)(P * (P + 1) / 2)), dim3(256), 0, ctx->stream, part, epart, ctx->amp, (int)ctx->d,
                       (int)P, (int)nB, e_dev, H_dev);
    GPB_HIP(hipGetLastError());
    return 0;
}

// mean / var [M], first / total [M][d] from e_dev, H_dev through the installed transform (its linear part in the exp modes)
int launch_sobol_obs(gpb_ctx* ctx, const double* e_dev, const double* H_dev, double* mean, double* var, double* first, double* total) {
    hipLaunchKernelGGL(k_sobol_obs, dim3((unsigned)ctx->M), dim3(256), 0, ctx->stream, e_dev, H_dev, sobol_lin(ctx), (int)ctx->d, mean,
                       var, first, total);
    GPB_HIP(hipGetLastError());
    return 0;
}

// curve_dev [G][M] at the grid t_dev [G] for parameter j of the planned box; zbuf_dev [G][P] is scratch
int launch_sobol_main_effect(gpb_ctx* ctx, int64_t j, const double* t_dev, int64_t G, double* zbuf_dev, double* curve_dev) {
    const int rc = launch_itab(ctx);
    if (rc) return rc;
    const int64_t N = ctx->N, Np = ctx->Np;
    const double* Etab = sobol_pieces(ctx).Etab;
    hipLaunchKernelGGL(k_sobol_main_effect, dim3((unsigned)((G + 63) / 64)), dim3(64), 0, ctx->stream, ctx->X, Etab, ctx->alpha, ctx->ls,
                       ctx->amp, t_dev, (int)G, (int)j, (int)N, Np, (int)pad_front(Np, N), (int)ctx->dpad, sobol_lin(ctx), zbuf_dev,
                       curve_dev);
    GPB_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpb
