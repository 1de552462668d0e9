// gpb_coupled.hip — the likelihood of a chain whose experimental covariance couples its emulators.
//   coupled_setup.h has the algebra: per row, with m, g the means and variances of all PT GPs of the chain in emuList order,
//       S = I + R diag(g) R^T     v = R m + v0     loglike = -1/2 (c_perp + v^T S^-1 v) - 1/2 (logdet0 + log det S)
//   one PT x PT Cholesky instead of the (sum M) x (sum M) one.
//   gpb_chain_like_set     the emulators' own blocks (gpb_like_set) + the joint tables in the chain's first context
//   coupling_check         stale / foreign couplings refuse, they never evaluate the block-diagonal likelihood instead
//   k_coupled<PP, false>   step (3) of chain_rows: one workgroup per row inside the box
//   k_coupled<PP, true>    the gradient's weights d loglike / d (m, g) of every row
#include "gpb_internal.h"
#include "coupled_setup.h"

namespace gpb {
namespace {

// where a row's m and g come from: the finalised mean_pc / var_pc [P][Wld] of the member contexts, GP `off + p` of the chain
// being GP p of its emulator
struct CpMember {
    const double *mean, *var;
    int64_t Wld;
    int off, P;
};
struct CpTable { CpMember c[MAX_CHAIN_CTX]; int E; };
struct CpGrad { double* wmu[MAX_CHAIN_CTX]; double* wv[MAX_CHAIN_CTX]; };

template <int PP> constexpr size_t coupled_lds() { return ((size_t)(PP + 1) * (PP + 1) + 3 * PP + PP / 4) * sizeof(double); }

// One workgroup of 256 threads per row.  LDS: the augmented matrix [S; v^T] ((PP + 1) rows of PP + 1 doubles, lower triangle
// used) | m -> z [PP] | g [PP] | 1 / L_jj [PP] | the pivot products of four columns each [PP / 4].
// PP = the padded order: R^T (RT [PP][PP], row p = column p of R) and v0 are zero beyond PT, so the rows of S beyond PT are
// unit rows, their pivots 1 and their v 0 (identity padding, as k_loglike_lowrank_multi): x * 1 = x, x + 0 = x, log 1 = 0.
// The arithmetic of a row is a function of the row's m and g alone: no other row, no batch size and no position enters.
//   S build      thread (ty, tx) of a 16 x 16 grid owns the TS x TS block (rows ty TS.., columns tx TS..) of the lower block
//                triangle: S_ij = delta_ij + sum_{p >= ty TS} (R_ip g_p) R_jp, p ascending (R_ip = 0 for p < i: exact no-ops)
//   factorise    right-looking, column by column, one barrier per column: column j stays as built (L_ij = S_ij / L_jj is
//                formed where it is used), the trailing elements (i, k), j < k <= i, are 2-D cyclic over the threads; row PP
//                carries v, so the forward solve z = L^-1 v comes along (z_j = v_j / L_jj once column j is reached)
//   conventions  of the block likelihood kernels: a non-positive pivot or an overflowing pivot product gives NaN and counts
//                in notpd; log det S = sum of log(product of four pivots), in column order
// GRAD (all W rows, no compaction): with Y = L^-1 R, t = Y^T z and the column norms |Y_p|^2 = (R^T S^-1 R)_pp give
//       d loglike / d m_p = -t_p        d loglike / d g_p = 1/2 t_p^2 - 1/2 |Y_p|^2
// L is scaled in place, L^-1 is formed row by row into the unused upper triangle (thread j: column j of L^-1 by forward
// substitution, kept as row j of the upper triangle — no thread reads another's row), R then takes L's place in the lower
// triangle and thread p walks Y_p = L^-1 R_p element by element.  Rows whose S fails give NaN weights.
template <int PP, bool GRAD>
__global__ __launch_bounds__(256) void k_coupled(const CpTable tab, int PT, const double* __restrict__ RT,
                                                 const double* __restrict__ v0g, double cperp, double logdet0,
                                                 double* __restrict__ ll, const int* __restrict__ cmp, double inside_const,
                                                 int* __restrict__ notpd, const CpGrad gr) {
    constexpr int LD = PP + 1, TS = PP / 16, UNR = TS == 4 ? 4 : 2;     // UNR: steps of the S build with their loads in flight
    extern __shared__ double sh[];
    double* S = sh;
    double* sm = S + (PP + 1) * LD;
    double* sg = sm + PP;
    double* srinv = sg + PP;
    double* sgp = srinv + PP;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t w = blockIdx.x;
    if (!GRAD && w >= cmp[0]) return;                  // (uniform: rows past the count do not exist)
    int my_e = 0;
    if (tid < PP) {                                    // gather m and g
        double m = 0.0, g = 0.0;
        if (tid < PT) {
            while (my_e + 1 < tab.E && tab.c[my_e + 1].off <= tid) ++my_e;
            const CpMember& c = tab.c[my_e];
            m = c.mean[(int64_t)(tid - c.off) * c.Wld + w];
            g = c.var[(int64_t)(tid - c.off) * c.Wld + w];
        }
        sm[tid] = m;
        sg[tid] = g;
    }
    __syncthreads();
    // v = R m + v0, into row PP: by the LAST PP threads, whose blocks of S below have the shortest sums (the first waves own
    // the blocks that start at p = 0).  Both loops are unrolled so that several loads of R (L2) are in flight at once; the
    // additions keep their order.
    if (tid >= 256 - PP) {
        const int i = tid - (256 - PP);
        double vi = v0g[i];
#pragma unroll 8
        for (int p = i; p < PT; ++p) vi = fma(RT[p * PP + i], sm[p], vi);
        S[PP * LD + i] = vi;
    }
    if (ty >= tx) {
        double acc[TS][TS];
#pragma unroll
        for (int a = 0; a < TS; ++a)
#pragma unroll
            for (int b = 0; b < TS; ++b) acc[a][b] = (ty == tx && a == b) ? 1.0 : 0.0;
#pragma unroll UNR
        for (int p = ty * TS; p < PT; ++p) {
            const double gp = sg[p];
            double ri[TS], rj[TS];
#pragma unroll
            for (int a = 0; a < TS; ++a) { ri[a] = RT[p * PP + ty * TS + a] * gp; rj[a] = RT[p * PP + tx * TS + a]; }
#pragma unroll
            for (int a = 0; a < TS; ++a)
#pragma unroll
                for (int b = 0; b < TS; ++b) acc[a][b] = fma(ri[a], rj[b], acc[a][b]);
        }
#pragma unroll
        for (int a = 0; a < TS; ++a)
#pragma unroll
            for (int b = 0; b < TS; ++b) S[(ty * TS + a) * LD + tx * TS + b] = acc[a][b];
    }
    __syncthreads();
    double q = 0.0, prod = 1.0;
    bool bad = false;
    for (int j = 0; j < PP; ++j) {
        const double ajj = S[j * LD + j];
        bad = bad || !(ajj > 0.0);
        const double rinv = rsqrt(ajj);                // 1 / L_jj
        const double zj = S[PP * LD + j] * rinv;       // forward solve: z_j
        q = fma(zj, zj, q);
        prod *= ajj;
        if ((j & 3) == 3) {
            if (tid == 0) sgp[j >> 2] = prod;
            prod = 1.0;
        }
        if (GRAD && tid == 0) { srinv[j] = rinv; sm[j] = zj; }
        double lk[TS];
#pragma unroll
        for (int b = 0; b < TS; ++b) lk[b] = S[(tx + 16 * b) * LD + j] * rinv;         // L_kj of this thread's columns
#pragma unroll
        for (int a = 0; a <= TS; ++a) {
            const int i = ty + 16 * a;                 // rows j < i <= PP (row PP: v)
            if (i > j && i <= PP) {
                const double li = S[i * LD + j] * rinv;
#pragma unroll
                for (int b = 0; b < TS; ++b) {
                    const int k = tx + 16 * b;
                    if (k > j && k <= i && k < PP) S[i * LD + k] = fma(-li, lk[b], S[i * LD + k]);
                }
            }
        }
        __syncthreads();                               // column j + 1 is complete; column j is not read again
    }
    if (tid < PP / 4) sgp[tid] = log(sgp[tid]);        // in parallel, off the factorisation's dependency chain
    __syncthreads();
    double logsum = 0.0;
    for (int g = 0; g < PP / 4; ++g) logsum += sgp[g];                 // fixed order
    bad = bad || !(logsum < INFINITY);                 // an overflowing pivot product is a failure, not a silent -inf
    if (!GRAD) {
        if (tid == 0) {
            double r = -0.5 * (cperp + q) - 0.5 * (logdet0 + logsum);
            if (bad) {
                r = nan("");
                atomicAdd(notpd, 1);
            }
            ll[cmp[4 + w]] = r + inside_const;
        }
        return;
    }
    // ---- the gradient's weights
    for (int e = tid; e < PT * PT; e += 256) {         // L_ik = S_ik / L_kk below the diagonal (the diagonal lives in srinv)
        const int i = e / PT, k = e % PT;
        if (k < i) S[i * LD + k] *= srinv[k];
    }
    __syncthreads();
    if (tid < PT) {                                    // column j of L^-1 -> row j of the upper triangle
        const int j = tid;
        const double xj = srinv[j];
        for (int i = j + 1; i < PT; ++i) {
            double s = S[i * LD + j] * xj;
            for (int k = j + 1; k < i; ++k) s = fma(S[i * LD + k], S[j * LD + k], s);
            S[j * LD + i] = -s * srinv[i];
        }
    }
    __syncthreads();
    for (int e = tid; e < PT * PT; e += 256) {         // R_kp, k <= p, at [p][k]: L is no longer needed
        const int p = e / PT, k = e % PT;
        if (k <= p) S[p * LD + k] = RT[p * PP + k];
    }
    __syncthreads();
    if (tid < PT) {
        const int p = tid;
        double t = 0.0, dg = 0.0;
        for (int i = 0; i < PT; ++i) {                 // Y_ip = sum_{k <= min(i, p)} (L^-1)_ik R_kp
            const int kmax = i < p ? i : p;
            double y = 0.0;
            for (int k = 0; k <= kmax; ++k) {
                const double linv = (k == i) ? srinv[i] : S[k * LD + i];
                y = fma(linv, S[p * LD + k], y);
            }
            t = fma(y, sm[i], t);
            dg = fma(y, y, dg);
        }
        const CpMember& c = tab.c[my_e];
        const int64_t o = w * c.P + (p - c.off);
        const double nanv = nan("");
        gr.wmu[my_e][o] = bad ? nanv : -t;
        gr.wv[my_e][o] = bad ? nanv : 0.5 * (t * t - dg);
    }
}

int fill_table(gpb_ctx* const* ctxs, int E, CpTable& tab) {
    int off = 0;
    for (int e = 0; e < E; ++e) {
        const gpb_ctx* c = ctxs[e];
        tab.c[e] = CpMember{c->mean_pc, c->var_pc, c->Wld, off, (int)c->P};
        off += (int)c->P;
    }
    tab.E = E;
    return off;
}

template <bool GRAD>
int launch_coupled(gpb_ctx* const* ctxs, int E, int64_t W, double* ll_dev, const int* cmpv, double inside_const, const CpGrad& gr) {
    gpb_ctx* ctx = ctxs[0];
    const gpb_ctx::Coupling& cp = ctx->cpl;
    CpTable tab;
    if (fill_table(ctxs, E, tab) != cp.PT) GPB_FAIL(GPB_E_STATE, "gpb: internal: coupled likelihood over another number of GPs");
    const int rc = with_int<64, 128>(cp.PP, [&](auto N) {
        constexpr int PP = decltype(N)::value;
        constexpr size_t sh = coupled_lds<PP>();
        if (sh > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_coupled<PP, GRAD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sh) != hipSuccess)
            return (int)GPB_E_HIP;
        hipLaunchKernelGGL((k_coupled<PP, GRAD>), dim3((unsigned)W), dim3(256), sh, ctx->stream, tab, cp.PT, cp.RT, cp.v0, cp.cperp,
                           cp.logdet0, ll_dev, cmpv, inside_const, ctx->notpd, gr);
        return 0;
    });
    if (rc == GPB_E_HIP) GPB_FAIL(GPB_E_HIP, "gpb: k_coupled: the kernel's LDS could not be reserved");
    if (rc) return dispatched(ctx, rc, "k_coupled");
    if (hipGetLastError() != hipSuccess) GPB_FAIL(GPB_E_HIP, "gpb: k_coupled launch failed");
    return 0;
}

}  // namespace

int coupling_check(gpb_ctx* const* ctxs, int E, const char* who) {
    gpb_ctx* ctx = ctxs[0];
    const gpb_ctx::Coupling& cp = ctx->cpl;
    if (!cp.on) return 0;
    bool same = (int)cp.members.size() == E;
    for (int e = 0; e < E && same; ++e) same = cp.members[e] == ctxs[e];
    if (!same)
        GPB_FAIL(GPB_E_STATE, std::string(who) + ": the first context holds a coupled likelihood of another list of contexts "
                                                 "(gpb_chain_like_set installs or clears it)");
    for (int e = 0; e < E; ++e)
        if (ctxs[e]->like_epoch != cp.epochs[e])
            GPB_FAIL(GPB_E_STATE, std::string(who) + ": the coupled likelihood is stale: an emulator's transform or likelihood "
                                                     "block was replaced after gpb_chain_like_set");
    return 0;
}

int launch_loglike_coupled(gpb_ctx* const* ctxs, int E, int64_t W, double* ll_dev, const int* cmpv, double inside_const) {
    return launch_coupled<false>(ctxs, E, W, ll_dev, cmpv, inside_const, CpGrad{});
}

int launch_like_w_coupled(gpb_ctx* const* ctxs, int E, int64_t W, double* const* wmu, double* const* wv) {
    CpGrad gr{};
    for (int e = 0; e < E; ++e) { gr.wmu[e] = wmu[e]; gr.wv[e] = wv[e]; }
    return launch_coupled<true>(ctxs, E, W, nullptr, nullptr, 0.0, gr);
}

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_chain_like_set(gpb_ctx* const* ctxs, int E, const double* yexp_host, const double* cov_exp_host,
                                  int* applies_host) {
    if (!chain_args_ok(ctxs, E)) return GPB_E_ARG;
    gpb_ctx* ctx = ctxs[0];
    if (!yexp_host || !applies_host) GPB_FAIL(GPB_E_ARG, "gpb_chain_like_set: null pointer");
    *applies_host = 0;
    int64_t MT = 0, PT = 0;
    bool pca = true;
    for (int e = 0; e < E; ++e) {
        const gpb_ctx* c = ctxs[e];
        if (!c) GPB_FAIL(GPB_E_ARG, "gpb_chain_like_set: null context");
        if (c->device != ctx->device || c->stream != ctx->stream)
            GPB_FAIL(GPB_E_ARG, "gpb_chain_like_set: the emulators' contexts must share one device and stream");
        if (!c->have_transform) GPB_FAIL(GPB_E_STATE, "gpb_chain_like_set before gpb_emu_set_transform");
        MT += c->M;
        PT += c->P;
        pca = pca && c->mode == GPB_MODE_PCA;
    }
    ctx->cpl.on = false;
    for (int e = 0; e < E; ++e) ctxs[e]->lrs_K = 0;    // a new experiment: the per-data-set tables (gpb_chain_like_sets) go
    if (!cov_exp_host) return 0;                      // the coupling is cleared, the blocks stay
    // every emulator's own diagonal block, as before: what reads yexp / Cexp per emulator keeps working
    std::vector<char> in_block((size_t)MT * (size_t)MT, 0);
    std::vector<double> blockv;
    for (int64_t e = 0, o = 0; e < E; o += ctxs[e]->M, ++e) {
        const int64_t M = ctxs[e]->M;
        blockv.resize((size_t)(M * M));
        for (int64_t i = 0; i < M; ++i)
            for (int64_t j = 0; j < M; ++j) {
                blockv[i * M + j] = cov_exp_host[(o + i) * MT + o + j];
                in_block[(o + i) * MT + o + j] = 1;
            }
        if (const int rc = gpb_like_set(ctxs[e], yexp_host + o, blockv.data())) {
            if (e) ctx->err = ctxs[e]->err;
            return rc;
        }
    }
    bool coupled = false;
    for (int64_t i = 0; i < MT * MT && !coupled; ++i) coupled = !in_block[i] && cov_exp_host[i] != 0.0;
    if (!coupled) return 0;                            // block-diagonal: the chain's block path, nothing installed
    if (!pca || PT > COUPLED_MAX_PT || MT > COUPLED_MAX_MT || gpb_chain_supported(ctxs, E) != 1) return 0;
    std::vector<CoupledBlock> blk;
    for (int e = 0; e < E; ++e)
        blk.push_back(CoupledBlock{ctxs[e]->M, ctxs[e]->P, ctxs[e]->h_A.data(), ctxs[e]->h_mu.data(), ctxs[e]->h_C0.data()});
    CoupledTables t;
    if (!coupled_setup(blk.data(), E, yexp_host, cov_exp_host, t)) return 0;
    const int64_t PP = PT <= 64 ? 64 : 128;
    std::vector<double> RT((size_t)(PP * PP), 0.0), v0((size_t)PP, 0.0);
    for (int64_t i = 0; i < PT; ++i) {
        v0[i] = t.v0[i];
        for (int64_t p = i; p < PT; ++p) RT[p * PP + i] = t.R[i * PT + p];
    }
    GPB_HIP(hipSetDevice(ctx->device));
    GPB_HIP(hipStreamSynchronize(ctx->stream));
    CoupledWs ws;
    if (const int rc = ctx_carve(ctx, ctx->cpl_tab, [&](Carver<double>& c) { ws.lay(c, PP); })) return rc;
    GPB_HIP(hipMemcpy(ws.RT, RT.data(), sizeof(double) * RT.size(), hipMemcpyHostToDevice));
    GPB_HIP(hipMemcpy(ws.v0, v0.data(), sizeof(double) * v0.size(), hipMemcpyHostToDevice));
    gpb_ctx::Coupling& cp = ctx->cpl;
    cp.PT = (int)PT;
    cp.PP = (int)PP;
    cp.cperp = t.cperp;
    cp.logdet0 = t.logdet0;
    cp.RT = ws.RT;
    cp.v0 = ws.v0;
    cp.members.assign(ctxs, ctxs + E);
    cp.epochs.resize((size_t)E);
    for (int e = 0; e < E; ++e) cp.epochs[e] = ctxs[e]->like_epoch;
    cp.on = true;
    *applies_host = 1;
    return 0;
}
