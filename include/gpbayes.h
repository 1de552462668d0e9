/*
 * gpbayes.h — C ABI of the MI355X-native GP-emulator + log-posterior engine.
 *
 * The reference (Hendrik1704/GPBayesTools-HIC) is pure Python and has no FFI of its
 * own; the hot path sits behind three duck-typed Python seams.  This
 * header is the C boundary a maintainer binds with ctypes; each
 * entry point names the reference interface it replaces.
 *
 * Conventions
 *   - plain C, no C++/torch types; all matrices row-major float64; sizes int64_t.
 *   - pointers flagged "host" are caller-owned host memory; pointers flagged "dev"
 *     are caller-owned device (HBM) memory on the context's device.  Functions with
 *     an `on_device` argument accept either.
 *   - every function returns int: 0 = ok, >0 = LAPACK-style info (1-based index of the
 *     first non-positive pivot), <0 = GPB_E_* error; gpb_last_error() gives the text.
 *   - work is enqueued on the context's HIP stream; functions that return host data
 *     synchronise that stream themselves, device-output functions do not
 *     (call gpb_sync or use stream order).
 *   - one context per (process, device, emulator); not thread-safe per context.
 *   - there is NO CPU fallback: if no gfx950 device is present gpb_ctx_create fails.
 *   - device buffers a context releases are kept for the next context of about that size (up to GPB_POOL_MB megabytes per
 *     process, default 8192, 0 = off): on this runtime hipFree + hipMalloc of a large buffer is a driver round trip of 60-100 ms.
 */
#ifndef GPBAYES_H
#define GPBAYES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPB_VERSION 110

/* The library is built with -fvisibility=hidden: these entry points are all it exports. */
#define GPB_API __attribute__((visibility("default")))

/* kernel_id  — sklearn kernels the reference instantiates (src/emulator.py:286-306) */
#define GPB_KERNEL_RBF      0   /* 1.*RBF(l) + White          sk:kernels.py:1525-1575 */
#define GPB_KERNEL_MATERN15 1   /* 1.*Matern(l, nu=1.5)+White sk:kernels.py:1721-1723 */
#define GPB_KERNEL_MATERN25 2   /* nu=2.5 (BASELINE cfg 5)    sk:kernels.py:1724-1726 */

/* observable-transform modes of Emulator.predict (src/emulator.py:558-601) */
#define GPB_MODE_PCA            0
#define GPB_MODE_NO_PCA         1  /* perform_no_PCA=True            :562-565,589-592 */
#define GPB_MODE_EXPDIAG        2  /* exp_and_cov_diagonal=True      :567-568,594-601 */
#define GPB_MODE_NO_PCA_EXPDIAG 3

/* errors */
#define GPB_E_ARG     (-1)
#define GPB_E_STATE   (-2)
#define GPB_E_HIP     (-3)
#define GPB_E_NODEV   (-4)
#define GPB_E_ALLOC   (-5)
#define GPB_E_RCCL    (-6)

/* gpb_gp_get selectors */
#define GPB_GET_K      0  /* [P,N,N] K(X,X)+(noise+alpha)I: blocks of the LOWER 64-block triangle as built (call before gpb_gp_factor, which overwrites them) */
#define GPB_GET_L      1  /* [P,N,N] lower Cholesky factor, upper zeroed  == GPR.L_     */
#define GPB_GET_LINV   2  /* [P,N,N] L^-1 (lower)                                       */
#define GPB_GET_ALPHA  3  /* [P,N]   K^-1 z                               == GPR.alpha_ */
#define GPB_GET_KSTAR  4  /* [P,W,N] K(X*,X) of the most recent predict / likelihood batch of W rows == kernel_(X*, X_train_)  sk:_gpr.py:443 */
#define GPB_GET_FORM   5  /* [P]     distance form each GP's kernel matrices are built in, chosen from theta alone: 0 = Gram form
                           *         |a|^2+|b|^2-2a.b on the centred design, 1 = sklearn's difference form (length scales far below the
                           *         design's extent: sum_k (extent_k/l_k)^2 > 1024, e.g. the Matern lower search bound, src/emulator.py:292-297) */

typedef struct gpb_ctx gpb_ctx;

/* ---- lifetime -------------------------------------------------------------------- */
GPB_API int  gpb_version(void);
GPB_API int  gpb_device_count(void);
/* stream: a hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream), or
 * NULL to create a private one. */
GPB_API int  gpb_ctx_create(int device, void* stream, gpb_ctx** out);
GPB_API int  gpb_ctx_destroy(gpb_ctx* ctx);
/* Re-target the context onto a caller stream; NULL selects the legacy default stream (what
 * torch.cuda.current_stream() is unless the caller changed it). */
GPB_API int  gpb_ctx_set_stream(gpb_ctx* ctx, void* stream);
GPB_API int  gpb_sync(gpb_ctx* ctx);
/* Hand every cached device buffer back to the driver (the cache of the header comment: GPB_POOL_MB megabytes per process, default
 * 8192, 0 = off).  The cache is invisible to other allocators of the process (torch's caching allocator, the caller's own
 * hipMalloc): call this before a large allocation elsewhere.  The library does it itself when one of its own allocations fails.
 * No reference counterpart (memory management of the native side). */
GPB_API int  gpb_pool_trim(void);
GPB_API const char* gpb_last_error(gpb_ctx* ctx);
GPB_API void* gpb_stream(gpb_ctx* ctx);

/* ---- GP state: replaces sklearn GaussianProcessRegressor state ------------------- *
 * gpb_gp_set        <- GPR(kernel, alpha).fit(X, z) inputs          src/emulator.py:309-315
 * gpb_gp_set_theta  <- kernel_.theta                                sk:_gpr.py:332
 * gpb_gp_factor     <- K=kernel_(X); K_ii+=alpha; L_=cholesky(K); alpha_=cho_solve   sk:_gpr.py:346-364
 * gpb_gp_lml        <- GPR.log_marginal_likelihood(theta, eval_gradient)             sk:_gpr.py:537-652
 * gpb_gp_predict    <- GPR.predict(X, return_cov=True) + .diagonal()   sk:_gpr.py:441-469, src/emulator.py:553,573-575
 */
GPB_API int gpb_gp_set(gpb_ctx* ctx, int64_t N, int64_t d, int64_t P,
               const double* X_host /*[N,d]*/, const double* Z_host /*[P,N]*/,
               int kernel_id, double alpha);
/* gpb_gp_set_multi: P GPs, each over ITS OWN design — the GPs of several emulators of a chain (the reference fits dataset
 * after dataset and GP after GP: examples/EmulatorTraining.ipynb:124-138, src/emulator.py:309-315) or the 1 + n_restarts
 * starts of every GP's hyper-parameter search (sk:_gpr.py:318-337) side by side in one batch.  All designs must pad to the
 * same multiple of 64 points.  Such a context is fit-only: gpb_gp_set_theta, gpb_gp_factor, gpb_gp_get, gpb_gp_lml and
 * gpb_gp_lml_subset work on it, the predict / likelihood entry points return GPB_E_STATE.
 * gpb_gp_lml_subset: log-marginal likelihood (+ gradient) of n of the stored GPs — the searches still running — at
 * theta[n, d+2]; a GP's values do not depend on which other GPs share the call (bit for bit).  Works on any context; leaves
 * it without a factorisation (gpb_gp_set_theta + gpb_gp_factor afterwards). */
GPB_API int gpb_gp_set_multi(gpb_ctx* ctx, int64_t P, int64_t d, const int64_t* N_host /*[P]*/,
                     const double* const* X_host /*[P] pointers to [N_p,d]*/,
                     const double* const* Z_host /*[P] pointers to [N_p]*/, int kernel_id, double alpha);
/* gpb_gp_set_point_noise <- GPR(kernel, alpha=<array of length N>): a known variance per training point on the diagonal of K
 * (sk:_gpr.py:347, `K[np.diag_indices_from(K)] += self.alpha` with an array) — stochastic kriging, the GP core of the reference's
 * EmulatorBAND(method='PCSK'), which hands the training events' statistical errors to surmise as `simsd`; NOT a port of surmise's PCSK.
 * s_host: P pointers to the N_p variances s[p][i] >= 0 of stored GP p, or NULL for none (what gpb_gp_set / gpb_gp_set_multi leave,
 * both of which reset the context to none).  The training diagonal of GP p becomes c + sigma_n^2 + (alpha + s[p][i]); the sum
 * alpha + s is formed first, so that s = 0 gives the bits of no call, a uniform s = s0 those of the scalar alpha' = fl(alpha + s0),
 * and sklearn's / the oracle's vector alpha_i = alpha + s_i the same diagonal.  The White level stays a hyper-parameter: the
 * homoscedastic remainder.  Valid on gpb_gp_set and gpb_gp_set_multi contexts; call it after either and before the next
 * gpb_gp_factor / gpb_gp_lml / gpb_gp_lml_subset (whose subsets and whose restart copies read their own GP's row).  Leaves the
 * context without a factorisation, as gpb_gp_lml_subset does.  Read by the K assembly, gpb_gp_cv / gpb_emu_cv (cov = G_F^-1 -
 * diag(alpha + s_F)) and nothing else: as in sklearn the per-point term is on the TRAINING diagonal only — the predictive prior
 * c + sigma_n^2, gpb_gp_predict / _cov / _grad, the Sobol indices and the likelihood kernels read L^-1 and alpha_ and are untouched.
 * Errors: GPB_E_STATE before gpb_gp_set; GPB_E_ARG for a null row or a negative or non-finite entry (nothing is changed then: the
 * context stays as it was). */
GPB_API int gpb_gp_set_point_noise(gpb_ctx* ctx, const double* const* s_host /*[P] pointers to [N_p], or NULL: none*/);
GPB_API int gpb_gp_lml_subset(gpb_ctx* ctx, int64_t n, const int32_t* gp_index /*[n]*/, const double* theta_host /*[n,d+2]*/,
                      double* lml_host /*[n]*/, double* grad_host /*[n,d+2] or NULL*/, int* info_host /*[n] or NULL*/);
GPB_API int gpb_gp_set_theta(gpb_ctx* ctx, const double* theta_host /*[P,d+2]*/);
GPB_API int gpb_gp_factor(gpb_ctx* ctx, int* info_host /*[P], may be NULL*/);
GPB_API int gpb_gp_get(gpb_ctx* ctx, int what, double* out_host);
/* Evaluates at theta_host (state of the context's factorisation is overwritten; call
 * gpb_gp_set_theta+gpb_gp_factor afterwards to restore).  grad_host may be NULL.
 * Non-PD K for GP p: lml[p] = -inf, grad[p,:] = 0, info[p] > 0 (sk:_gpr.py:588-589). */
GPB_API int gpb_gp_lml(gpb_ctx* ctx, const double* theta_host /*[P,d+2]*/,
               double* lml_host /*[P]*/, double* grad_host /*[P,d+2] or NULL*/,
               int* info_host /*[P] or NULL*/);
/* mean/var are [W,P] (reference layout of the concatenated per-GP outputs). */
GPB_API int gpb_gp_predict(gpb_ctx* ctx, const double* Xs, int64_t W, int on_device,
                   double* mean /*[W,P]*/, double* var /*[W,P] or NULL*/);

/* Full predictive covariance between the W query points, per GP (what GPR.predict(return_cov=True) returns
 * and GPR.sample_y draws from: sk:_gpr.py:441-469, 498-540; src/emulator.py:608-633).  cov is [P,W,W].
 * Small batches only (W <= 8192): the MCMC path never forms it. */
GPB_API int gpb_gp_predict_cov(gpb_ctx* ctx, const double* Xs, int64_t W, int on_device,
                       double* mean /*[W,P]*/, double* cov /*[P,W,W]*/);

/* Gradient of the per-GP predictions with respect to the query point (the reference has none; closed form of
 * GPR.predict's mean k*^T alpha_ and variance k** - k*^T K^-1 k*, sk:_gpr.py:443,454-460, differentiated in x*):
 *   dmean[w,p,j] = sum_i alpha_i dk(x_w, x_i)/dx_j,  dvar[w,p,j] = -2 sum_i beta_i dk(x_w, x_i)/dx_j,  beta = K^-1 k*(x_w).
 * dvar may be NULL (the mean alone skips beta, one GEMM of the size of the predict call).  fp64 whatever gpb_ctx_option 51
 * selects; a row's bits do not depend on the batch it is evaluated in.  Needs a factorisation (gpb_gp_factor). */
GPB_API int gpb_gp_predict_grad(gpb_ctx* ctx, const double* Xs, int64_t W, int on_device,
                        double* dmean /*[W,P,d]*/, double* dvar /*[W,P,d] or NULL*/);

/* ---- emulator transform: replaces Emulator.predict after the per-GP calls -------- *
 * gpb_emu_set_transform <- _trans_matrix[:npc], scaler.mean_, _cov_trunc, scaler.scale_  src/emulator.py:335-363
 * gpb_emu_predict       <- Emulator.predict(X, return_cov, extra_std)                   src/emulator.py:465-605
 */
GPB_API int gpb_emu_set_transform(gpb_ctx* ctx, int mode, int64_t M,
                          const double* A_host /*[P,M] or NULL (no-PCA)*/,
                          const double* mu_host /*[M]*/,
                          const double* cov_trunc_host /*[M,M] or NULL*/,
                          const double* scale_host /*[M] or NULL (PCA)*/);
GPB_API int gpb_emu_predict(gpb_ctx* ctx, const double* Xs, int64_t W, int on_device,
                    const double* extra_std /*[W] or NULL (=0), same memory space as Xs*/,
                    double* mean /*[W,M]*/, double* cov /*[W,M,M] or NULL*/);

/* gpb_emu_predict_jac: Jacobian of the emulator's mean in observable space (Emulator.predict(X, return_cov=False),
 * src/emulator.py:465-605) with respect to the input, through the transform, the exp of the EXPDIAG modes and, when one is
 * set, the parameter map: Xs is then [W, d_in] in the original parameters (gpb_param_map_set) and jac [W, M, d_in].
 * The response matrix the reference's SensitivityAnalysis notebook builds from 2 d finite-difference predictions. */
GPB_API int gpb_emu_predict_jac(gpb_ctx* ctx, const double* Xs, int64_t W, int on_device, double* jac /*[W,M,d_in]*/);

/* ---- closed-form cross-validation: hold-out predictions of the fitted GPs without refitting ------------------------ *
 * gpb_gp_cv  <- for every fold F: GPR(kernel_ at the SAME theta, alpha).fit(X without F, z without F)  sk:_gpr.py:346-364
 *               followed by .predict(X_F, return_cov=True)                                          sk:_gpr.py:441-469
 * gpb_emu_cv <- those per-GP hold-out means / variances through Emulator.predict's observable transform with
 *               extra_std = 0                                                               src/emulator.py:555-605
 * (the reference's only accuracy check, Emulator.testEmulatorErrors, src/emulator.py:636-679, retrains on the first nev - k events
 * for k validation points; here theta, scaler and PCA are those of the full fit: the textbook GP leave-one-out / leave-k-out.)
 * With Ky = K + (sigma_n^2 + alpha) I = L L^T (gpb_gp_factor) and a fold F of k points (Rasmussen & Williams 5.4.2, for blocks):
 *   G_F  = (Ky^-1)_FF = (L^-1[:, F])^T (L^-1[:, F])      a k x k Gram matrix over the rows of the resident L^-1
 *   mean = z_F - G_F^-1 alpha_F                           the refit's predictive mean at X_F (alpha_ = Ky^-1 z, GPB_GET_ALPHA)
 *   cov  = G_F^-1 - alpha I                               the refit's predictive covariance at X_F (sklearn's prior carries the
 *                                                         White noise but not GPR's alpha); var = its diagonal, not clipped
 * idx_host [n_idx]: distinct design-point indices in [0, N), grouped into folds; fold_ptr_host [nf + 1]: offsets into idx, from 0
 * to n_idx, every fold 1 .. 64 points (fold_ptr_host == NULL: one point per fold, nf = n_idx).  idx_host == NULL: leave-one-out
 * of all N points in order (n_idx = nf = N, fold_ptr_host = NULL).  Both are host arrays; on_device says where the OUTPUTS live
 * (0: host, the call synchronises; 1: device memory, asynchronous).  mean / var [n_idx, P] in the order of idx (var may be
 * NULL); cov [P, nf, kmax, kmax] or NULL: the folds' covariance blocks, zero-padded to the largest fold size kmax.  A call whose
 * folds all hold one point takes one streaming pass over L^-1 (a column's sum of squares); other calls one workgroup per
 * (fold, GP).  A fold's bits do not depend on the folds or GPs that share the call.  A fold whose G_F has a non-positive pivot
 * gets NaN for that GP and counts in the context's not-positive-definite counter; the call does not fail.
 * Errors: GPB_E_STATE without a factorisation, on a gpb_gp_set_multi context and (gpb_emu_cv) without a transform; GPB_E_ARG for
 * an empty fold, a fold of more than 64 points, an index outside [0, N), a repeated index, a fold_ptr that does not increase
 * from 0 to n_idx.  The factorisation, alpha and the results of later predict / likelihood calls are untouched.  gpb_emu_cv
 * (mean [n_idx, M], cov [n_idx, M, M] or NULL, all four GPB_MODE_*) overwrites the workspace of the last predict batch:
 * gpb_gp_get(GPB_GET_KSTAR) is undefined after it (GPB_E_STATE) until the next predict / likelihood call. */
GPB_API int gpb_gp_cv(gpb_ctx* ctx, const int32_t* idx_host /*[n_idx] or NULL*/, int64_t n_idx,
              const int32_t* fold_ptr_host /*[nf+1] or NULL*/, int64_t nf, int on_device,
              double* mean /*[n_idx,P]*/, double* var /*[n_idx,P] or NULL*/, double* cov /*[P,nf,kmax,kmax] or NULL*/);
GPB_API int gpb_emu_cv(gpb_ctx* ctx, const int32_t* idx_host /*[n_idx] or NULL*/, int64_t n_idx,
               const int32_t* fold_ptr_host /*[nf+1] or NULL*/, int64_t nf, int on_device,
               double* mean /*[n_idx,M]*/, double* cov /*[n_idx,M,M] or NULL*/);

/* ---- closed-form Sobol sensitivity indices of the posterior mean over a uniform prior box --------------------------- *
 * The global counterpart of gpb_emu_predict_jac (the reference's SensitivityAnalysis notebook is local: 2 d finite differences
 * at one point).  The RBF kernel is a product over the input dimensions and the prior a box [lo, hi] (widths w = hi - lo), so every
 * integral of the posterior mean over a subset of the inputs is a finite sum of products of error functions (Oakley & O'Hagan
 * 2004); nothing is sampled.  GP p has the mean m_p(x) = c_p sum_i alpha_pi prod_l exp(-(x_l - x_il)^2 / 2 l_pl^2); with a = x_il,
 * b = x_i'l, l = l_pl, l' = l_ql, s = 1/l^2 + 1/l'^2, c = (a/l^2 + b/l'^2) / s:
 *   I^p_l(a)     = l sqrt(pi/2) / w_l [erf((hi_l - a) / (sqrt2 l)) - erf((lo_l - a) / (sqrt2 l))]
 *   Q^pq_l(a, b) = exp(-(a - b)^2 / 2(l^2 + l'^2)) sqrt(pi / 2s) / w_l [erf((hi_l - c) sqrt(s/2)) - erf((lo_l - c) sqrt(s/2))]
 *   e_p    = c_p sum_i alpha_pi prod_l I^p_l(x_il)                                                  = E[m_p]
 *   H^pq_S = c_p c_q sum_ii' alpha_pi alpha_qi' prod_{l in S} Q^pq_l(x_il, x_i'l) prod_{l not in S} I^p_l(x_il) I^q_l(x_i'l)
 *                                                                                                   = E[E[m_p | x_S] E[m_q | x_S]]
 * gpb_gp_sobol: e [P] and H [P, P, 2d + 1] for the subsets {j} (slot j), all \ {j} (slot d + j) and all (slot 2d); H[p][q] ==
 *   H[q][p] bit for bit, both filled.  A (p, q) block's bits do not depend on the other GPs of the context (no atomics, every sum
 *   in a fixed order that depends on the padded design size alone).
 * gpb_emu_sobol: through the linear observable transform f_m = mu_m + sum_p A_pm m_p (PCA modes: the transform's A; no-PCA modes:
 *   scale_m on GP m alone): mean [M] = mu_m + sum_p A_pm e_p, var [M] = V_all, first [M, d] = V_{j} / V, total [M, d] =
 *   1 - V_{all \ j} / V with V_S(m) = sum_pq A_pm A_qm (H^pq_S - e_p e_q).  In the two EXPDIAG modes these describe the
 *   log-observable (the transform in front of the exp), which is what is linear in the GPs.
 * gpb_emu_main_effect: curve [G, M] = E[f_m | x_j = t_g] = mu_m + sum_p A_pm c_p sum_i alpha_pi exp(-(t_g - x_ij)^2 / 2 l_pj^2)
 *   prod_{l != j} I^p_l(x_il) on the grid t [G] (same convention for the EXPDIAG modes).
 * lo_host / hi_host [d] are host arrays; on_device says where the outputs (and t) live (0: host, the call synchronises; 1: device
 * memory, asynchronous).  Only the N design points are visited.  Length scales far below the box width make Q factors underflow to
 * zero; the products are formed without quotients, so such terms are 0, never NaN.
 * Errors: GPB_E_STATE without a factorisation, on a gpb_gp_set_multi context and (the gpb_emu_ calls) without a transform;
 * GPB_E_ARG for a Matern kernel (a function of the full scaled distance, not a product over dimensions: no closed form), for a
 * context with a parameter map (not linear in the original parameters), hi <= lo in any dimension, j outside [0, d), G < 1, more
 * than 361 GPs or 16320 design points.  The factorisation, alpha and the predict workspace are untouched. */
GPB_API int gpb_gp_sobol(gpb_ctx* ctx, const double* lo_host /*[d]*/, const double* hi_host /*[d]*/, int on_device,
                 double* e /*[P]*/, double* H /*[P,P,2d+1]*/);
GPB_API int gpb_emu_sobol(gpb_ctx* ctx, const double* lo_host /*[d]*/, const double* hi_host /*[d]*/, int on_device,
                  double* mean /*[M]*/, double* var /*[M]*/, double* first /*[M,d]*/, double* total /*[M,d]*/);
GPB_API int gpb_emu_main_effect(gpb_ctx* ctx, const double* lo_host /*[d]*/, const double* hi_host /*[d]*/, int64_t j,
                        const double* t /*[G]*/, int64_t G, int on_device, double* curve /*[G,M]*/);

/* ---- variance-reduction sequential design: where the next model runs go ------------------------------------------------ *
 * (the reference's design.py is a one-shot space-filling generator — gpb_maxpro_lhd below is its counterpart; nothing there
 * chooses a second wave from a fitted emulator.)
 * Needs only what is resident after gpb_gp_factor — X, theta, L^-1 — and no training output.  For GP p, amplitude c, kernel k,
 * tau = sigma_n^2 + alpha, v(a) = L^-1 k(X, a), the posterior covariance of the latent function (no White term) is
 *   s(a, b) = c k(a, b) - v(a)^T v(b)
 * and a new run at x, observed with the training runs' noise, conditions every GP of every context at once:
 *   s'(a, b) = s(a, b) - s(a, x) s(x, b) / (s(x, x) + tau)
 * With candidates x_c [C, d], reference points x_r [R, d] of weights w_r >= 0 (sum 1) and GP weights g_p >= 0 the score
 *   J(c) = sum_p g_p [sum_r w_r s_p(r, c)^2] / (s_p(c, c) + tau_p)
 * is exactly the drop of sum_p g_p sum_r w_r s_p(r, r) when x_c joins the design (active learning Cohn; Seo et al. 2000).
 * gpb_design_begin builds the context's design workspace on its stream: V_c, V_r, S_rc = c k(x_r, x_c) - V_r^T V_c [P, R, C]
 *   (an fp64 MFMA product over the design's rows; padding rows contribute exactly zero) and s(c, c).  All three kernel families.
 *   The points are in the GPs' input space: a caller with a parameter map applies gpb_param_map first.  Xc, Xr, w are device
 *   arrays (copied: they may be released after the call), g a host array.
 * gpb_chain_design_run enqueues the whole greedy loop of T picks with no host synchronisation, over the E contexts of a chain
 *   (E = 1: one emulator): J = fl(fl(J_1 + J_2) + J_3 ...) in the order of ctxs, each J_e summed over its GPs in index order;
 *   step t takes the eligible candidate with the largest J (the lowest index on exact ties), clears its flag and conditions
 *   every s_p on it by the rank-one formula.  eligible [C] (uint8, device, in/out; NULL: all), picks [T] (int32), gain [T] =
 *   J_t(pick_t), scores [T, C] or NULL (ineligible entries -inf): device arrays, valid once the stream has run.  With fewer than T
 *   eligible candidates the remaining picks are -1 and their gain NaN.  A run conditions the workspace in place: another run
 *   needs another gpb_design_begin.  No floating-point atomics; every sum in an order fixed by the padded shapes alone — equal
 *   inputs give equal bits, and step-0 scores do not depend on T; no [C, C] matrix is formed.
 * gpb_design_set_noise (optional, between gpb_design_begin and gpb_chain_design_run): candidate c is observed with its own
 *   tau_p(c) = sigma_n^2 + (alpha + s_c[p][c]) in J's denominator and in the rank-one conditioning — a candidate run with larger
 *   statistical errors teaches less (the design counterpart of gpb_gp_set_point_noise; sklearn has none).  s_c_dev [P, C]: device
 *   array of variances >= 0 in GP p's target units (copied; the caller checks its values: a negative or NaN entry gives that
 *   candidate a meaningless score, nothing worse), NULL: back to tau_p.  Not called: tau_p, the same bits as before; a zero array
 *   gives those bits too (alpha + 0 first).  gpb_design_begin resets it.
 * gpb_design_end releases the workspace (synchronises the stream).
 * Errors: GPB_E_STATE without a factorisation, on a gpb_gp_set_multi context, for a run before begin (or after a new
 * factorisation, or a second run), for contexts begun with different C or R; GPB_E_ARG for C, R or T < 1, C or R > 8192, T > C,
 * a negative g, more than 32 contexts, contexts on different streams; gpb_design_set_noise: GPB_E_STATE before gpb_design_begin or
 * after the run that consumed it.  The factorisation and alpha are untouched.  The predict
 * workspace does NOT survive gpb_design_begin: it holds the reference points' K*^T afterwards and may have been re-allocated;
 * later predict / likelihood calls recompute it and return what they would have returned before. */
GPB_API int gpb_design_begin(gpb_ctx* ctx, const double* Xc_dev /*[C,d]*/, int64_t C, const double* Xr_dev /*[R,d]*/, int64_t R,
                     const double* w_dev /*[R]*/, const double* g_host /*[P]*/);
GPB_API int gpb_design_set_noise(gpb_ctx* ctx, const double* s_c_dev /*[P,C] or NULL*/);
GPB_API int gpb_chain_design_run(gpb_ctx* const* ctxs, int E, int64_t T, uint8_t* eligible_dev /*[C] or NULL*/,
                         int32_t* picks_dev /*[T]*/, double* gain_dev /*[T]*/, double* scores_dev /*[T,C] or NULL*/);
GPB_API int gpb_design_end(gpb_ctx* ctx);

/* ---- posterior-predictive summaries of a whole chain ----------------------------------------------------------------------- *
 * gpb_emu_predict_diag <- Chain._predict's per-emulator call, mean and np.diagonal(cov) only  src/mcmc.py:153-166, src/emulator.py:553-605
 * gpb_ppd_summary      <- what examples/ClosureTest.ipynb and PlotMCMC.ipynb take from `_predict(posteriorSamples)` — the reference
 *                         for fifteen samples, because the [S, nobs, nobs] covariance is all `_predict` returns — for every sample
 *                         of a chain: bands of the means, the predictive distribution with the emulator's own uncertainty, and where
 *                         the measurement sits in it.  Closed form, nothing sampled.
 * gpb_emu_predict_diag: gpb_emu_predict without the [W, M, M] array, written observable-major: element (m, w) at m * ld + w, ld >= W;
 *   mean_T[m][w] is bit for bit gpb_emu_predict's mean[w][m] and var_T[m][w] its cov[w][m][m] — the same predict launch and the same
 *   transform arithmetic — in all four GPB_MODE_*, with and without extra_std, under whichever predict arithmetic key 51 selects.
 *   Columns w >= W of the rows are not touched: a long chain goes through slab by slab into one [M, S] array by advancing the
 *   pointers.  Xs are GP-input-space rows (a caller with a parameter map applies gpb_param_map first); Xs, extra_std and the outputs
 *   live where on_device says (0: host, the call synchronises; 1: device, asynchronous).  var_T may be NULL.
 *   Errors: those of gpb_emu_predict, and GPB_E_ARG for ld < W.
 * gpb_ppd_summary: every observable row m of mu_T / var_T [M, ld] (device arrays as gpb_emu_predict_diag writes them; var_T may be
 *   NULL = 0) reduced over its samples s < S <= ld.  The context gives the device and the stream only: no GP state is needed, and M
 *   is the caller's (the rows of several emulators in one array).  q_host [nq]: levels in [0, 1], 1 <= nq <= 16.  vadd_dev [M] or
 *   NULL: a variance added to every sigma_s^2 of row m (the experimental variance for the PIT); yobs_dev [M]: the measurement.
 *   Outputs (NULL: skipped, its work too), in host memory when on_device = 0 (the call synchronises) or device memory (asynchronous):
 *     moments [M, 3]    E_s mu | E_s sigma^2 (the emulator part; 0 without var_T) | E_s (mu - E mu)^2 (the parameter part, two
 *                       passes, divided by S): by the law of total variance the last two sum to the predictive variance
 *     order [M, nq, 2]  the order statistics mu_(k) and mu_(min(k + 1, S - 1)) of the row, k = floor(q (S - 1)): the two neighbours
 *                       numpy's default ("linear") percentile interpolates between, exact (a radix select, nothing is sorted)
 *     mixq [M, nq]      the q-quantile of the predictive mixture F_m(y) = 1/S sum_s Phi((y - mu_s) / tau_s), tau_s^2 =
 *                       max(sigma_s^2 + vadd_m, 0): exactly 64 halvings of [min_s(mu_s - 9 tau_s), max_s(mu_s + 9 tau_s)] (mid =
 *                       (a + b) / 2; F(mid) < q moves a, otherwise b; stops early only when mid is no longer strictly inside), the
 *                       result is b; a sample with tau_s = 0 contributes the step y >= mu_s; q = 0 gives -inf, q = 1 +inf
 *     pit [M]           F_m(yobs_m): the per-observable posterior-predictive p-value
 *   F is a sum of erfc / 2 in a fixed tree whose shape depends on S alone; no floating-point atomics: a row's bits do not depend on
 *   M, on the other rows, on ld or on which outputs share the call, and on_device 0 and 1 give the same bits.  Inputs must be
 *   finite (the caller checks).
 *   Errors (GPB_E_ARG): S < 1 or M < 1 (or either above 2^31 - 1), ld < S, nq outside 1 .. 16, a level outside [0, 1], with mixq a
 *   level strictly between 0 and 1e-15 or strictly between 1 - 1e-15 and 1 (beyond the bracket's reach), mixq with neither var_T
 *   nor vadd, pit without yobs. */
GPB_API int gpb_emu_predict_diag(gpb_ctx* ctx, const double* Xs /*[W,d]*/, int64_t W, int on_device,
                         const double* extra_std /*[W] or NULL*/, double* mean_T /*[M,ld]*/, double* var_T /*[M,ld] or NULL*/,
                         int64_t ld);
GPB_API int gpb_ppd_summary(gpb_ctx* ctx, const double* mu_T /*[M,ld] dev*/, const double* var_T /*[M,ld] dev or NULL*/,
                    int64_t M, int64_t S, int64_t ld, const double* q_host /*[nq]*/, int nq,
                    const double* vadd_dev /*[M] or NULL*/, const double* yobs_dev /*[M] or NULL*/, int on_device,
                    double* moments /*[M,3] or NULL*/, double* order /*[M,nq,2] or NULL*/, double* mixq /*[M,nq] or NULL*/,
                    double* pit /*[M] or NULL*/);

/* ---- convergence diagnostics of a resident chain ---------------------------------------------------------------------------- *
 * gpb_mcmc_diag <- emcee's autocorr.integrated_time (function_1d, auto_window) behind EnsembleSampler.get_autocorr_time — the
 *                  reference's sampler class is emcee's (src/mcmc.py:68-92), and neither it nor emcee has an R-hat — for a chain
 *                  that already lies in device memory: the walker-averaged autocorrelation function, the integrated autocorrelation
 *                  time with emcee's automatic window, and split-R-hat (Gelman et al., BDA3 section 11.4), per parameter j < d.
 *   The context gives the device and the stream only: no GP state is needed, the factorisation, the predict workspace and everything
 *   else in the context are untouched.  x_dev: element (step t, walker w, parameter j) at t * step_stride + w * walker_stride + j —
 *   the sampler's [nsteps, nwalkers, d] store and the pickles' [nwalkers, nsteps, d], or a thinned / cut view of either, without a
 *   copy.  Outputs (NULL: skipped) in host memory when on_device = 0 (the call synchronises) or device memory (asynchronous).
 *   Per (parameter j, walker w): the mean over t, two passes in a fixed order; y_w(t) the centred series; c0_w = sum_t y_w(t)^2.
 *   A walker all of whose values of parameter j are equal never moved (decided by comparing the values, not from a rounded mean: its
 *   mean is its value and c0_w == 0 exactly; so is one whose differences are so small that their squares underflow): it is left
 *   out of parameter j's average and counted in nconst[j] (DEVIATION: emcee divides by its c0 and returns NaN for the whole
 *   parameter).  If all walkers of j are constant: rho[j, :], tau[j], rhat[j] = NaN and window[j] = -1.
 *     rho [d, max_lag + 1]  rho[j, k] = mean over the walkers that moved of  sum_t y_w(t) y_w(t + k) / c0_w: raw lag sums, no
 *                           1 / (n - k) factor — what emcee's zero-padded FFT yields.  Computed as the diagonal sums of Y Y^T, Y[t, w] =
 *                           y_w(t) / sqrt(c0_w), 64 x 64 blocks within max_lag of the diagonal only.
 *     tau [d], window [d]   taus[m] = 2 sum_{k <= m} rho[j, k] - 1, accumulated sequentially in k; window[j] = the first m in [0,
 *                           max_lag] with m >= c taus[m] (emcee's auto_window); tau[j] = taus[window[j]].  No such m within max_lag:
 *                           window[j] = max_lag with bit 30 set (GPB_DIAG_NO_WINDOW) and tau[j] = taus[max_lag].  (DEVIATION: when
 *                           every m is "still inside", emcee's np.argmin over an all-True mask returns window 0; that quirk is not
 *                           reproduced.)
 *     moments [d, 3]        the mean over all draws | W | B of split-R-hat: halves of h = nsteps / 2 draws, the first t < h, the second
 *                           t >= nsteps - h (the middle draw of an odd nsteps is dropped); W = the mean over the 2 nwalkers
 *                           half-walkers of their sample variances (divisor h - 1); B = h times the sample variance (divisor
 *                           2 nwalkers - 1) of their means.  Constant walkers are included.
 *     rhat [d]              sqrt(((h - 1) / h W + B / h) / W)
 *     nconst [d]            walkers of parameter j that never moved
 *   No floating-point atomics; every sum runs in an order fixed by the padded shapes (nsteps to 64, nwalkers to 16) alone.  A
 *   parameter's bits do not depend on d or on the other parameters, on which of the layouts the data arrived in, on on_device, or on
 *   which outputs share the call.  A lag's block partials are added in an order that depends on nsteps only: rho[j, k], k <= L, is
 *   bit for bit the same for every max_lag >= L, hence tau and window do not depend on max_lag whenever the window lies inside it.
 *   Workspace: Y and the per-block lag partials, from the context's buffer cache; the parameters are processed in groups that keep
 *   it under GPB_DIAG_WS_MB megabytes (one parameter at a time where a single one needs more: nsteps = 5000, nwalkers = 4096 is
 *   166 MB per parameter).  The grouping changes no bit.
 *   Inputs must be finite (the caller checks).
 *   Errors (GPB_E_ARG): nsteps < 4; nwalkers < 1 or d < 1; nsteps, nwalkers or d above 2^31 - 1; max_lag outside [0, nsteps - 1];
 *   c <= 0 or not finite; strides that let two elements alias: walker_stride < d, step_stride < d, or neither step_stride >=
 *   walker_stride * nwalkers nor walker_stride >= step_stride * nsteps. */
#define GPB_DIAG_NO_WINDOW (1 << 30)
#define GPB_DIAG_WS_MB 512
GPB_API int gpb_mcmc_diag(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d,
                  int64_t step_stride, int64_t walker_stride, int64_t max_lag, double c, int on_device,
                  double* rho /*[d,max_lag+1] or NULL*/, double* tau /*[d] or NULL*/, int32_t* window /*[d] or NULL*/,
                  double* moments /*[d,3] or NULL*/, double* rhat /*[d] or NULL*/, int32_t* nconst /*[d] or NULL*/);

/* ---- rank-normalised convergence diagnostics of a resident chain -------------------------------------------------------------- *
 * gpb_chain_rank_diag <- Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021, Bayesian Analysis 16): rank-normalised split-R-hat
 *                        (bulk and folded) and the effective sample sizes of the bulk, the mean and the quantile indicators, per
 *                        parameter j < d, for a chain that already lies in device memory — what Stan, `posterior` and ArviZ report;
 *                        the reference has no convergence check at all.  This comment is the specification (tests/rank_reference.py
 *                        restates it in numpy / scipy); where it differs from ArviZ it says DEVIATION.
 *   The context gives the device, the stream and the buffer cache only, as for gpb_mcmc_diag; x_dev, the strides and the two layouts
 *   as gpb_mcmc_diag reads them.  Outputs (NULL: skipped, with the work only it needs) in host memory when on_device = 0 (the call
 *   synchronises) or device memory (asynchronous).  Values must be finite (the caller checks).
 *   Kept draws: h = nsteps / 2; split chain c = w holds steps t < h of walker w, c = nwalkers + w steps t >= nsteps - h.  The middle
 *   step of an odd nsteps enters nothing below (DEVIATION: ArviZ takes its quantiles before the split).  m = 2 nwalkers split chains
 *   of h draws, n = m h.  -0.0 counts as +0.0.
 *   Ranks: r = the average rank (1-based; ties share the mean of their positions: scipy.stats.rankdata(method="average")) of a value
 *   among all n kept values of its parameter; z = Phi^-1((r - 3/8) / (n + 1/4)) (csrc/ndtri.h: AS 241).
 *   Series per parameter, K = 2 + nq: (a) z; (b) x; (c) per level p = probs[k] the 0 / 1 series I(x <= q_p), q_p = np.quantile(kept,
 *   p) bit for bit (the order statistics at floor(p (n - 1)) and the next, numpy's interpolation).  For R-hat only: (d) z of the ranks
 *   of |x - med|, med = np.median(kept) = the mean of the two middle order statistics.
 *   R-hat of a series as [m, h]: W = the mean of the chains' sample variances (divisor h - 1), B = h times the sample variance
 *   (divisor m - 1) of their means, sqrt(((h - 1) / h W + B / h) / W); NaN when the numerator is 0.
 *   ESS of a series: acov_c(t) = (1 / h) sum_s y_c(s) y_c(s + t), y_c centred by the chain's own mean (biased, no wrap-around), A(t) =
 *   its mean over the chains — the t-th diagonal sum of Y^T Y, Y[s, c] = y_c(s), over m h; mean_var = A(0) h / (h - 1); var_plus =
 *   mean_var (h - 1) / h + the sample variance of the chain means; rho(t) = 1 - (mean_var - A(t)) / var_plus, rho(0) = 1.  Then Stan's
 *   estimator (Geyer's initial positive sequence, then the initial monotone sequence), every sum sequential in t:
 *       re = 1; ro = rho(1); R[0] = 1; R[1] = ro; t = 1
 *       while t < h - 3 and re + ro > 0:  re = rho(t + 1); ro = rho(t + 2); if re + ro >= 0: R[t + 1] = re, R[t + 2] = ro;  t += 2
 *       max_t = t - 2;  if re > 0: R[max_t + 1] = re
 *       for t = 1, 3, ... <= max_t - 2:  if R[t + 1] + R[t + 2] > R[t - 1] + R[t]: R[t + 1] = R[t + 2] = (R[t - 1] + R[t]) / 2
 *       tau = -1 + 2 sum(R[0 .. max_t]) + R[max_t + 1];  tau = max(tau, 1 / log10(n));  ess = n / tau
 *   (entries of R never set are 0).  A chain all of whose values are equal has its value as its mean and variance 0, and chain means
 *   that are all equal have variance 0, both exactly; a series with var_plus == 0 (a parameter that never varies, an indicator that
 *   is all 0 or all 1) has ess = NaN and stop = -1 (DEVIATION: ArviZ returns n).  Only lags <= max_lag <= h - 1 are formed: when the
 *   first loop needs rho beyond max_lag, stop = max_lag with bit 30 set (GPB_RANK_NO_BAND) and ess = NaN — the caller widens the
 *   band.  rho(k) has the same bits for every band that holds k, so no result depends on where such a search started.
 *     rank2 [d, n] (int64)  2 r of the kept draws in (step, walker) order: draw (kept step tk < 2 h, walker w) at tk nwalkers + w
 *                           (written straight into device memory with on_device = 1; for host memory it is staged on the device
 *                           first, 8 d n bytes that stay in the context's buffer cache: ask for it where it is wanted)
 *     median [d]            med
 *     quant [d, nq]         q_p
 *     rhat [d, 2]           R-hat of (a) — bulk — and of (d) — folded
 *     ess [d, K]            of (a), (b), (c) in the order of probs
 *     stop [d, K] (int32)   max_t, or max_lag | GPB_RANK_NO_BAND, or -1
 *     sd [d]                sqrt(var_plus) of (b)
 *   The rank transform is a device radix sort (eight-bit digits, least significant first, every pass stable; a digit all keys share
 *   is skipped) of the order-preserving keys of one parameter's kept draws, twice when rhat is asked for.  No floating-point
 *   atomics; every sum runs in an order fixed by the padded shapes (h to 64, m to 16) alone.  A parameter's bits do not depend on d,
 *   on the other parameters, on the layout, on on_device, on the levels other than its own, or on which outputs share the call.
 *   Workspace: the sort's buffers of one parameter (24 n bytes and the ranks, 8 n), and Y with its lag partials for a group of
 *   parameters, from the context's buffer cache; the groups keep it under GPB_RANK_WS_MB megabytes (one parameter at a time where a
 *   single one needs more).  The grouping changes no bit.
 *   Errors (GPB_E_ARG): nsteps < 4; nwalkers < 1 or d < 1; nsteps, nwalkers or d above 2^31 - 1; n above 2^31 - 1; nq outside 1 ... 8;
 *   a level outside (0, 1); max_lag outside [0, h - 1]; strides that let two elements alias (gpb_mcmc_diag's rule). */
#define GPB_RANK_NO_BAND (1 << 30)
#define GPB_RANK_MAX_Q 8
#define GPB_RANK_WS_MB 1024
GPB_API int gpb_chain_rank_diag(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d,
                  int64_t step_stride, int64_t walker_stride, const double* probs_host /*[nq]*/, int nq, int64_t max_lag,
                  int on_device, int64_t* rank2 /*[d,n] or NULL*/, double* median /*[d] or NULL*/, double* quant /*[d,nq] or NULL*/,
                  double* rhat /*[d,2] or NULL*/, double* ess /*[d,2+nq] or NULL*/, int32_t* stop /*[d,2+nq] or NULL*/,
                  double* sd /*[d] or NULL*/);

/* ---- corner-plot marginals of a resident chain ------------------------------------------------------------------------------ *
 * gpb_chain_marginals <- examples/PlotMCMC.ipynb (plot_corner_1dataset): `ax.hist(samples[:, i], bins=20)` per parameter and
 *                        `ax.hist2d(samples[:, j], samples[:, i], bins=20)` per pair — np.histogram and np.histogram2d of every column
 *                        and column pair, for a chain that already lies in device memory, all pairs in one call.
 *   The context gives the device, the stream and the buffer cache only: no GP state is needed, the factorisation, the predict
 *   workspace and everything else in the context are untouched.  x_dev: element (step t, walker w, parameter j) at t * step_stride +
 *   w * walker_stride + j, exactly as gpb_mcmc_diag reads it — the sampler's [nsteps, nwalkers, d] store, the pickles' [nwalkers,
 *   nsteps, d], a chain[discard::thin] view of either, without a copy; a flat [S, d] particle set is nsteps = S, nwalkers = 1.
 *   edges_host [d, B + 1]: the bin edges of every parameter, taken as given (they need not be uniform).
 *   BIN RULE: a value x of parameter j is in bin b iff e[j][b] <= x < e[j][b + 1]; the last bin also takes x == e[j][B]; anything
 *   else, NaN included, is outside for j.  That is bit for bit what np.histogram(x, bins=e) and np.histogram2d(..., bins=[ei, ej])
 *   count, and their bins=B, range=(lo, hi) forms when e = np.linspace(lo, hi, B + 1).  A value is searched in the edges; no bin
 *   index is computed from (x - lo) / (hi - lo) * B.
 *   pairs_host [npairs, 2] (int32) or NULL = all i < j in lexicographic order, npairs = d (d - 1) / 2.
 *   Outputs (NULL: skipped, its work too) in host memory when on_device = 0 (the call synchronises) or device memory (asynchronous):
 *     h1 [d, B]            h1[j][b]: the samples of parameter j in bin b
 *     h2 [npairs, B, B]    h2[p][bi][bj]: the samples with parameter pairs[p][0] in bin bi and parameter pairs[p][1] in bin bj; a
 *                          sample outside for either parameter is not counted, as in histogram2d
 *     outside [d]          the samples outside for j
 *   WEIGHT RULE: with w_dev [nsteps] (nwalkers == 1 only: a particle set) sample t adds the integer q_t = llrint(w_t * wscale)
 *   (round half to even), clamped to [0, 2^32], NaN giving 0, instead of 1 — to h1, h2 and outside alike.  The caller passes wscale
 *   = 2^32 / max w: the resolution is 2^-32 of the largest weight and the sums are exact in int64 ((2^31 - 1) 2^32 < 2^63); numpy
 *   reproduces them with np.rint(w * wscale).astype(np.int64) and np.add.at.
 *   All accumulation is integer (LDS and global integer atomics); no floating-point sum appears anywhere.  The counts therefore do
 *   not depend on arrival order, on which of the layouts the data arrived in, on on_device, on the pairs that share the call or on
 *   which outputs are requested.  Workspace, from the context's buffer cache: one byte per (sample, parameter) — its bin, or 255 —
 *   written by the pass that reads the chain once and read by the pair pass; the samples go through in groups that keep it under
 *   GPB_MARG_WS_MB megabytes, and the grouping changes no count.
 *   Errors (GPB_E_ARG): nsteps, nwalkers or d below 1 or above 2^31 - 1; B outside 1 .. 64; edges that are not finite and strictly
 *   increasing; a pair index outside [0, d) or a pair (i, i); npairs < 0; pairs_host == NULL with npairs != d (d - 1) / 2 (checked
 *   when h2 is requested); npairs B^2 above 2^31 - 1; strides that let two elements alias (gpb_mcmc_diag's rule); weights with
 *   nwalkers != 1; with weights a wscale that is not finite and positive. */
#define GPB_MARG_WS_MB 512
GPB_API int gpb_chain_marginals(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d,
                        int64_t step_stride, int64_t walker_stride, const double* edges_host /*[d,B+1]*/, int B,
                        const int32_t* pairs_host /*[npairs,2] or NULL = all i<j, lexicographic*/, int64_t npairs,
                        const double* w_dev /*[nsteps] or NULL*/, double wscale, int on_device,
                        int64_t* h1 /*[d,B] or NULL*/, int64_t* h2 /*[npairs,B,B] or NULL*/, int64_t* outside /*[d] or NULL*/);

/* ---- posterior bands of the parametrised curves, closure distance, trace histograms ------------------------------------------ *
 * gpb_chain_curves     <- examples/PlotMCMC.ipynb (plot_zeta_s_posterior, plot_eta_s_posterior, plot_yloss_posterior): the posterior
 *                         of the functions zeta/s (T), eta/s (mu_B), <y_loss> (y_init) — `np.percentile(curves[S, 100], ..., axis=0)`
 *                         over ALL samples of a chain — and (compute_Delta_d, create_Delta_d_distribution) the closure distance
 * gpb_chain_trace_hist <- plot_chain_histogram: `np.histogram2d(step, value, bins=[n_steps, 30])` per parameter
 *   The context gives the device, the stream and the buffer cache only.  x_dev, nsteps, nwalkers, d and the strides exactly as
 *   gpb_chain_marginals reads them (the same aliasing rule; a flat [S, d] set is nsteps = S, nwalkers = 1).
 * gpb_chain_curves: sample s = t * nwalkers + w, whatever the memory layout; S = nsteps nwalkers <= 2^31 - 1.  Curve c < ncurves
 *   has the descriptor desc_host[c] = (fn, col0, col1, col2, col3) and the grid grid_host[c][0 .. G); its value for sample s at grid
 *   point g is v(c, g, s) = curve_value(fn, theta_s[cols], aux, grid[c][g]) of csrc/curve_fn.h, every operation rounded on its own
 *   (no fused multiply-add), as numpy's vectorised forms round them:
 *     fn 0  zeta/s   cols (zmax, T0, sigma+, sigma-):  zmax exp(-((g - T0) (g - T0)) / (2 (s s))),  s = sigma- if g < T0 else sigma+
 *     fn 1  eta/s    cols (e0, e2, e4; col3 = -1): 0 <= g <= 0.2: e0 + (e2 - e0) (g / 0.2); 0.2 < g < 0.4: e2 + (e4 - e2) ((g - 0.2)
 *                    / 0.2); g >= 0.4: e4; g < 0: 0
 *     fn 2  y_loss   cols (y2, y4, y6; col3 = -1): 0 <= g <= 2: y2 (g / 2); 2 < g < 4: y2 + (y4 - y2) ((g - 2) / 2); g >= 4: y4 +
 *                    (y6 - y4) ((g - 4) / 2); g < 0: 0
 *     fn 3  delta    (sum_j ((theta_j - truth_j) / width_j)^2) / d, j ascending, one add after the other; aux_host = truth [d] |
 *                    width [d]; the columns and the grid value are ignored
 *   Outputs (NULL: skipped, its work too) in host memory when on_device = 0 (the call synchronises) or device memory (asynchronous):
 *     order [ncurves, G, nq, 2]   the order statistics v_(k) and v_(min(k + 1, S - 1)) over s, k = floor(q (S - 1)) — gpb_ppd_summary's
 *                                 contract, the levels converted as it converts them.  Exact: a radix select on the order-preserving
 *                                 64-bit key, eight passes of 8 bits; nothing is sorted or interpolated.  NO [G, S] ARRAY IS FORMED:
 *                                 every pass evaluates v again from the sample's parameters.  Workspace: 256-bin digit tables and
 *                                 the ranks' prefixes per (curve, grid point, rank) — a function of ncurves, G and nq, not of S.
 *     values [ncurves, G, ldv]    v itself, element (c, g, s) at (c G + g) ldv + s: for small S, and for fn 3, whose [1, S] row feeds
 *                                 gpb_ppd_summary and gpb_chain_marginals.  Evaluated by the same code as the select's passes.
 *   All accumulation is integer (LDS and global integer atomics): the results do not depend on the layout, the slabs the samples are
 *   counted in, on_device, or on the curves and grid points that share the call.  Inputs must be finite (the caller checks).
 *   Errors (GPB_E_ARG): the shapes and strides rule of gpb_chain_marginals; S above 2^31 - 1; ncurves outside 1 .. 8; G outside
 *   1 .. 1024; with order nq outside 1 .. 16 or a level outside [0, 1]; fn outside 0 .. 3; a needed column outside [0, d); fn 3
 *   without aux or with a truth that is not finite or a width that is not finite and positive; values with ldv < S; a grid value that
 *   is not finite.
 * gpb_chain_trace_hist: hist[j][t][b] = the walkers of step t whose parameter j lies in bin b of edges_host [d, B + 1] by
 *   gpb_chain_marginals' BIN RULE (searched in the edges, the last edge inclusive, NaN and the rest outside -> outside[j][t]).
 *   Integer counts, written once per (step, parameter): no dependence on layout or on_device.  The step axis needs no binning:
 *   histogram2d's bins = n_steps over [0, n_steps - 1] puts step t in bin t.
 *   Errors (GPB_E_ARG): the shapes and strides rule; B outside 1 .. 64; edges that are not finite and strictly increasing. */
GPB_API int gpb_chain_curves(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d,
                     int64_t step_stride, int64_t walker_stride, int ncurves, const int32_t* desc_host /*[ncurves,5]*/,
                     const double* aux_host /*[2d] or NULL*/, const double* grid_host /*[ncurves,G]*/, int G,
                     const double* q_host /*[nq]*/, int nq, int on_device, double* order /*[ncurves,G,nq,2] or NULL*/,
                     double* values /*[ncurves,G,ldv] or NULL*/, int64_t ldv);
GPB_API int gpb_chain_trace_hist(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d,
                         int64_t step_stride, int64_t walker_stride, const double* edges_host /*[d,B+1]*/, int B, int on_device,
                         int64_t* hist /*[d,nsteps,B] or NULL*/, int64_t* outside /*[d,nsteps] or NULL*/);

/* ---- response matrix and Fisher information over a set of posterior rows ------------------------------------------------------ *
 * gpb_sens_accumulate <- examples/SensitivityAnalysis.ipynb: the observable-by-parameter response matrix `(Y+ - Y-) / (2 h) * x /
 *                        ((Y+ + Y-) / 2)` of 2 d finite-difference predictions at one design point — here in its analytic limit, from
 *                        the Jacobian gpb_emu_predict_jac gives, summed over all rows of a chain — and the matrix that weighs the
 *                        response by the uncertainties, J^T C^-1 J with the likelihood's covariance (src/mcmc.py:288-290).
 *   The context gives the device, the stream and the buffer cache only; M and d are the caller's.  All arrays are device memory.
 *   Per row w, with Cw = C[w] + Cadd = L L^T (C_dev IS DESTROYED: large rows are factorised in place):
 *     F_w [d, d]   = J^T Cw^-1 J, formed as (L^-1 J)^T (L^-1 J); both triangles are stored and hold the same bits
 *     R_w [M, d]   = (x_j J_mj) / y_m                 (a zero y_m gives IEEE inf / NaN in that entry's sums only)
 *     I_w [M, d]   = (J_mj J_mj) / Cw_mm              (the information observable m alone carries)
 *   A row whose Cw has a non-positive pivot is BAD: it contributes what a row of weight 0 contributes — nothing, no NaN — and
 *   adds 1 to cnt[1].  A row with wt == 0 is skipped the same way and is not counted; nothing of it is read into a sum.
 *   acc_dev [GPB_SENS_ACC_DOUBLES(M, d)], running sums the caller zeroes (with cnt_dev) before the first slab:
 *     [0] sum wt | [GPB_SENS_ACC_F] sum wt F [d, d] | [GPB_SENS_ACC_R] sum wt R [M, d] | [GPB_SENS_ACC_R2] sum wt (R R) [M, d] |
 *     [GPB_SENS_ACC_I] sum wt I [M, d];   cnt_dev [2]: rows seen so far (cnt[0] += W), bad rows so far.
 *   Equal inputs give equal bits, however the rows are split into calls: no floating-point atomics; rows are summed in chunks
 *   of 256 consecutive rows, each by one fixed tree (sixteen runs of sixteen rows), the chunk sums are added to acc in chunk
 *   order by one thread per entry, and a call whose cnt[0] at entry is not a multiple of 256 is refused.  Any sequence of slabs
 *   whose sizes are multiples of 256, except the last, leaves the bits of one call on all rows.  The call reads cnt[0] back
 *   (one stream synchronisation); the kernels are asynchronous.
 *   Cw and L^-1 J live in LDS while M (M | 1) + M d <= GPB_SENS_LDS_DOUBLES, in the row's slab of C_dev and a workspace above.
 *   Errors: GPB_E_ARG for a null pointer (Cadd_dev and wt_dev may be NULL), W < 0 or above 2^31 - 1, M or d < 1, M > 2048,
 *   d > 64; GPB_E_STATE for a call that does not start on a chunk boundary.  A refused call writes nothing.  W == 0 is a no-op. */
#define GPB_SENS_MAX_M 2048
#define GPB_SENS_MAX_D 64
#define GPB_SENS_LDS_DOUBLES 8064
#define GPB_SENS_ACC_F 1
#define GPB_SENS_ACC_R(M, d) (1 + (int64_t)(d) * (d))
#define GPB_SENS_ACC_R2(M, d) (1 + (int64_t)(d) * (d) + (int64_t)(M) * (d))
#define GPB_SENS_ACC_I(M, d) (1 + (int64_t)(d) * (d) + 2 * (int64_t)(M) * (d))
#define GPB_SENS_ACC_DOUBLES(M, d) (1 + (int64_t)(d) * (d) + 3 * (int64_t)(M) * (d))
GPB_API int gpb_sens_accumulate(gpb_ctx* ctx, int64_t W, int64_t M, int64_t d, const double* J_dev /*[W,M,d]*/,
                        const double* y_dev /*[W,M]*/, double* C_dev /*[W,M,M], destroyed*/, const double* Cadd_dev /*[M,M] or NULL*/,
                        const double* x_dev /*[W,d]*/, const double* wt_dev /*[W] or NULL*/,
                        double* acc_dev /*[GPB_SENS_ACC_DOUBLES(M,d)]*/, int64_t* cnt_dev /*[2]*/);

/* ---- goodness of fit and data-set influence over a set of posterior rows -------------------------------------------------------- *
 * gpb_gof_accumulate <- src/mcmc.py:23-65 (mvn_loglike): its two pieces, 1/2 dY^T C^-1 dY and sum ln L_ii, which the reference adds
 *                       up over all emulators and returns as one number — here kept per row and emulator, with the whitened
 *                       residuals and the closed-form predictive p-value, so that a calibration can be judged data set by data set
 *                       (examples/ClosureTest.ipynb judges it by eye from fifteen predictive curves).
 *   The context gives the device, the stream and the buffer cache only; M is the caller's.  All arrays are device memory.
 *   Per row w, with dY = y[w] - yexp and Cw = C[w] + Cadd = L L^T (C_dev IS DESTROYED: large rows are factorised in place):
 *     z [M]      = L^-1 dY, the whitened sequential residuals: z_m is the residual of observable m given observables 0 .. m - 1,
 *                  each N(0, 1) if the model describes the data
 *     chi2       = z^T z                          -> chi2_out[w]
 *     ll         = -1/2 chi2 - sum ln L_ii        -> ll_out[w]   (mvn_loglike's value, without the 2 pi constant; log det Cw =
 *                  -2 ll - chi2)
 *     p          = Q(M / 2, chi2 / 2), gpb_chi2_sf's function: the posterior-predictive p-value of the chi2 discrepancy in closed
 *                  form (for y_rep ~ N(mu_w, Cw) the replicate's chi2 is chi2_M exactly; nothing is sampled)
 *     pull [M]   = dY_m / sqrt(Cw_mm), the marginal pulls
 *   chi2_out and ll_out are written at stride 1, W entries each: a caller fills row e of an [E, ld] array slab by slab.
 *   A row whose Cw has a non-positive pivot is BAD: NaN in chi2_out and ll_out, nothing in any sum, 1 added to cnt[1].  A row with
 *   wt == 0 is not evaluated: NaN in chi2_out and ll_out, nothing of it is read into a sum, and it is not counted as bad.
 *   acc_dev [GPB_GOF_ACC_DOUBLES(M)], running sums the caller zeroes (with cnt_dev) before the first slab:
 *     [GPB_GOF_ACC_W] sum wt | [GPB_GOF_ACC_P] sum wt p | [GPB_GOF_ACC_Z] sum wt z [M] | [GPB_GOF_ACC_Z2] sum wt (z z) [M] |
 *     [GPB_GOF_ACC_PULL] sum wt pull [M] | [GPB_GOF_ACC_PULL2] sum wt (pull pull) [M];   cnt_dev [2]: rows seen so far, bad rows so far.
 *   Equal inputs give equal bits, however the rows are split into calls — gpb_sens_accumulate's rules: no floating-point atomics;
 *   chunks of 256 consecutive rows, each summed by one fixed tree (sixteen runs of sixteen rows); the chunk sums added to acc in
 *   chunk order by one thread per entry; a call whose cnt[0] at entry is not a multiple of 256 is refused.  Any sequence of slabs
 *   whose sizes are multiples of 256, except the last, leaves the bits of one call on all rows.  The call reads cnt[0] back (one
 *   stream synchronisation); the kernels are asynchronous.
 *   Cw and z live in LDS while (M + 1) (M | 1) <= GPB_GOF_LDS_DOUBLES (M <= 89), in the row's slab of C_dev and a workspace above.
 *   The dot products of the factorisation and of z are carried in two doubles, as gpb_sens_accumulate carries them.
 *   Errors: GPB_E_ARG for a null pointer (Cadd_dev and wt_dev may be NULL), W < 0 or above 2^31 - 1, M < 1, M > 2048; GPB_E_STATE
 *   for a call that does not start on a chunk boundary.  A refused call writes nothing.  W == 0 is a no-op.
 * gpb_chi2_sf: out[i] = Q(ndf / 2, x[i] / 2), the survival function of the chi-square distribution with ndf degrees of freedom
 *   (regularised upper incomplete gamma function; csrc/chi2_sf.h: the series below x / 2 < ndf / 2 + 1, a continued fraction above,
 *   at most GPB_CHI2_SF_MAX_ITER steps of either).  NaN in gives NaN out; x <= 0 gives 1.  ndf finite and positive, not necessarily
 *   an integer.  Relative error a few 1e-15 at small ndf, growing to ~1e-12 at ndf = 2048 (the prefactor exp(a ln t - t -
 *   lgamma(a)) carries the rounding of terms of size ~1e4).  Errors (GPB_E_ARG): a null pointer, n < 0 or above 2^31 - 1, such an ndf.
 * gpb_gof_influence: what the posterior would be WITHOUT data set e, by importance reweighting.  ll_T [E, ld]: row e holds the
 *   ll of emulator e for the S rows (gpb_gof_accumulate's ll_out).  Per emulator the weights w_s = wt_s exp(-(ll_T[e, s] - min)),
 *   min the minimum of ll_T[e, .] over the rows used, and
 *     out_dev [E, 2 + 2 d]:  sum w | sum w w | sum w x_j [d] | sum w (x_j x_j) [d]
 *   A row with a NaN ll or wt == 0 is skipped by a branch.  The minimum is exact and order free; the sums are the chunk trees above
 *   over s, added in chunk order: equal inputs give equal bits, and a row of out depends neither on E nor on the other rows of ll_T.
 *   An emulator without a usable row leaves zeros.  Errors (GPB_E_ARG): a null pointer (wt_dev may be NULL), E outside 1 .. 64,
 *   d outside 1 .. 512, S < 1 or above 2^31 - 1, ld < S. */
#define GPB_GOF_MAX_M 2048
#define GPB_GOF_MAX_D 512
#define GPB_GOF_MAX_E 64
#define GPB_GOF_LDS_DOUBLES 8064
#define GPB_GOF_ACC_W 0
#define GPB_GOF_ACC_P 1
#define GPB_GOF_ACC_Z 2
#define GPB_GOF_ACC_Z2(M) (2 + (int64_t)(M))
#define GPB_GOF_ACC_PULL(M) (2 + 2 * (int64_t)(M))
#define GPB_GOF_ACC_PULL2(M) (2 + 3 * (int64_t)(M))
#define GPB_GOF_ACC_DOUBLES(M) (2 + 4 * (int64_t)(M))
GPB_API int gpb_gof_accumulate(gpb_ctx* ctx, int64_t W, int64_t M, const double* y_dev /*[W,M]*/, double* C_dev /*[W,M,M], destroyed*/,
                       const double* yexp_dev /*[M]*/, const double* Cadd_dev /*[M,M] or NULL*/, const double* wt_dev /*[W] or NULL*/,
                       double* chi2_out /*[W]*/, double* ll_out /*[W]*/, double* acc_dev /*[GPB_GOF_ACC_DOUBLES(M)]*/,
                       int64_t* cnt_dev /*[2]*/);
GPB_API int gpb_chi2_sf(gpb_ctx* ctx, const double* x_dev /*[n]*/, int64_t n, double ndf, double* out_dev /*[n]*/);
GPB_API int gpb_gof_influence(gpb_ctx* ctx, const double* ll_T /*[E,ld]*/, int64_t E, int64_t S, int64_t ld, const double* x_dev /*[S,d]*/,
                      int64_t d, const double* wt_dev /*[S] or NULL*/, double* out_dev /*[E,2+2d]*/);

/* ---- leave-one-out predictive accuracy: pointwise conditionals, Pareto-smoothed importance sampling, WAIC ------------------------- *
 * The reference has no model comparison; the specification is this comment and the numpy model tests/psis_reference.py.
 * gpb_loo_pointwise: per row w, with dY = y[w] - yexp, Cw = C[w] + Cadd = L L^T, P = Cw^-1 and g = P dY, for every observable m
 *     ll_T[m, w] = -1/2 ln(2 pi / P_mm) - 1/2 g_m^2 / P_mm  =  ln p(y_m | y_-m, theta_w)     (with the 2 pi constant)
 *     zc_T[m, w] = g_m / sqrt(P_mm)      the standardised conditional residual; zc_T may be NULL
 *   the leave-one-out conditionals of a Gaussian that does not factorise (Buerkner, Gabry, Vehtari 2021).  Both outputs are
 *   observable-major, element (m, w) at m * ld + w, as gpb_emu_predict_diag writes.  flag_dev [W] bytes: 1 for a row whose Cw has a
 *   non-positive pivot (its column of both outputs is NaN), else 0.  C_dev IS DESTROYED (rows with M > 89 are worked in place).
 *   One workgroup per row: gpb_gof_accumulate's left-looking Cholesky with z = L^-1 dY as row M of the factor, its dot products in
 *   two doubles; then L is inverted in place row by row, and P_mm = sum_{k >= m} (L^-1)_km^2, g_m = sum_{k >= m} (L^-1)_km z_k in
 *   ascending k.  In LDS while (M + 1) (M | 1) <= GPB_GOF_LDS_DOUBLES.  A row's bits depend on the row alone.
 *   Errors (GPB_E_ARG): a null pointer (Cadd_dev and zc_T may be NULL), W < 0 or above 2^31 - 1, M < 1, M > 2048, ld < W.
 * gpb_psis: Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry, JMLR 2024, as ArviZ's _psislw computes it)
 *   of every row of lr_T [R, ld], S finite log ratios each (the caller checks):
 *     1  x = lr - max(lr)
 *     2  M = min(S // 5, ceil(3 sqrt(S))); cutoff = max((M + 1)-th largest x, ln DBL_MIN) by an exact radix select;
 *        the tail is {x > cutoff}, n_tail its size
 *     3  n_tail <= 4: khat = +inf, nothing is smoothed
 *     4  the tail sorted ascending, ties by sample index; t_j = exp(x_j) - exp(cutoff); the Zhang-Stephens fit of csrc/psis_fit.h:
 *        m_est = 30 + floor(sqrt(n_tail)) candidates b_i = (1 - sqrt(m_est / (i - 1/2))) / (3 t_[floor(n / 4 + 1/2)]) + 1 / t_[n],
 *        k_i = mean log1p(-b_i t), profile weights from n (ln(-b_i / k_i) - k_i - 1), those below 10 eps dropped and the rest
 *        renormalised, bhat = sum w_i b_i, k = mean log1p(-bhat t), sigma = -k / bhat, khat = (n k + 5) / (n + 10)
 *     5  the j-th smallest tail value becomes ln(sigma expm1(-khat log1p(-p_j)) / khat + exp(cutoff)), p_j = (j - 1/2) / n
 *        (-sigma log1p(-p_j) for the fraction at khat == 0); a khat that is not finite smooths nothing
 *     6  values above 0 become 0; lw = x - logsumexp(x); ess = 1 / sum exp(2 lw)
 *   khat [R], n_tail [R], ess [R], lw_T [R, ld]: each may be NULL.  on_device != 0: lr_T and the outputs are device memory and the
 *   call is asynchronous; 0: host memory, staged.  Every sum runs in a tree fixed by S, n_tail and m_est alone, there is no
 *   floating-point atomic, and a row's bits depend on neither R, ld, the other rows, on_device nor the outputs asked for.
 *   Errors (GPB_E_ARG): a null lr_T, R < 1 or above 2^31 - 1, S < 1, ld < S, S > GPB_PSIS_MAX_S = 2^24 (the tail, at most 12288
 *   values, is sorted in LDS).
 * gpb_psis_loo: the same steps on lr = -ll_T [R, ld] (pointwise log-likelihoods of unit r for the S samples) and, in the same
 *   passes, out [R, GPB_LOO_NOUT]:
 *     [GPB_LOO_ELPD] logsumexp(lw + ll) | [GPB_LOO_LPPD] logsumexp(ll) - ln S | [GPB_LOO_PWAIC] the variance of ll, ddof 1, about
 *     the mean of a first pass | [GPB_LOO_KHAT] | [GPB_LOO_ESS] | [GPB_LOO_NTAIL] | [GPB_LOO_PIT] sum exp(lw) Phi(zc_T), Phi from
 *     erfc, NaN when zc_T is NULL | [GPB_LOO_MINLL] min ll.
 *   Errors: those of gpb_psis, and a null out. */
#define GPB_PSIS_MAX_S (1 << 24)
#define GPB_LOO_ELPD 0
#define GPB_LOO_LPPD 1
#define GPB_LOO_PWAIC 2
#define GPB_LOO_KHAT 3
#define GPB_LOO_ESS 4
#define GPB_LOO_NTAIL 5
#define GPB_LOO_PIT 6
#define GPB_LOO_MINLL 7
#define GPB_LOO_NOUT 8
GPB_API int gpb_loo_pointwise(gpb_ctx* ctx, int64_t W, int64_t M, const double* y_dev /*[W,M]*/, double* C_dev /*[W,M,M], destroyed*/,
                      const double* yexp_dev /*[M]*/, const double* Cadd_dev /*[M,M] or NULL*/, double* ll_T /*[M,ld]*/,
                      double* zc_T /*[M,ld] or NULL*/, int64_t ld, unsigned char* flag_dev /*[W]*/);
GPB_API int gpb_psis(gpb_ctx* ctx, const double* lr_T /*[R,ld]*/, int64_t R, int64_t S, int64_t ld, int on_device, double* khat /*[R]*/,
             int64_t* n_tail /*[R]*/, double* ess /*[R]*/, double* lw_T /*[R,ld] or NULL*/);
GPB_API int gpb_psis_loo(gpb_ctx* ctx, const double* ll_T /*[R,ld]*/, const double* zc_T /*[R,ld] or NULL*/, int64_t R, int64_t S,
                 int64_t ld, int on_device, double* out /*[R,GPB_LOO_NOUT]*/);

/* ---- posterior clusters of a resident chain --------------------------------------------------------------------------------- *
 * gpb_chain_kmeans <- examples/generate_posterior_clusters.py: `StandardScaler().fit_transform(chain)`, `KMeans(n_clusters,
 *                     n_init=10).fit(...)`, `scaler.inverse_transform(kmeans.cluster_centers_)` — weighted k-means of the rows of a
 *                     chain that already lies in device memory, R restarts in lock-step: every pass reads a row once per group of
 *                     restarts whose centres fit a workgroup's LDS (all of them at k d <= 200 or so) and serves all their centres.
 *   The context gives the device, the stream and the buffer cache only; no GP state is touched.  x_dev, nsteps, nwalkers, d and the
 *   strides exactly as gpb_chain_marginals reads them (the same aliasing rule; a flat [S, d] set is nsteps = S, nwalkers = 1); the
 *   rows are counted outer axis first (the axis whose stride spans the other).  w_dev [nsteps] or NULL: non-negative weights,
 *   nwalkers == 1 only.  k clusters, R restarts (sklearn's n_init), max_iter >= 1, tol >= 0, standardize 0 / 1.
 *   Exactly one of init_host [R, k, d] (the starting centres, in the chain's own units) and u_host [R, k] (uniforms in [0, 1) that
 *   drive the seeding below) is non-NULL: the device draws no random number.
 *   1. MOMENTS.  Per column the weighted mean and the population standard deviation (ddof = 0), compensated sums in a fixed order.
 *      A column whose values are all equal has mean = that value and scale 1 (decided by min == max, not from a rounded variance);
 *      so has one whose standard deviation is 0.  standardize = 0: mean = 0, scale = 1.  A row with a non-finite coordinate has
 *      weight 0 from here on, label -1, and is counted in n_skipped.  z = (x - mean) / scale is formed on the fly in every pass.
 *   2. SEEDING (u_host): the published k-means++ (Arthur & Vassilvitskii 2007).  Centre 0 of restart r is the first row whose
 *      running weight sum exceeds u[r, 0] W; centre c the first row whose running sum of w_i D_i exceeds u[r, c] sum w D, D_i the
 *      squared distance to the nearest centre chosen so far.  The running sum is hierarchical and fixed by S: one add after the
 *      other over the 64 rows of a wave, the 4 waves of a tile, the tiles of a range, the ranges.  If sum w D == 0 (fewer distinct
 *      rows than centres) centre c repeats centre c - 1.  sklearn's own seeding (greedy, 2 + log k trials, Mersenne stream) is NOT
 *      reproduced; parity with sklearn goes through init_host.
 *   3. LLOYD, sklearn's loop: assign every row to the nearest centre (ties: the lowest index); move every centre to the weighted
 *      mean of its rows; a restart stops when the labels of its rows of positive weight equal the previous iteration's, or when the
 *      summed squared centre shift is <= tol * mean_j var(z_j) (the weighted variances: 1 for a standardised column that is not
 *      constant), or after max_iter iterations; then one more assignment against the final centres gives labels, sizes and the
 *      inertia sum w_i min_c |z_i - c|^2.  n_iter counts as sklearn's n_iter_.  DEVIATION: a cluster that loses all its weight
 *      keeps its centre and reports size 0 (sklearn relocates it).  A stopped restart is frozen while the others go on.
 *   4. The best restart has the lowest inertia; the lowest index wins a tie.
 *   REPRODUCIBLE SUMS: a centre is sum_i llrint(z_ij w_i 2^F) / sum_i llrint(w_i 2^G), 64-bit integer sums (LDS and global integer
 *   atomics) with F = 61 - e, 2^e > max_j sum_i w_i |z_ij|, and G = 61 - e(W) (G = 0 without weights); the inertia is the integer
 *   sum of llrint(w_i D_i 2^FI), FI from the bound sum w D <= 2 sum w |z|^2 + 2 W |c_0|^2.  Equal inputs give equal bits; a
 *   restart's bits do not depend on the restarts that share the call, and with init_host not on the layout.  A centre coordinate
 *   is within n_c 2^-(F + 1) / W_c of the exact weighted mean of its rows: 2^-(F + 1) <= 2^-39 at S = 2^23 without weights.
 *   Outputs in host memory (NULL: skipped); the call synchronises.
 *     centers [R, k, d]   in the chain's own units (c scale + mean)       inertia [R], n_iter [R], converged [R] (0 / 1)
 *     size [R, k]         rows of positive weight per cluster             wsum [R, k]  their weight
 *     mean [d], scale [d] what z was formed with                          seed_index [R, k]  the seeded rows (-1 with init_host)
 *     best                the best restart                                n_skipped    rows with a non-finite coordinate
 *     labels_dev [S]      (int32, DEVICE memory, optional) the best restart's labels in row order, -1 for a skipped row
 *   Errors (GPB_E_ARG): nsteps, nwalkers or d below 1; d above 64; nsteps nwalkers above 2^31 - 1; strides that let two elements
 *   alias; weights with nwalkers != 1, or negative or not finite; k outside 1 .. 32; R outside 1 .. 16; max_iter < 1; tol negative
 *   or not finite; standardize not 0 / 1; both or neither of init_host and u_host; init_host not finite; u_host outside [0, 1); k
 *   above the number of rows with positive weight. */
GPB_API int gpb_chain_kmeans(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d,
                     int64_t step_stride, int64_t walker_stride, const double* w_dev /*[nsteps] or NULL*/, int k, int R,
                     int max_iter, double tol, int standardize, const double* init_host /*[R,k,d] or NULL*/,
                     const double* u_host /*[R,k] or NULL*/, double* centers /*[R,k,d]*/, double* inertia /*[R]*/,
                     int32_t* n_iter /*[R]*/, int32_t* converged /*[R]*/, int64_t* size /*[R,k]*/, double* wsum /*[R,k]*/,
                     double* mean /*[d]*/, double* scale /*[d]*/, int64_t* seed_index /*[R,k]*/, int32_t* best,
                     int64_t* n_skipped, int32_t* labels_dev /*[S], device, or NULL*/);

/* ---- nearest-neighbour distances of resident chains -------------------------------------------------------------------------- *
 * gpb_chain_knn <- examples/PlotMCMC.ipynb overlays posterior and prior, and two or three posteriors (plot_corner_compare_datasets,
 *                  plot_compare_posteriors_3datasets), and leaves the comparison to the eye.  The numbers for it — the
 *                  Kozachenko-Leonenko entropy, the Wang-Kulkarni-Verdu divergence (gpbayestools_hic_amd/divergence.py) — need,
 *                  for every row of a set A, the distances to its nearest rows in A itself or in another set B: nA nB d coordinate
 *                  pairs of fp64 arithmetic, brute force, for chains that already lie in device memory.
 *   The context gives the device, the stream and the buffer cache only; no GP state is touched.  a_dev and b_dev with their sizes
 *   and strides exactly as gpb_chain_marginals and gpb_chain_kmeans read a chain (the same aliasing rule; a flat [S, d] set is
 *   nsteps = S, nwalkers = 1); the rows are numbered outer axis first, as in gpb_chain_kmeans.  b_dev == NULL: SELF mode, the
 *   neighbours of every row of A are sought in A, the row itself excluded by its number (the b_ sizes are ignored).  Otherwise
 *   CROSS mode: the candidates of every row of A are all rows of B.
 *   THE RULE, which a numpy model reproduces bit for bit (tests/knn_reference.py):
 *     z = x * inv_scale[j]                                       every coordinate of A and of B, one rounding
 *     acc = 0;  for j = 0 .. d - 1:  t = za_j - zb_j;  acc = acc + t * t        in that order, no fused multiply-add
 *   A row with a scaled coordinate that is not finite is skipped: as a query it gets r2 = +inf, idx = -1, zeros = 0, and it is
 *   never a candidate; n_skipped[0] counts such rows of A, n_skipped[1] those of B (0 in self mode).  A candidate at distance
 *   exactly 0 — a repeated row, which every MCMC chain has after a rejected move — is counted in zeros[i]; with skip_zero = 1 it
 *   is not listed, with skip_zero = 0 it is listed like any other.
 *   r2[i] holds the kmax smallest squared distances in ascending order, idx[i] their row numbers; equal distances are ordered by
 *   ascending row number; with fewer than kmax candidates the tail is +inf / -1.  The difference form is deliberate: the
 *   neighbours are the pairs where |a|^2 + |b|^2 - 2 a.b cancels worst.
 *   No output depends on splits (the number of ranges B is cut into so that a small A still fills the device; 0: chosen from the
 *   sizes), on the memory layout, on on_device, on which optional outputs are requested or on the slabs A goes through: the lists
 *   of the ranges are merged in (distance, row number) order.  Workspace, from the context's buffer cache: the scaled copy of B
 *   (of A in self mode), written once per call, and per slab of A its scaled rows, the ranges' partial lists and the staged
 *   results; the slabs keep what grows with them under GPB_KNN_WS_MB megabytes.
 *   Outputs in host memory when on_device = 0 or device memory when 1; n_skipped always in host memory; the call synchronises.
 *   Errors (GPB_E_ARG): sizes below 1; more than 2^31 - 1 rows; d outside 1 .. 64; kmax outside 1 .. 16; inv_scale_host not finite
 *   and positive; strides that let two elements alias; splits < 0; skip_zero or on_device not 0 / 1; r2 or n_skipped NULL. */
#define GPB_KNN_WS_MB 256
GPB_API int gpb_chain_knn(gpb_ctx* ctx, const double* a_dev, int64_t a_nsteps, int64_t a_nwalkers, int64_t a_step_stride,
                  int64_t a_walker_stride, const double* b_dev /*NULL: the neighbours are sought in A itself*/, int64_t b_nsteps,
                  int64_t b_nwalkers, int64_t b_step_stride, int64_t b_walker_stride, int64_t d,
                  const double* inv_scale_host /*[d]*/, int kmax, int skip_zero, int splits /*0: automatic*/, int on_device,
                  double* r2 /*[nA,kmax]*/, int32_t* idx /*[nA,kmax] or NULL*/, int32_t* zeros /*[nA] or NULL*/,
                  int64_t* n_skipped /*host, [2]*/);

/* ---- kernel Stein discrepancy and Stein thinning of a resident point set ------------------------------------------------------- *
 * gpb_stein_thin, gpb_stein_ksd <- nothing in the reference project: examples/generate_posterior_clusters.py picks the parameter
 *                  sets for further full-model runs by k-means, and no diagnostic says how well a point set represents the
 *                  posterior.  The kernel Stein discrepancy (Gorham & Mackey 2017) needs only the points and the score
 *                  grad log p at them (gpb_chain_logpost_grad); Stein thinning (Riabiz et al. 2022) picks, greedily, the m rows
 *                  whose empirical measure has the smallest discrepancy (gpbayestools_hic_amd/thinning.py).
 *   The context gives the device, the stream and the buffer cache only; no GP state is touched.  x_dev, g_dev: rows x_i and scores
 *   g_i, i < n, row i at [i row_stride], d contiguous doubles (device memory).  ginv_host [d][d]: a symmetric positive definite
 *   Gamma^-1 (host memory; the library checks that it is finite with a positive diagonal, the CALLER that it is SPD).
 *   THE RULE, which a numpy model reproduces bit for bit (tests/stein_reference.py).  The base kernel is the inverse multiquadric
 *   k(x, y) = (1 + (x - y)^T Gamma^-1 (x - y))^(-1/2); kp is the Stein kernel of the Langevin operator, one operation per rounding,
 *   no fused multiply-add, IEEE sqrt and division:
 *     b_i = Gamma^-1 x_i          once per row: acc = 0; acc = acc + Ginv[j][l] * x[l], l ascending
 *     tr  = sum_j Ginv[j][j]      from 0, j ascending, on the host
 *     q = 1; t1 = t3 = t4 = 0
 *     for l = 0 .. d - 1:  r = x_il - x_jl;  h = b_il - b_jl
 *                          q = q + r * h;  t1 = t1 + h * h;  t3 = t3 + (g_il - g_jl) * h;  t4 = t4 + g_il * g_jl
 *     s = sqrt(q); i1 = 1 / s; i2 = 1 / q; i3 = i1 * i2; i5 = i3 * i2
 *     kp(i, j) = (-3 * t1) * i5 + (tr + t3) * i3 + t4 * i1                        evaluated left to right
 *   A row with a non-finite entry in x, g or b is SKIPPED: never picked, left out of every sum (it adds +0), counted in
 *   n_skipped; its obj and its row_sum are NaN.
 *   gpb_stein_thin: obj_i = kp(i, i); S = 0; for t = 1 .. m: pi_t = the row of smallest obj among the rows that are not skipped
 *     and whose obj is not NaN, the LOWEST row number on a tie; S = S + obj[pi_t]; ksd[t - 1] = sqrt(S) / t; idx[t - 1] = pi_t;
 *     obj_i = obj_i + 2 * kp(i, pi_t) for every i.  Rows may repeat and m may exceed n.  ksd[t - 1] is the discrepancy of the
 *     first t picks.  With no row to pick, idx = -1 and ksd = NaN from there on and obj is left as it is.  obj (optional)
 *     receives the objective after the last update.  All m iterations are enqueued in one call; the host waits once, at the end.
 *   gpb_stein_ksd: row_sum_i = sum_j kp(i, j) over all j, j = i included, in THIS order: the columns are cut into chunks of
 *     GPB_STEIN_CHUNK; a chunk's partial starts at 0 and takes its columns in ascending j; the row sum starts at 0 and takes the
 *     chunk partials in ascending order.  ksd2 = (sum_i row_sum_i) / (nv * nv), nv = (double)(n - n_skipped): the rows are cut
 *     into chunks of 256 (a skipped row and the rows behind n count as +0); a chunk's 256 values v are summed as four groups of 64,
 *     each by the butterfly v[l] = v[l] + v[l ^ o], o = 32, 16, .. 1, then (w0 + w1) + (w2 + w3); the total starts at 0 and takes
 *     the chunk sums in ascending order.  No output depends on splits (the number of ranges the columns are cut into so that a
 *     small set still fills the device; 0: chosen from the sizes), on on_device, on the strides or on the slabs of query rows
 *     the call goes through (their chunk partials are kept under GPB_STEIN_PART_MB megabytes).
 *   Outputs in host memory when on_device = 0 or device memory when 1; n_skipped always in host memory; the calls synchronise.
 *   Errors (GPB_E_ARG; nothing is written): a NULL x_dev, g_dev, ginv_host, idx, ksd, ksd2 or n_skipped; n outside 1 .. 2^31 - 1;
 *   d outside 1 .. 64; m outside 1 .. 2^20; a row stride below d; ginv_host not finite or with a diagonal entry <= 0; splits outside
 *   0 .. 64; on_device not 0 / 1. */
#define GPB_STEIN_CHUNK 1024
#define GPB_STEIN_PART_MB 16
GPB_API int gpb_stein_thin(gpb_ctx* ctx, const double* x_dev, const double* g_dev, int64_t n, int64_t d, int64_t x_row_stride,
                  int64_t g_row_stride, const double* ginv_host /*[d,d]*/, int64_t m, int on_device, int32_t* idx /*[m]*/,
                  double* ksd /*[m]*/, double* obj /*[n] or NULL*/, int64_t* n_skipped /*host*/);
GPB_API int gpb_stein_ksd(gpb_ctx* ctx, const double* x_dev, const double* g_dev, int64_t n, int64_t d, int64_t x_row_stride,
                  int64_t g_row_stride, const double* ginv_host /*[d,d]*/, int splits /*0: automatic*/, int on_device,
                  double* row_sum /*[n] or NULL*/, double* ksd2, int64_t* n_skipped /*host*/);

/* ---- expected information gain of planned measurements ------------------------------------------------------------------------ *
 * gpb_eig_simulate, gpb_eig_lse <- nothing in the reference project: it reports what the data taught (the posterior) and never asks
 *                  what a planned measurement is expected to teach.  The nested Monte Carlo estimator of the mutual information
 *                  between parameters and data (gpbayestools_hic_amd/eig.py) needs the diagonal Gaussian log-likelihood of every
 *                  simulated data vector under every sample: S_out S_in M terms and a log-sum-exp per row and group of observables.
 *   The context gives the device, the stream and the buffer cache only; no GP state is touched.  All arrays are OBSERVABLE-MAJOR,
 *   as gpb_emu_predict_diag writes them: mu_T, var_T [M][ld_in] (sample j of observable m at [m ld_in + j]), y_T, z_T [M][ld_out].
 *   INNER SET: samples j < S_in with means mu_jm, variances s_jm = var_jm + vadd_m (var_T == NULL: 0; vadd_dev == NULL: 0; every s
 *   must be finite and > 0 and every input finite — the CALLER checks that, the library does not) and log-weights logw_j (NULL: 0).
 *   OUTER SET: positions i < S_out, each with an index o_i = outer_idx_dev[i] (int32, device) into the inner set.  THE LIBRARY checks
 *   the indices, on the device, before any kernel reads through one: an index outside [0, S_in) is GPB_E_ARG.
 *   gpb_eig_simulate: y_im = mu_{o_i,m} + sqrt(s_{o_i,m}) z_im, no fused multiply-add, z from normal_pair (csrc/philox.h) of the
 *   counter (i, p, 0, tag 15) for the observables 2p and 2p + 1: the key is the POSITION i, so repeated indices get different
 *   noise.  z_T (optional) receives the draws.  Columns >= S_out of y_T and z_T are not touched.
 *   gpb_eig_lse: for the groups g < G of observables [ranges_host[2g], ranges_host[2g + 1]) (host, int32) and
 *     l_ij(g) = logw_j - sum_{m in g} [ (y_im - mu_jm)^2 / s_jm + ln s_jm ] / 2           (the (M_g / 2) ln 2 pi term is left out)
 *     lse_excl[g, i] = ln sum_{j != o_i} exp l_ij(g)          (-inf when S_in == 1)
 *     self[g, i]     = l_{i, o_i}(g), summed term by term in the order of m
 *   lse_excl is evaluated as a matrix product on the fp64 matrix pipe: with c_m = mean_j mu_jm, t = 1 / s, u = (mu - c) t,
 *   q = -(y - c)^2 / 2, l = y - c and b_gj = logw_j - sum_{m in g} [(mu_jm - c_m)^2 t_jm + ln s_jm] / 2,
 *     l_ij(g) = sum_{m in g} (q_im t_jm + l_im u_jm) + b_gj,
 *   followed by an online log-sum-exp (running maximum and sum of exponentials) over the inner samples; no S_out x S_in array exists.
 *   Its error is that of a dot product of 2 M_g terms: |lse_excl - exact| <= (2 M_g + 64) 2^-52 (max_j (sum_k |a_ik b_jk| + |b_gj|)
 *   + |lse_excl| + 1) (tests/test_gpu_eig.py).  The inner axis is cut into `splits` ranges (0: chosen from the sizes, 1 .. 64: at
 *   most that many) so that few outer rows still fill the device; the ranges are merged in range order, no floating-point
 *   atomics: the same call gives the same bits, another `splits` the same value within the rounding above.
 *   Workspace, from the context's buffer cache: the two operand panels, 16 M (S_in + S_out) bytes rounded up to whole tiles.
 *   Outputs lse_excl, self [G, S_out] in host memory when on_device = 0 or device memory when 1; both calls synchronise.
 *   Errors (GPB_E_ARG): M outside 1 .. 4096; S_in or S_out below 1 or above 2^31 - 65; ld_in < S_in or ld_out < S_out; an outer index
 *   outside [0, S_in); G outside 1 .. 64; a group that is empty or not inside [0, M); splits outside 0 .. 64; on_device not 0 / 1;
 *   a NULL mu_T, outer_idx_dev, y_T, ranges_host, lse_excl or self. */
GPB_API int gpb_eig_simulate(gpb_ctx* ctx, const double* mu_T, const double* var_T /*or NULL*/, const double* vadd_dev /*[M] or NULL*/,
                     int64_t M, int64_t S_in, int64_t ld_in, const int32_t* outer_idx_dev /*[S_out]*/, int64_t S_out, uint64_t seed,
                     double* y_T /*[M,ld_out]*/, double* z_T /*[M,ld_out] or NULL*/, int64_t ld_out);
GPB_API int gpb_eig_lse(gpb_ctx* ctx, const double* mu_T, const double* var_T /*or NULL*/, const double* vadd_dev /*[M] or NULL*/,
                const double* logw_dev /*[S_in] or NULL*/, int64_t M, int64_t S_in, int64_t ld_in, const double* y_T,
                const int32_t* outer_idx_dev /*[S_out]*/, int64_t S_out, int64_t ld_out, const int32_t* ranges_host /*[G,2]*/, int G,
                int splits /*0: automatic*/, int on_device, double* lse_excl /*[G,S_out]*/, double* self /*[G,S_out]*/);

/* ---- history matching: implausibility, NROY space, maps ----------------------------------------------------------------------- *
 * gpb_hm_uniform, gpb_hm_implausibility, gpb_hm_maps <- nothing in the reference project: its `predict` returns [S, nobs, nobs]
 *                  arrays and nothing asks how much of the prior box the data already rule out (Craig et al. 1997; Vernon, Goldstein &
 *                  Bower 2010; gpbayestools_hic_amd/history.py).
 *   The context gives the device, the stream and the buffer cache only; no GP state is touched.  Every array but lo_host, hi_host,
 *   ranges_host, edges_host and pairs_host is DEVICE memory; the calls enqueue on the context's stream and do not synchronise.
 *   gpb_hm_uniform: candidate rows r < S of X_dev [S][ld], x[r][j] = lo_j + (hi_j - lo_j) u, two roundings after the subtraction (no
 *   fused multiply-add), u = u01(p.x, p.y) of p = philox(seed, (uint32) R, (uint32) (R >> 32), j, 16) (csrc/philox.h) with R = row0 + r
 *   the ABSOLUTE row: a row's bits do not depend on how a call is cut into slabs.  Columns >= d are not touched.
 *   Errors (GPB_E_ARG): d outside 1 .. 512; S < 1 or above 2^31 - 1; bounds that are not finite or hi_j <= lo_j; ld < d.
 *   gpb_hm_implausibility: mu_T, var_T [M][ld] OBSERVABLE-MAJOR as gpb_emu_predict_diag writes them.  Per sample s < S and observable m:
 *     r = |yexp_m - mu_T[m][s]|,  v = var_T[m][s] + vadd_m  (var_T == NULL: 0; vadd_dev == NULL: 0)
 *     I_m = r / sqrt(v) when v > 0 and r is not NaN (inf / inf, a non-finite mean under vadd_m = +inf, counts as 0); otherwise,
 *     a NaN v included, I_m = 0 if r == 0, else +inf — and the sample is BAD.  *bad_dev (int64, device) is ADDED the number of bad
 *     samples, each once.  vadd_m = +inf gives I_m = 0 exactly: the way to mask an observable.  No output is ever NaN.
 *     top_T[k][s], k < K: the (k + 1)-th largest I_m over all observables; arg[s] (int32, or NULL): the observable of the largest,
 *     the lowest index on ties; gmax_T[g][s] (or NULL), g < G: the largest I_m over [ranges_host[2g], ranges_host[2g + 1]).  top_T and
 *     gmax_T have the leading dimension ldo; columns >= S are not touched.  One lane per sample, the K largest kept in registers; a
 *     sample's outputs depend on its own column alone (no floating-point atomics).
 *   Errors (GPB_E_ARG): M outside 1 .. 4096; K outside 1 .. min(4, M); G outside 0 .. 64; a range that is empty or not inside [0, M);
 *     ld or ldo below S; S < 1 or above 2^31 - 1; a NULL mu_T, yexp_dev, top_T or bad_dev.
 *   gpb_hm_maps: rows x_dev [S][row_stride] with a score per row.  Over the bin edges edges_host [d][B + 1] — gpb_chain_marginals' BIN
 *     RULE: bin b iff e[b] <= x < e[b + 1], the last bin closed, NaN and the rest outside — for every bin of every parameter
 *     (min1, cnt1, nroy1 [d][B]) and every bin pair of every pair of parameters (min2, cnt2, nroy2 [npairs][B][B]; pairs_host
 *     [npairs][2], NULL = all i < j in lexicographic order) that a row falls into: cnt += 1; nroy += 1 if score < cutoff (strict);
 *     min = min(min, score).  init = 1 first sets the minima to +inf and the counts to 0 (an empty bin reads +inf, 0, 0), init = 0
 *     accumulates onto what the arrays hold: slabs add up.  Either triple may be NULL (as a whole).  The minimum is an integer minimum
 *     of order-preserving 64-bit keys (csrc/order_key.h), the counts are integer adds: the result does not depend on arrival order or
 *     on the slabs.  Scores must not be NaN; +inf counts and never lowers a minimum.  While the call is in flight min1 / min2 hold keys.
 *   Errors (GPB_E_ARG): B outside 1 .. 64; row_stride < d; edges not finite or not strictly increasing; a pair index outside [0, d)
 *     or a pair (i, i); without a pair list npairs != d (d - 1) / 2; npairs B^2 above 2^31 - 1; S < 1 or above 2^31 - 1; a cutoff
 *     that is not finite; init not 0 / 1; a triple of which only a part is given. */
GPB_API int gpb_hm_uniform(gpb_ctx* ctx, const double* lo_host /*[d]*/, const double* hi_host /*[d]*/, int64_t d, uint64_t row0, int64_t S,
                   uint64_t seed, double* X_dev /*[S,ld]*/, int64_t ld);
GPB_API int gpb_hm_implausibility(gpb_ctx* ctx, const double* mu_T, const double* var_T /*or NULL*/, int64_t M, int64_t S, int64_t ld,
                          const double* yexp_dev /*[M]*/, const double* vadd_dev /*[M] or NULL*/, const int32_t* ranges_host /*[G,2] or NULL*/,
                          int G, int K, double* top_T /*[K,ldo]*/, int32_t* arg /*[S] or NULL*/, double* gmax_T /*[G,ldo] or NULL*/,
                          int64_t ldo, int64_t* bad_dev /*[1], added to*/);
GPB_API int gpb_hm_maps(gpb_ctx* ctx, const double* x_dev /*[S,row_stride]*/, int64_t S, int64_t d, int64_t row_stride,
                const double* score_dev /*[S]*/, double cutoff, const double* edges_host /*[d,B+1]*/, int B,
                const int32_t* pairs_host /*[npairs,2] or NULL*/, int64_t npairs, int init, double* min1 /*[d,B]*/, int64_t* cnt1,
                int64_t* nroy1, double* min2 /*[npairs,B,B]*/, int64_t* cnt2, int64_t* nroy2);

/* ---- maximum-projection Latin-hypercube designs -------------------------------------------------------------------------------- *
 * gpb_maxpro_lhd, gpb_maxpro_run_order <- src/design.py:64-74, R's `MaxProRunOrder(MaxProLHD(npoints, ndim)$Design)`;
 * gpb_maxpro_criterion: the criterion that generator minimises, for any design.
 *   The context gives the device, the stream and the buffer cache only; no GP state is touched.  2 <= d <= 64, 4 <= n <= 4096.
 *   Levels l[i][c] in {0 .. n-1}, every column a permutation; the design is x = (l + 0.5) / n.  Pair terms
 *   t_ij = prod_c (s (l_ic - l_jc))^-2 with s = e^1.5 / n, the objective f = ln sum_{i<j} t_ij, and the criterion of Joseph, Gul, Ba
 *   (2015), psi = (mean_{i<j} prod_c (x_ic - x_jc)^-2)^(1/d):  ln psi = (f + 3 d - ln(n (n - 1) / 2)) / d  (csrc/maxpro_index.h).
 *   gpb_maxpro_lhd: simulated annealing over column-wise swaps, R <= 16 independent restarts from init_levels [R, n, d].  Stage k
 *   of n_stages has the temperature temp0 cool^k and runs blocks_per_stage blocks; a block is `block` (1 .. 64) proposals, all
 *   drawn and evaluated at the block's starting state; in slot order the first that passes ln u < -(f' - f) / temp is applied,
 *   the rest of the block is discarded.  A proposal (column, rows a != b, u) is decoded from Philox4x32-10 with the counter
 *   (global block index, restart0 + r, slot, 11): a restart's result depends on its start and its index alone.  The pair matrix
 *   and f are rebuilt from the levels at every stage start.  Per restart: levels_out [R, n, d] the best levels seen, f_start,
 *   f_best (recomputed from those levels), accepted and consumed proposals, and trace [R, n_stages blocks_per_stage] (or NULL):
 *   per block the accepted slot, or -1.  Host memory; the call synchronises once before the annealing and once behind it.
 *   Errors (GPB_E_ARG): n, d, R, block outside their limits; a column that is no permutation; a start whose f is not finite (two
 *   rows adjacent in every column of a wide design); temperatures that are not positive and finite; more than 2^31 - 1 blocks.
 *   gpb_maxpro_criterion: ln psi of a real design X [n, d] (host), +inf when two rows share a coordinate; sum_out (or NULL) the sum
 *   of the pair terms prod_c (e^1.5 (x_ic - x_jc))^-2.
 *   gpb_maxpro_run_order: order_out [n] (int32): row `first` (-1: the row nearest the cube's centre), then again and again the
 *   row with the smallest sum of its pair terms with the rows chosen so far; the lowest index wins a tie. */
GPB_API int gpb_maxpro_lhd(gpb_ctx* ctx, int64_t n, int64_t d, int R, int restart0, const int32_t* init_levels /*[R,n,d]*/,
                   uint64_t seed, int64_t n_stages, int64_t blocks_per_stage, int block, double temp0, double cool,
                   int32_t* levels_out /*[R,n,d]*/, double* f_start /*[R]*/, double* f_best /*[R]*/, int64_t* accepted /*[R]*/,
                   int64_t* consumed /*[R]*/, int32_t* trace /*[R, n_stages blocks_per_stage] or NULL*/);
GPB_API int gpb_maxpro_criterion(gpb_ctx* ctx, const double* X /*[n,d]*/, int64_t n, int64_t d, double* lnpsi_out,
                         double* sum_out /*or NULL*/);
GPB_API int gpb_maxpro_run_order(gpb_ctx* ctx, const double* X /*[n,d]*/, int64_t n, int64_t d, int64_t first,
                         int32_t* order_out /*[n]*/);

/* ---- likelihood block: replaces Chain._predict + mvn_loglike for ONE emulator ---- *
 * gpb_like_set   <- expdata[i0:i0+M], expdata_cov[i0:i0+M, i0:i0+M]    src/mcmc.py:139,302-324
 * gpb_loglike    <- -1/2 dY^T C^-1 dY - sum log diag chol(C), C = cov_model + cov_exp
 *                   for this emulator's diagonal block                 src/mcmc.py:23-65,153-166,288-293
 * The reference's covariance is block-diagonal over emulators (src/mcmc.py:163-164) and
 * the experimental covariance is diagonal (src/mcmc.py:320-322), so the multivariate
 * normal factorises: log-likelihood = sum over emulators of gpb_loglike blocks.
 * Rows whose block is not positive definite get NaN (the reference yields garbage there,
 * src/mcmc.py:44-54); *n_notpd_host counts them.
 */
GPB_API int gpb_like_set(gpb_ctx* ctx, const double* yexp_host /*[M]*/, const double* cov_exp_host /*[M,M]*/);
GPB_API int gpb_loglike(gpb_ctx* ctx, const double* Xs, int64_t W, int on_device,
                double* ll /*[W], same memory space as Xs*/, int accumulate,
                int* n_notpd_host /*may be NULL; forces a sync when non-NULL*/);

/* gpb_logpost <- Chain.log_posterior / log_likelihood for the LAST (or only) emulator of a chain, all on the
 *                device and asynchronous: block log-likelihood (added onto ll when accumulate != 0), then
 *                inside = all(lo < x < hi) strictly; ll = inside ? ll + inside_const : outside_value
 *                                                                       src/mcmc.py:188-222, 261-299 */
GPB_API int gpb_logpost(gpb_ctx* ctx, const double* Xs_dev /*[W,d]*/, int64_t W, double* ll_dev /*[W]*/, int accumulate,
                const double* lo_dev /*[d]*/, const double* hi_dev /*[d]*/, double outside_value,
                double inside_const);

/* gpb_mvn_loglike <- map(mvn_loglike, dY, cov): generic batched form on caller-provided
 *                    dY[W,M], cov[W,M,M] (any covariance, e.g. from foreign emulators)   src/mcmc.py:23-65,293 */
GPB_API int gpb_mvn_loglike(gpb_ctx* ctx, const double* dY, const double* cov, int64_t W, int64_t M, int on_device,
                    double* ll /*[W]*/, int* n_notpd_host /*may be NULL*/);

/* ---- chain-level helpers (device, for resident sampling loops) ------------------- *
 * gpb_box_finish <- inside=all(min<X<max) (strict); lp[~inside]=-inf|-1e300;
 *                   lp[inside] = ll + const                             src/mcmc.py:194-198,220-221,275-276,296-297
 */
GPB_API int gpb_box_finish(gpb_ctx* ctx, const double* X_dev /*[W,d]*/, int64_t W, int64_t d,
                   const double* lo_dev, const double* hi_dev, double outside_value,
                   double inside_const, double* ll_inout_dev /*[W]*/);

/* ---- parameterTrafoPCA input map (device pre-pass) -------------------------------- *
 * gpb_param_map_set <- the fitted scalers / PCAs of the three parameter groups          src/emulator.py:79-241
 * gpb_param_map     <- the per-row mapping X[W,d_in] -> GP input [W,d_out] that
 *                      Emulator.predict performs with Python loops before the GP calls  src/emulator.py:492-551
 * col_src[j] >= 0: output column j is original column col_src[j]; col_src[j] = -1 - (g*maxpc + c): principal
 * component c of group g.  group_desc[g] = {fn, col0, col1, col2, col3 (-1 = unused), npc}, fn 0 = zeta/s(T)
 * (:102-108), 1 = eta/s(mu_B) (:111-117), 2 = y_loss(y_init) (:120-126).  tables[g] = grid[100] | scaler mean[100]
 * | scaler scale[100] | PCA mean[100] | components[maxpc][100]. */
GPB_API int gpb_param_map_set(gpb_ctx* ctx, int64_t d_in, int64_t d_out, const int32_t* col_src /*[d_out]*/,
                      int32_t n_groups, const int32_t* group_desc /*[G][6]*/,
                      const double* tables /*[G][4+maxpc][100]*/, int32_t maxpc);
GPB_API int gpb_param_map(gpb_ctx* ctx, const double* X_dev /*[W,d_in]*/, int64_t W, double* out_dev /*[W,d_out]*/);

/* ---- emcee-equivalent stretch move (device resident) ------------------------------ *
 * Replaces emcee.EnsembleSampler.sample as driven by LoggingEnsembleSampler.run_mcmc
 * (src/mcmc.py:68-92,372-412): red/blue stretch move, a=2, counter-based Philox RNG
 * replicated on every rank.
 * gpb_stretch_propose: for the walkers of half `half` draw the complementary walker and z, write
 *   proposals q[nhalf,d] and the (d-1) ln z factor[nhalf].  Walker k of the half is index pi(2k+half):
 *   pi = identity when randomize_split = 0 (emcee inds = arange(n) % 2), else a per-step keyed
 *   pseudo-random permutation (emcee's default randomize_split=True), evaluated inline on every rank.
 * gpb_stretch_accept: accept where (d-1)*ln z + lp' - lp > ln u; updates pos, lp, naccept.
 */
GPB_API int gpb_stretch_propose(gpb_ctx* ctx, const double* pos_dev /*[nw,d]*/, int64_t nwalkers, int64_t d,
                        int half, uint64_t seed, uint64_t step, double a,
                        double* q_dev /*[nw/2,d]*/, double* factor_dev /*[nw/2]*/, int randomize_split);
GPB_API int gpb_stretch_accept(gpb_ctx* ctx, double* pos_dev, double* lp_dev /*[nw]*/, int64_t nwalkers, int64_t d,
                       int half, uint64_t seed, uint64_t step,
                       const double* q_dev, const double* factor_dev, const double* lpq_dev /*[nw/2]*/,
                       int64_t* naccept_dev /*[nw]*/, int randomize_split);
/* NaN log-probabilities the accept step has seen since the last reset (emcee raises "Probability function returned
 * NaN" when one occurs, emcee/ensemble.py; on the device such a proposal is rejected and counted).  Synchronises. */
GPB_API int gpb_stretch_nan_count(gpb_ctx* ctx, int64_t* count_host, int reset);

/* gpb_emcee_run <- the loop emcee.EnsembleSampler.sample runs under LoggingEnsembleSampler.run_mcmc
 *                  (src/mcmc.py:68-92, 372-412) with Chain.log_posterior (src/mcmc.py:261-299) as the log-probability,
 * for a chain whose observables come from THIS context's emulator alone: nsteps stretch-move steps (two half-ensemble
 * updates each: propose -> GP predict -> block log-likelihood + prior box -> accept), enqueued back to back on the
 * context's stream with no host involvement per step.  pos/lp hold the ensemble and its log-probabilities on entry
 * and on exit; chain_dev [nsteps, nw, d] / lpchain_dev [nsteps, nw] (either may be NULL) receive the state after every
 * step; steps are numbered step0, step0 + 1, ... in the counter-based generator.  With a communicator installed
 * (gpb_dist_init) every rank evaluates its rows of each half-ensemble batch and one in-stream all-gather per batch
 * completes the vector; nwalkers / 2 must then divide evenly over the ranks.  Asynchronous. */
GPB_API int gpb_emcee_run(gpb_ctx* ctx, double* pos_dev /*[nw,d]*/, double* lp_dev /*[nw]*/, int64_t nwalkers, int64_t nsteps,
                  uint64_t seed, uint64_t step0, double a, int randomize_split,
                  const double* lo_dev /*[d]*/, const double* hi_dev /*[d]*/, double outside_value, double inside_const,
                  double* chain_dev, double* lpchain_dev, int64_t* naccept_dev /*[nw]*/);

/* Chains of several emulators (Chain.emuList, src/mcmc.py:139-166): the covariance is block-diagonal over the emulators,
 * the log-likelihood the sum of their blocks.  ctxs[0..E) are the emulators' contexts in emuList order, all on one device
 * and stream, each with its likelihood block installed (gpb_like_set) and, for parameterTrafoPCA emulators, its
 * parameter map (gpb_param_map_set); rows are in the chain's ORIGINAL parameters [W, ndim].
 * gpb_chain_logpost   <- Chain.log_posterior / log_likelihood for the whole chain, rows inside the box only.
 * gpb_chain_emcee_run <- gpb_emcee_run for such a chain (a communicator, if any, is taken from ctxs[0]).
 * Both need the block likelihood kernels for every emulator (PCA modes with M <= 64 or npc <= 16); GPB_E_STATE
 * otherwise (the caller then sequences gpb_loglike / gpb_box_finish itself).
 * gpb_chain_supported: 1 when the two calls would accept these contexts as they stand, 0 when not, < 0 on bad arguments. */
GPB_API int gpb_chain_supported(gpb_ctx* const* ctxs, int E);
GPB_API int gpb_chain_logpost(gpb_ctx* const* ctxs, int E, const double* Xs_dev /*[W,ndim]*/, int64_t W, double* ll_dev /*[W]*/,
                      const double* lo_dev, const double* hi_dev, double outside_value, double inside_const);
GPB_API int gpb_chain_emcee_run(gpb_ctx* const* ctxs, int E, double* pos_dev, double* lp_dev, int64_t nwalkers, int64_t nsteps,
                        uint64_t seed, uint64_t step0, double a, int randomize_split,
                        const double* lo_dev, const double* hi_dev, double outside_value, double inside_const,
                        double* chain_dev, double* lpchain_dev, int64_t* naccept_dev);
/* gpb_chain_like_set <- the experiment of a whole chain: expdata[0, :], expdata_cov[:, :] over the MT = sum M_e observables
 *   of ctxs[0..E) in emuList order, where expdata_cov may couple the emulators (a shared normalisation uncertainty, errors
 *   correlated across emulators): the reference adds whatever expdata_cov holds and factorises the full matrix per row
 *   (src/mcmc.py:288-293).  Every emulator's own diagonal block is installed through gpb_like_set, so all that reads a
 *   block per emulator keeps working.  When cov_exp_host has a non-zero entry outside the blocks, the joint tables of the
 *   coupled likelihood are built in ctxs[0] (host, O(MT^3) once): the covariance of a row is C0 + A^T diag(g) A with
 *   C0 = blockdiag(C_trunc,e) + C_exp and A = blockdiag(A_e), so a row costs one PT x PT Cholesky, PT = sum P_e GPs.
 *   *applies_host = 1: the coupling is installed and gpb_chain_logpost, gpb_chain_emcee_run, gpb_chain_smc_reweight /
 *   gpb_chain_smc_move, gpb_chain_ptlmc_run and gpb_chain_logpost_grad evaluate the coupled likelihood for exactly this
 *   list of contexts (rows whose S is not positive definite: NaN, counted with ctxs[0]).  That needs every emulator in
 *   PCA mode, PT <= 128, MT <= 2048, gpb_chain_supported == 1, C0 positive definite and A of full rank.
 *   *applies_host = 0 (return value still 0): the matrix is block-diagonal (the chain's block path, as before), or one of
 *   those conditions fails — then nothing is installed and the caller evaluates the dense matrix itself
 *   (gpb_emu_predict + gpb_mvn_loglike).  cov_exp_host = NULL clears a coupling and leaves the blocks.
 *   A later gpb_like_set, gpb_emu_set_transform or gpb_gp_set on any member makes the coupling stale: the chain calls then
 *   fail with GPB_E_STATE until gpb_chain_like_set is called again; they never evaluate the block-diagonal likelihood in
 *   its place.  The member contexts must outlive the coupling.  GPB_E_ARG: a null pointer or context, E outside 1 .. 64,
 *   contexts on different devices or streams.  Synchronises. */
GPB_API int gpb_chain_like_set(gpb_ctx* const* ctxs, int E, const double* yexp_host /*[MT]*/,
                       const double* cov_exp_host /*[MT,MT], or NULL: clear the coupling*/, int* applies_host);
/* Many data vectors against ONE experimental covariance in one resident run (Chain.run_closure: the closure study of
 *   examples/ClosureTest.ipynb over a whole validation set).  The data enter the low-rank block likelihood only through a
 *   P-vector v0 = Q^T L0^-1 (mu - yexp) and a scalar c_perp per emulator; the factorisation of C0 stays in the context.
 * gpb_chain_like_sets: after gpb_chain_like_set, whose covariance all sets share: per emulator the device tables
 *   v0[K][16] (zero padded beyond P) and cperp[K] of the rows of yexp_host [K][MT], MT = sum M_e in emuList order; O(M^2) host
 *   work per set and emulator, no second Cholesky.  Row k of the tables is, bit for bit, what a single-set installation of
 *   yexp_host[k] leaves.  K = 0 drops the tables, and so does any later gpb_like_set / gpb_chain_like_set /
 *   gpb_emu_set_transform / gpb_gp_set of a member.  GPB_E_ARG: K < 0 or K > 65536, a null pointer or context.  GPB_E_STATE:
 *   no likelihood installed, an emulator that does not take the low-rank likelihood kernel (PCA mode, at most 16 GPs, C0
 *   positive definite, A of full rank, option keys 11 / 23 / 43 at their defaults), more than 24 emulators, or a coupled
 *   chain likelihood installed.  A covariance PER set is not supported (a factorisation per set).  Synchronises.
 * gpb_chain_logpost_sets: gpb_chain_logpost for rows that belong to different data sets: row w is judged against set
 *   w / rows_per_set.  ll of a row of set k equals, bit for bit, gpb_chain_logpost of that row with data set k installed.
 *   GPB_E_ARG: W no multiple of rows_per_set, W >= 2^31, or W / rows_per_set beyond the tables' K.  GPB_E_STATE: no tables
 *   (or dropped), and what gpb_chain_logpost refuses.  Asynchronous, all pointers device memory.
 * gpb_chain_emcee_sets_run: gpb_chain_emcee_run over K independent ensembles of nwalkers walkers each, ensemble s calibrated
 *   against data set s: pos_dev [K][nwalkers][d], lp_dev [K][nwalkers] (the caller's initial values: gpb_chain_logpost_sets
 *   with rows_per_set = nwalkers), naccept_dev [K][nwalkers], chain_dev [nsteps][K][nwalkers][d] and lpchain_dev
 *   [nsteps][K][nwalkers] (either may be NULL).  The proposals of all ensembles form one batch of K nwalkers / 2 rows per
 *   half-step.  Ensemble s takes exactly the draws of a stand-alone gpb_chain_emcee_run with seed = seeds_host[s], partners
 *   from its own other half only: its walkers are that run's, bit for bit.  Unfused sequence (propose, evaluate, accept,
 *   store), not sharded.  GPB_E_ARG: K outside 1 .. 65535, nwalkers odd or outside 2 .. 2^30, K nwalkers > 2^30, K beyond
 *   the tables.  GPB_E_STATE: a communicator is installed, and what gpb_chain_logpost_sets refuses.  All checks and all
 *   workspace growth precede the first launch.  NaN proposals are rejected and counted (gpb_stretch_nan_count).
 *   Asynchronous. */
GPB_API int gpb_chain_like_sets(gpb_ctx* const* ctxs, int E, int64_t K, const double* yexp_host /*[K,MT]*/);
GPB_API int gpb_chain_logpost_sets(gpb_ctx* const* ctxs, int E, const double* Xs_dev /*[W,ndim]*/, int64_t W, int64_t rows_per_set,
                           double* ll_dev /*[W]*/, const double* lo_dev, const double* hi_dev, double outside_value,
                           double inside_const);
GPB_API int gpb_chain_emcee_sets_run(gpb_ctx* const* ctxs, int E, double* pos_dev, double* lp_dev, int64_t K, int64_t nwalkers,
                             int64_t nsteps, const uint64_t* seeds_host /*[K]*/, uint64_t step0, double a, int randomize_split,
                             const double* lo_dev, const double* hi_dev, double outside_value, double inside_const,
                             double* chain_dev, double* lpchain_dev, int64_t* naccept_dev);
/* gpb_chain_logpost_grad <- Chain.log_posterior / log_likelihood together with the gradient in the chain's parameters,
 *   the (lp, grad) tuple the reference's PTLMC sampler takes from its logpostfunc (src/mcmc.py:446-453, 499-528, 545-569).
 *   ll_dev receives bit for bit what gpb_chain_logpost writes (or, for contexts it does not accept, what the per-emulator
 *   sequence gpb_loglike ... gpb_logpost writes), under whichever predict arithmetic is selected; grad_dev [W, ndim] is fp64:
 *   per emulator the block's d lp / d (mean, variance) of every GP (all four transform modes), folded with the GP
 *   derivatives of gpb_gp_predict_grad and the parameter map's Jacobian.  Rows outside the box: outside_value and a zero
 *   gradient.  Rows whose block is not positive definite: NaN in both.  Asynchronous, all pointers device memory. */
GPB_API int gpb_chain_logpost_grad(gpb_ctx* const* ctxs, int E, const double* Xs_dev /*[W,ndim]*/, int64_t W, double* ll_dev /*[W]*/,
                           double* grad_dev /*[W,ndim]*/, const double* lo_dev, const double* hi_dev, double outside_value,
                           double inside_const);
/* gpb_chain_ptlmc_run <- Chain.samplerPTLMC's step loop (surmise's parallel-tempered Langevin sampler, src/mcmc.py:623-670,
 *   with tempexchange, src/mcmc.py:679-692) for the chain of ctxs (the contexts gpb_chain_logpost_grad accepts; for
 *   contexts gpb_chain_supported rejects, the per-emulator sequence gpb_loglike ... gpb_logpost evaluates the rows).
 *   nsteps steps numbered step0, step0 + 1, ... (global step k), enqueued back to back on the contexts' stream, no host
 *   synchronisation; one call of n steps gives the bits of n calls of one step.  T = numtemps + numchain rungs (2 .. 4096),
 *   temps_dev [T] the ladder, temps13_dev [T] its cube roots, hc_dev / covmat0_dev [d, d] the proposal factor and
 *   covariance (src/mcmc.py:604-615).  State, device memory in and out: theta [T, d], fval [T] (lp / temps), dfval [T, d]
 *   (grad / temps; NULL: the branch without a gradient), tune [2] = (tau, numtimes).  One step: N(0, 1) draws and the
 *   proposal, its lp (and gradient), the accept test log u < fvalp - fval + qadj per rung, five sweeps of T exchange picks
 *   in one lane, numtimes += accepted / T, at tuning steps (k < samptunning, k % 10 == 0) the tau update towards taracc,
 *   at production steps the numchain untempered rungs written to save_dev [numchain, nsave, d] at k - samptunning (when
 *   below nsave; save_dev may be NULL).  naccept_dev [T] (accepted proposals per rung) and nswap_dev [T - 1] (exchanges
 *   between rungs i and i + 1) are incremented; either may be NULL.  Philox4x32-10 keyed by seed, counters
 *   (rung, k, pair, 2) for the normals, (rung, k, 0, 3) for the accept draw, (pick, k, 0, 4) for the exchange.
 *   Asynchronous. */
GPB_API int gpb_chain_ptlmc_run(gpb_ctx* const* ctxs, int E, int64_t numtemps, int64_t numchain, int64_t nsteps, uint64_t step0,
                        uint64_t seed, int64_t samptunning, double taracc, double* theta_dev, double* fval_dev,
                        double* dfval_dev, double* tune_dev, const double* temps_dev, const double* temps13_dev,
                        const double* hc_dev, const double* covmat0_dev, const double* lo_dev, const double* hi_dev,
                        double outside_value, double inside_const, double* save_dev, int64_t nsave, int64_t* naccept_dev,
                        int64_t* nswap_dev);
/* gpb_chain_hmc_run <- Chain.run_HMC's step loop (hmc.HMCSampler): Hamiltonian Monte Carlo over C independent chains of the
 *   chain of ctxs (the contexts gpb_chain_logpost_grad accepts), a diagonal metric, L leapfrog steps per trajectory, the prior
 *   box as reflecting walls.  nsteps steps numbered step0, step0 + 1, ... (global step k, below 2^32), enqueued back to back on
 *   the contexts' stream, no host synchronisation, no graph capture; one call of n steps gives the bits of n calls of one
 *   step, and a chain's bits do not depend on C (with adapt = 0).  State, device memory in and out: x [C, d], lp [C] and grad
 *   [C, d] (gpb_chain_logpost_grad at x), state [10] 8-byte slots: the doubles ln eps, ln eps-bar, H-bar, mu and the update
 *   count of the dual averaging, then the 64-bit counts of accepted, divergent and escaped trajectories and of NaN rows, and
 *   one slot the loop keeps for itself (zero between calls).  minv_dev [d] the inverse masses, msqrt_dev [d] = 1 / sqrt(minv).
 *   One step of chain c: momenta p_j = z_j msqrt_j with z ~ N(0, 1) from Philox counters (c, k, pair, 12); H0 = -lp + K0,
 *   K = 1/2 sum_j (p_j p_j) minv_j in index order; the step size eps_k = exp(state[0]) (1 + jitter (2 u - 1)), u from (0, k, 0,
 *   13), the same for all chains; L times: p += (eps_k / 2) g, x_j += eps_k (minv_j p_j), then per coordinate at most 8
 *   reflections (x_j < lo_j: x_j = lo_j + (lo_j - x_j), p_j = -p_j; x_j > hi_j: x_j = hi_j - (x_j - hi_j), p_j = -p_j; still
 *   outside after that: the trajectory has escaped), one gpb_chain_logpost_grad at the C rows, p += (eps_k / 2) g'; the
 *   proposal is taken where ln u < -(H1 - H0), u from (c, k, 0, 14), and the trajectory has not escaped (NaN rejects; a row
 *   exactly on a wall evaluates to outside_value and rejects): x, lp and grad are replaced in place, lp bit for bit what
 *   gpb_chain_logpost gives at that row.  A trajectory is divergent where H1 - H0 > 1000 or is NaN.  adapt != 0: after each step
 *   one dual-averaging update (Hoffman & Gelman 2014, algorithm 5: gamma 0.05, t0 10, kappa 0.75) of the state towards
 *   target_accept with the mean over the chains of a_c = min(1, exp(-(H1 - H0))) (0 for NaN or escaped), summed as integers of
 *   2^-32: reproducible whatever the grid.  save_dev [nsave, C, d] and lpsave_dev [nsave, C] (either NULL) receive the state
 *   after step save0 + i thin at slot i < nsave; naccept_dev [C] (may be NULL) is incremented.
 *   diag (may be NULL; GPB_E_ARG unless nsteps == 1): device outputs of the step, each may be NULL.
 *   Errors (GPB_E_ARG): C outside 1 .. 1048576, d outside 1 .. 256, L outside 1 .. 1024, jitter outside [0, 1), with adapt a
 *   target_accept outside (0, 1), a step number of 2^32 or above, a null pointer, nsave or thin below 1 with save_dev; and what
 *   gpb_chain_logpost_grad refuses, before anything is enqueued.  Asynchronous. */
typedef struct gpb_hmc_diag {
    double* p0_dev;     /* [C, d] the initial momenta */
    double* logu_dev;   /* [C] ln u of the accept test */
    double* dh_dev;     /* [C] H1 - H0 */
    double* a_dev;      /* [C] the accept probabilities a_c */
    double* traj_dev;   /* [L, C, d] the positions after each drift (walls applied) */
    double* eps_dev;    /* [1] the step's step size eps_k */
} gpb_hmc_diag;
GPB_API int gpb_chain_hmc_run(gpb_ctx* const* ctxs, int E, int64_t C, int64_t nsteps, uint64_t step0, uint64_t seed, int64_t L,
                      double jitter, int adapt, double target_accept, double* x_dev, double* lp_dev, double* grad_dev,
                      double* state_dev, const double* minv_dev, const double* msqrt_dev, const double* lo_dev,
                      const double* hi_dev, double outside_value, double inside_const, double* save_dev, double* lpsave_dev,
                      int64_t nsave, uint64_t save0, int64_t thin, int64_t* naccept_dev, const gpb_hmc_diag* diag);
/* gpb_chain_smc_reweight / gpb_chain_smc_move <- Chain.run_SMC (smc.SMCSampler): a tempered sequential Monte Carlo sampler
 *   over the chain of ctxs — pocoMC's outer algorithm (adaptive tempering from the prior box to the posterior, resampling,
 *   MCMC moves, a running evidence) with the particle covariance as the preconditioner; there is no normalizing flow.
 *   State, device memory in and out: x [N, d] particles in the chain's original parameters, logl [N] their
 *   log-likelihoods (what gpb_chain_logpost writes with outside_value / inside_const), Lc [d, d] the lower Cholesky factor
 *   of the particle covariance (written by reweight, read by move) and the state block of GPB_SMC_STATE_WORDS 8-byte
 *   words: doubles [0] beta, [1] logz, [2] log_sigma, [3] the effective sample size at the new beta, [4] the last logz
 *   increment; unsigned 64-bit counters [8], [9] scratch of the accept kernel (zero between calls), [10] accepted
 *   proposals, [11] proposals with a NaN log-likelihood, [12] particles with a NaN log-likelihood at the last reweighting
 *   (weight 0), [13] flags: bit 0 a non-positive pivot in the Cholesky factorisation, bit 1 no particle with a finite
 *   weight.  The kernels only set the flags; the caller reads the block once per stage and decides.
 *   Limits (GPB_E_ARG): 2 <= N <= 1048576; 1 <= d <= 128 (Lc and four rows live in LDS: 8 d^2 + 32 d bytes of the 160 KiB
 *   of a workgroup); stage and step numbers below 2^32.
 * gpb_chain_smc_reweight: one stage's reweighting.  beta in (beta_prev, 1] with ESS(beta) = (sum w)^2 / sum w^2 =
 *   ess_fraction * N for w_i = exp((beta - beta_prev)(logl_i - max logl)): 1 when ESS(1) >= the target, else the upper end
 *   after exactly 60 halvings of [beta_prev, 1]; logz += logsumexp((beta - beta_prev) logl) - ln N; systematic resampling
 *   with one uniform u from the Philox counter (stage, 0, 0, 8): positions min((u + i) / N, 1 - 2^-53), the ancestor the
 *   first index whose inclusive cumulative normalised weight exceeds the position, x and logl gathered; mean and covariance
 *   (divided by N) of the resampled particles and Lc.  Optional device outputs: ancestors [N], mean [d].
 * gpb_chain_smc_move: nsteps Metropolis steps numbered step0, step0 + 1, ... (global step k; stage_step0 is the index s of
 *   the first of them within its stage), enqueued back to back, no host synchronisation; one call of n steps gives the bits
 *   of n calls of one step.  Per step and particle i: z ~ N(0, I_d) from counters (i, k, pair, 9), x' = x + exp(log_sigma)
 *   Lc z, all N proposals in one evaluation of the chain (gpb_chain_logpost, or for contexts gpb_chain_supported rejects the
 *   per-emulator sequence), accepted where ln u < beta (logl' - logl) with u from (i, k, 0, 10) and logl' neither NaN nor
 *   outside_value; then log_sigma += (accepted / N - 0.234) / (s + 1).
 *   Both are asynchronous on the contexts' stream; all pointers device memory. */
#define GPB_SMC_STATE_WORDS 16
GPB_API int gpb_chain_smc_reweight(gpb_ctx* const* ctxs, int E, int64_t N, uint64_t stage, uint64_t seed, double ess_fraction,
                           double* x_dev /*[N,d]*/, double* logl_dev /*[N]*/, double* state_dev, double* Lc_dev /*[d,d]*/,
                           int64_t* ancestors_dev /*[N] or NULL*/, double* mean_dev /*[d] or NULL*/);
GPB_API int gpb_chain_smc_move(gpb_ctx* const* ctxs, int E, int64_t N, int64_t nsteps, uint64_t step0, uint64_t stage_step0,
                       uint64_t seed, double* x_dev, double* logl_dev, double* state_dev, const double* Lc_dev,
                       const double* lo_dev, const double* hi_dev, double outside_value, double inside_const);
/* gpb_chain_emcee_prepare: everything of gpb_chain_emcee_run that can fail on one rank alone — argument and state checks,
 * workspace allocation — and nothing that is enqueued.  A sharded caller runs it on every rank and lets the ranks agree on
 * the outcome (an all-reduce of the return codes) BEFORE any rank calls gpb_chain_emcee_run: a rank that failed there
 * would leave the others waiting inside the in-stream all-gather. */
GPB_API int gpb_chain_emcee_prepare(gpb_ctx* const* ctxs, int E, int64_t nwalkers);

/* ---- walker sharding over RCCL (one process per GPU) ------------------------------ *
 * gpb_dist_uid: rank 0 obtains a 128-byte ncclUniqueId to broadcast out of band.
 * gpb_dist_init / gpb_dist_allgather: in-stream ncclAllGather of per-walker
 * log-posteriors (count doubles per rank) — the one exchange per log-prob batch.
 */
/* gpb_dist_available: 1 when librccl loads with the four entry points used here (no communicator is created): ranks
 * vote on it before gpb_dist_init, whose ncclCommInitRank is itself collective. */
GPB_API int gpb_dist_available(void);
GPB_API int gpb_dist_uid(void* uid128_host);
GPB_API int gpb_dist_init(gpb_ctx* ctx, int rank, int nranks, const void* uid128_host);
GPB_API int gpb_dist_allgather(gpb_ctx* ctx, const double* send_dev, double* recv_dev, int64_t count);
GPB_API int gpb_dist_finalize(gpb_ctx* ctx);

/* ---- options and measurement ------------------------------------------------------- *
 * gpb_ctx_option: launch-geometry and behaviour options of a context (no reference counterpart; the defaults are what the
 * numbers in DESIGN.md were measured with).  None changes a result except key 18, which moves a GP between two distance forms
 * that agree to ~1e-13, and key 51, which evaluates V = L^-1 K*^T in another arithmetic.  Keys (value ranges are checked;
 * GPB_E_ARG otherwise):
 *   0 XCD affinity of the predict kernel (-1 auto, 0 by walker tile, 1 by row block); 4 outer panel width of the blocked
 *   Cholesky (0: by size); 5 tile order of the static 64-row predict launches (1 sorted, 2 snake, 3 snake of pairs);
 *   7 / 22 switch points of the tile-shape rule (64x64 / 64x128 tiles per 256 CUs), 33 / 34 / 35 the same for compacted
 *   batches; 8 largest batch whose dense block log-likelihood runs one workgroup per walker; 9 / 12 / 14 / 50 tile (64, 128; 0 = by
 *   fill) of the in-panel Cholesky updates / the triangular-inverse levels / the end-of-panel updates / K^-1 of the LML gradient; 10 wave priority of
 *   predict tiles by K-loop length; 11 the block log-likelihood kernels sum the predict partials themselves; 17 skip the all-zero
 *   m-tiles of the predict kernel's diagonal blocks; 18 distance form of the kernel matrices (1: per GP from theta, see
 *   GPB_GET_FORM; 0: difference form for every GP; 2: Gram form for every GP); 19 / 20 design chunks per cross-kernel workgroup /
 *   walkers per lane there; 23 low-rank form of the block log-likelihood when it applies; 25 Cholesky lookahead on a side stream;
 *   27 evaluate only the rows inside the prior box; 28 size the tile rule of a compacted batch by its live rows; 29 / 30 fusions
 *   of the resident step loop (box test and gather in the proposal kernel; accept + next proposal in one launch); 36 balanced
 *   row shares of a sharded step loop (0 off: default, 1 from 8 ranks on, 2 always); 40 the emulators of a chain share one launch
 *   per kernel kind; 42 force the predict tile (0: by rule; 128, 64, 32 = 64 rows x 32 walkers, 65 = 64 x 128: every shape gives
 *   the same bits); 43 route the block log-likelihood through the generic LDS / HBM Cholesky kernel (what M > 64 takes) whatever M;
 *   44 the number of 128x128 predict tiles per 256 CUs from which the rule takes them (0: default 960);
 *   47 Cholesky by column pairs (every second trailing update takes two block columns at once, K = 128): 1 where it is the faster
 *   schedule (default: 1024 <= N <= 3072), 2 always, 0 never; results agree to rounding (another order of the same sums);
 *   49 the block log-likelihoods of a chain of emulators as one workgroup per (walker tile, emulator) and an ordered sum (1,
 *   default) or as one workgroup per walker tile that walks the emulators (0); same bits;
 *   51 V = L^-1 K*^T (sk:_gpr.py:454-460, src/emulator.py:573-575) on the INT8 matrix pipe (csrc/gpb_sliced.hip): operands as
 *   D signed 8-bit digit planes, the digit products of the D upper levels summed exactly in int32, combined in fp64; a walker's
 *   bits do not depend on batch, tile, compaction or rank count.  Contexts with a padded design size above 16384 (where the int32
 *   sums could wrap), fit-only multi contexts and calls that need K*^T in fp64 (joint covariance, gradients) take the fp64 kernel
 *   whatever the value.  3 (default): D = 7, the 28 products of levels 6..12 — as accurate as the fp64 kernel everywhere in the
 *   search box, for every context; 0: the fp64 kernel; 1: D = 6, the 21 products of levels 5..10, for every batch of a context
 *   whose GPs all have 1 + c / sigma_n^2 <= 128 (the rule reads theta alone; other contexts keep the fp64 kernel): the variance
 *   within ~2e-11 relative of the fp64 kernel's, a log-posterior within ~1e-11 .. 2e-9 depending on how far its two terms
 *   cancel; 2: D = 6 with the rule off (accuracy probes).  At cfg 4 D = 7 runs the predict launch in ~0.7 of the fp64 kernel's
 *   time, D = 6 in ~0.5.
 *   Keys 26 / 32 (one rank's share of a sharded step on a single GPU: a measurement hook) take non-zero values in the debug build
 *   only (libgpbayes_debug.so: include/gpbayes_debug.h) and return GPB_E_ARG here.  So does key 52, the bytes of gpb_chain_marginals'
 *   per-group workspace (0: GPB_MARG_WS_MB megabytes): a test hook for the sample groups, which change no count; and key 53, the
 *   bytes of gpb_chain_rank_diag's workspace (0: GPB_RANK_WS_MB megabytes): a test hook for the parameter groups, which change no bit.
 * gpb_debug_has_variants: 1 when the loaded library is that debug build (-DGPB_DEBUG_VARIANTS), 0 for the product library.
 * gpb_profile_enable / _read: HIP-event timing of the dominant kernel (k_predict: V = L^-1 K*^T + sum of squares) on the
 *   context's stream — number of timed launches, their summed duration, the (GP, walker) pairs they processed; read resets.
 *   bench.py's roofline block comes from these.
 * gpb_profile_fit_piece: enqueue ONE piece of gpb_gp_factor alone (0 = K(X,X) assembly, 1 = Cholesky, 2 = triangular inverse,
 *   3 = alpha) so that the pieces can be timed apart; leaves the context without a factorisation (gpb_gp_factor afterwards). */
GPB_API int gpb_ctx_option(gpb_ctx* ctx, int key, int value);
GPB_API int gpb_debug_has_variants(void);
GPB_API int gpb_profile_enable(gpb_ctx* ctx, int on);
GPB_API int gpb_profile_read(gpb_ctx* ctx, int64_t* launches, double* total_ms, double* units);
GPB_API int gpb_profile_fit_piece(gpb_ctx* ctx, int piece);

#ifdef __cplusplus
}
#endif
#endif /* GPBAYES_H */
