// gpb_internal.h — context layout and launch prototypes shared by the .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>
#include "../../include/gpbayes.h"
#include "../../include/gpbayes_debug.h"
#include "dev_buf.h"
#include "dispatch.h"
#include "lowrank_setup.h"
#include "ws_layout.h"

namespace gpb {

constexpr int NB = 64;          // Cholesky diagonal block / padding granule of N
constexpr int WPAD = 128;       // walker-batch padding granule (GEMM tile width)
constexpr int KX_CHUNK = 64;    // design points per kcross workgroup (mean partial granule)

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
__host__ __device__ inline int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }

}  // namespace gpb

// Which stored GP the compact slot `a` of a fit launch stands for, and that GP's design size.  A context normally holds P GPs
// over ONE design (gpb_gp_set: map = n = nullptr); gpb_gp_set_multi gives every GP its own design (the GPs of several
// emulators, or the restarts of a hyper-parameter search, in one batch: n = per-GP sizes, all padded to the same Np) and
// gpb_gp_lml_subset evaluates a subset of the stored GPs in the first slots of the workspaces (map = slot -> stored GP).
struct GpSel {
    const int* map;
    const int* n;
    int N;
    int64_t x_stride, xm_stride;   // per-GP strides of the design / its column means (0: one design for all GPs)
    __device__ __forceinline__ int q(int a) const { return map ? map[a] : a; }
    __device__ __forceinline__ int64_t Nq(int qq) const { return n ? (int64_t)n[qq] : (int64_t)N; }
};

// Where a design of N points sits among the Np = multiple of 64 stored rows: rows [pad_front, pad_front + N).  The padding goes in
// FRONT in whole 16-row units — the predict tiles' K-step: those leading zero rows of K*^T are skipped outright and their rows of V
// fall into the lightest row block — and the remainder (< 16 rows) behind.
__host__ __device__ __forceinline__ int64_t pad_front(int64_t Np, int64_t N) { return ((Np - N) / 16) * 16; }

// k(r) / c as a function of the squared scaled distance, plain libm form (fast_math.h has the fast forms of k_kmat_mfma and k_kcross)
template <int KIND>
__device__ __forceinline__ double shape_fn(double r2) {
    if (KIND == GPB_KERNEL_RBF) {
        return exp(-0.5 * r2);                                   // sk:kernels.py:1557
    } else if (KIND == GPB_KERNEL_MATERN15) {
        const double t = sqrt(r2) * 1.7320508075688772;          // sk:kernels.py:1721-1723
        return (1.0 + t) * exp(-t);
    } else {
        const double t = sqrt(r2) * 2.23606797749979;            // sk:kernels.py:1724-1726
        return (1.0 + t + t * t / 3.0) * exp(-t);
    }
}

struct LoopGroup;
struct gpb_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;

    // ---- GP state -------------------------------------------------------------
    int64_t N = 0, Np = 0, d = 0, dpad = 0, P = 0;
    int kind = 0;
    double alpha_reg = 0.0;
    bool have_theta = false, factored = false;
    std::vector<double> h_theta;   // host [P][d+2]
    bool multi = false;            // gpb_gp_set_multi: every GP has its own design (fit-only context: no predict / likelihood)
    int64_t Pstore = 0;            // GPs stored (P is the number a launch covers: Pstore, or the subset's size inside gpb_gp_lml_subset)
    gpb::DevBuf<int> gpN;            // device [Pstore] design points per GP (multi)
    int* gpmap = nullptr;          // device [Pstore] slot -> stored GP of the current subset evaluation
    bool subset = false;           // inside gpb_gp_lml_subset
    std::vector<int> h_N;          // host [Pstore]
    std::vector<int> h_map;        // host [P] of the current subset
    GpSel sel() const {
        return GpSel{subset ? gpmap : nullptr, multi ? gpN.get() : nullptr, (int)N, multi ? Np * dpad : 0, multi ? dpad : 0};
    }
    gpb::DevBuf<double> X;           // [Np][dpad]   raw design (pad rows/cols zero); multi: [Pstore][Np][dpad]
    gpb::DevBuf<double> Xsc;         // [P][Np][dpad] design / length_scale_p
    gpb::DevBuf<double> xmean;       // [dpad] column means of the design (0 in the padding); multi: [Pstore][dpad]
    gpb::DevBuf<double> muS;         // [P][dpad] xmean / length_scale_p
    gpb::DevBuf<double> Xc;          // [P][Np][dpad] Xsc - muS: centred scaled design (dot-product form of k_kcross)
    gpb::DevBuf<double> dnorm;       // [P][Np] squared norms of the rows of Xc
    // Distance form per GP (chosen from theta alone: gpb_gp_set_theta -> choose_forms).  0 = Gram form r^2 = |a|^2 + |b|^2 - 2 a.b
    // on the centred design (k_kcross<DOT>, k_kmat_mfma), 1 = difference form sum ((a_k - b_k))^2 on X / l as sklearn's cdist
    // computes it (sk:kernels.py:1556,1564,1711-1716).  The Gram form's cancellation costs ~eps (|a|^2 + |b|^2) absolute in
    // r^2: a GP whose S = sum_k (extent_k / l_k)^2 exceeds gram_limit takes the difference form.
    std::vector<double> h_ext;     // host [d] column extents (max - min) of the design; multi: [Pstore][d]
    std::vector<int> h_form;       // host [P]
    int* gpform = nullptr;         // device [P]
    gpb::DevBuf<int> kmtiles;        // device [Np/64 (Np/64 + 1) / 2][2]: (row block, column block) of tile t of the lower block triangle (k_kmat_mfma)
    int n_diff = 0;                // GPs in the difference form
    double gram_limit = 1024.0;    // S above this: difference form (r^2 within ~1e-13 absolute, K within ~2e-13, below it)
    double* ls = nullptr;          // [P][dpad]    length scales (1 in pad columns)
    double* amp = nullptr;         // [P] c
    double* noise = nullptr;       // [P] sigma_n^2
    gpb::DevBuf<double> Z;           // [P][Np]
    // per-point simulation noise (gpb_gp_set_point_noise; nullptr: none): s [Pstore][Np], laid out and indexed like Z (design point i
    // of stored GP q at [q * Np + pad_front + i], zero in the padding).  The training diagonal is c + sigma_n^2 + (alpha_reg + s).
    gpb::DevBuf<double> pnoise;
    gpb::DevBuf<double> K;           // [P][Np][Np]  K, overwritten by L (lower) in gp_factor
    gpb::DevBuf<double> Linv;        // [P][Np][Np]
    // sliced-integer predict (gpb_sliced.hip, option key 51): int8 digit planes of L^-1 (made on first use after a factorisation)
    // and of the current K*^T batch, row / column scales
    // 0 = fp64 kernel always; 1 = six digit planes where their rule admits the context; 2 = six, rule off (tests);
    // 3 (default) = seven digit planes (fp64-accurate) wherever the int32 sums stay exact (Np <= 16384)
    int predict_sliced = 3;
    gpb::DevBuf<int8_t> slA;         // [P][D][Np/16][Np128][16], room for D = 7 planes per GP
    gpb::DevBuf<int8_t> slB;         // [P][D][Np/16][Wcap][16] (leading dimension of a batch: Wld), room for D = 7
    gpb::DevBuf<double> sl_scale;    // rowscale [P][Np128] | colscale [P] | rowexp (int) [P][Np128]
    bool slA_valid = false;
    int slA_depth = 0;             // digit planes per operand of the planes in slA (6 or 7)
    int batch_sliced = 0;          // the current batch's K*^T exists as this many digit planes (launch_kcross), 0: as fp64
    bool want_kst = false;         // the caller of launch_kcross needs the fp64 K*^T itself (joint covariance)
    gpb::DevBuf<double> T;           // [P][Np][Np]  workspace (trtri / K^-1)
    gpb::DevBuf<double> yv;          // [P][Np]      L^-1 z
    gpb::DevBuf<double> alpha;       // [P][Np]      K^-1 z
    gpb::DevBuf<int> info;           // [P]
    gpb::DevBuf<double> lmlbuf;      // [P][4]
    gpb::DevBuf<double> gpart;       // gradient partials

    // ---- predict workspace ------------------------------------------------------
    int64_t Wcap = 0;              // padded capacity (multiple of WPAD)
    int64_t last_W = 0;            // rows of the most recent K*^T batch (gpb_gp_get GPB_GET_KSTAR)
    int64_t Wld = 0;               // leading dimension of the current batch's workspaces (set by launch_predict: the padded batch)
    gpb::DevBuf<double> Xs;          // [Wcap][d] staged inputs (when caller passes host memory)
    gpb::DevBuf<double> estd;        // [Wcap]
    gpb::DevBuf<double> KsT;         // [P][Np][Wcap]
    gpb::DevBuf<double> mpart;       // [Np/KX_CHUNK][P][Wcap]
    gpb::DevBuf<double> spart;       // [Np/64][P][Wcap]  sum-of-squares partials per 64-row block
    gpb::DevBuf<double> mean_pc;     // [P][Wcap]
    gpb::DevBuf<double> var_pc;      // [P][Wcap]
    unsigned long long* live_hint = nullptr;   // pinned host memory: (batch rows << 32) | live rows of the last finished compaction
    gpb_ctx* hint_from = nullptr;  // whose live_hint sizes this context's tile rule (the chain's first emulator compacts)
    int fuse_accept_propose = 1;   // tune key 30: accept of a half-step + proposal of the next in one launch (needs premark 2)
    int balance_shards = 0;        // tune key 36: sharded C loop takes equal slices of the ordered live-row list (1: from 8 ranks on, 2: always; default off)
    gpb::DevBuf<int> bal_ws;         // its flags / ranks / scatter lists
    int sim_rank = 0;              // tune key 32: which rank of sim_ranks the measurement hook plays
    int tile_by_live = 1;          // tune key 28
    int premark = 2;               // tune key 29: the C-driven loop's proposal kernel takes the prior-box test (1) and gathers the rows inside (2)
    gpb::DevBuf<double> cmp_X;       // the rows of the current batch inside the prior box, gathered in order [Wcap][chain ndim]
    gpb::DevBuf<int> cmp_idx;        // compaction of a log-posterior batch to the rows inside the prior box: [0] = count, [4..] = row indices
    int compact = 1;               // gpb_logpost / gpb_emcee_run evaluate the rows inside the box only (the reference: src/mcmc.py:278-283)
    gpb::DevBuf<unsigned long long> rows_live;   // device counter: rows evaluated by compacted launches while profiling
    bool prof_compacted = false;
    gpb::DevBuf<double> vbuf;        // [P][Np][Wcap] V = L^-1 K*^T (covariance path only)
    gpb::DevBuf<double> gbuf;        // gradient path (gpb_grad.hip): beta^T = (K^-1 K*^T)^T [P][Wld][Np], then per-row pieces
    gpb::DevBuf<double> covbuf;      // [P][Wc][Wc]
    gpb::DevBuf<double> out_stage;   // staging for host outputs
    gpb::DevBuf<double> diag_ws;     // chain diagnostics (gpb_diag.hip): Y [G][nsteps to 64][nwalkers to 16] | lag partials | walker statistics
    // chain marginals (gpb_marg.hip): edges | h1 | outside | h2 | pairs | integer weights | one code byte per (sample, parameter)
    // of a sample group; marg_ws_bytes caps the last two (option key 52 lowers it, in the debug build only: the grouping's test)
    gpb::DevBuf<int64_t> marg_ws;
    // rank-normalised diagnostics (gpb_rank.hip): RankWs of ws_layout.h; rank_ws_bytes caps it (option key 53 lowers it, in the
    // debug build only: the grouping's test)
    gpb::DevBuf<int64_t> rank_ws;
    int64_t rank_ws_bytes = (int64_t)GPB_RANK_WS_MB << 20;
    int64_t marg_ws_bytes = (int64_t)GPB_MARG_WS_MB << 20;
    gpb::DevBuf<int64_t> hm_ws;      // history matching (gpb_hm.hip): HmWs of ws_layout.h; marg_ws_bytes caps the codes of a sample group
    gpb::DevBuf<int64_t> curves_ws;  // posterior curves and trace histograms (gpb_curves.hip): CurvesWs of ws_layout.h
    gpb::DevBuf<int64_t> kmeans_ws;  // posterior clusters (gpb_kmeans.hip): KmeansWs of ws_layout.h
    gpb::DevBuf<int64_t> knn_ws;     // nearest-neighbour distances (gpb_knn.hip): KnnWs of ws_layout.h
    gpb::DevBuf<int64_t> stein_ws;   // Stein thinning and discrepancy (gpb_stein.hip): SteinThinWs / SteinKsdWs of stein_plan.h
    gpb::DevBuf<double> eig_ws;      // expected information gain (gpb_eig.hip): EigWs of ws_layout.h
    gpb::DevBuf<int64_t> maxpro_ws;  // MaxPro Latin-hypercube designs (gpb_maxpro.hip): MaxproWs of ws_layout.h
    gpb::DevBuf<double> sens_ws;     // gpb_sens_accumulate (gpb_sens.hip): per-row F | diag Cw | L^-1 J (large rows) | chunk sums | flags
    // goodness of fit (gpb_gof.hip): gpb_gof_accumulate's per-row z | pulls | p | chunk sums | flags, or gpb_gof_influence's minima | chunk sums
    gpb::DevBuf<double> gof_ws;
    // leave-one-out (gpb_loo.hip, gpb_psis.hip): gpb_loo_pointwise's z | row copy of the rows worked in place, or gpb_psis's gathered
    // tails x | sample index | index by rank | rank and, for host callers, the staged rows and results
    gpb::DevBuf<double> loo_ws;
    // cross-validation (gpb_cv.hip): the folds of the planned call (idx [n] | fold_ptr [nf + 1], host copy h_cv), then the
    // leave-one-out path's sum-of-squares partials [P][Np/64][Np]
    gpb::DevBuf<int> cv_ws;
    std::vector<int> h_cv;
    int64_t cv_n = 0, cv_nf = 0, cv_kmax = 0;
    bool cv_loo = false, cv_has_idx = false;
    // Sobol indices (gpb_sobol.hip): I | E tables [P][N][dpad] each, e partials [P][Np/64], then what the call needs (tile
    // partials, staged results); the box of the planned call, lo [d] | hi [d]
    gpb::DevBuf<double> sobol_ws;
    std::vector<double> h_sobol_box;
    // sequential design (gpb_design.hip): gpb_design_begin's block x_c [C][d] | x_r [R][d] | w [Rp] | g [P] | s(c,c) [P][Cp] |
    // V_c [P][Np][Cp] | V_r [P][Np][Rp] | S_rc [P][Rp][Cp] (Cp, Rp: C, R padded to 128), then gpb_chain_design_run's own
    // (design_run: the picks' scaled rows u_c [T][P][Cp], the pending u_r [P][Rp], chunk partials, scores, denominators)
    gpb::DevBuf<double> design_ws;
    gpb::DevBuf<double> design_run;
    int64_t design_C = 0, design_R = 0;
    bool design_ready = false;     // begun and not yet consumed by a run (the run conditions S_rc in place)
    bool design_noise = false;     // gpb_design_set_noise: the begin block's s_c [P][Cp] holds the candidates' simulation noise

    // ---- emulator transform / likelihood ----------------------------------------
    int mode = 0;
    int64_t M = 0;
    bool have_transform = false, have_like = false;
    // host copies of the observable transform (PCA modes) for the low-rank form of the likelihood
    std::vector<double> h_A, h_mu, h_C0;
    // low-rank likelihood (gpb_like.hip, k_loglike_lowrank): C = C0 + A^T D A with C0 = C_trunc + C_exp fixed
    gpb::DevBuf<double> lr_R;        // [16][16] upper-triangular R of  L0^-1 A^T = Q R  (zero padded)
    gpb::DevBuf<double> lr_v0;       // [16]     Q^T L0^-1 (mu - yexp)
    double lr_cperp = 0.0;         // |(I - Q Q^T) L0^-1 (mu - yexp)|^2
    double lr_logdet0 = 0.0;       // log det C0
    bool lr_ok = false;
    int lowrank = 1;               // use it when it applies (tune key 23)
    int lr_split = 1;              // option key 49: a chain's block likelihoods as one workgroup per (walker tile, emulator) + an ordered sum
    gpb::DevBuf<double> lr_blocks;   // [E][Wcap] the emulators' blocks of a chain's batch (chain's first context)
    // many data sets against the installed covariance (gpb_chain_like_sets): the factorisation of C0 kept on the host
    // (lowrank_setup.h), and per data set k the row v0[k][16] (zero padded like lr_v0) and cperp[k].  lrs_K = 0: none.
    gpb::LowrankFactor lr_fac;
    gpb::DevBuf<double> lrs_v0;      // [lrs_K][16]
    gpb::DevBuf<double> lrs_cperp;   // [lrs_K]
    int64_t lrs_K = 0;
    gpb::DevBuf<uint64_t> sets_seeds;  // gpb_chain_emcee_sets_run: the ensembles' generator keys [K]
    gpb::DevBuf<double> A;           // [P][M]
    gpb::DevBuf<double> mu;          // [M]
    gpb::DevBuf<double> scale;       // [M]
    gpb::DevBuf<double> C0;          // [M][M] cov_trunc (zeros if absent)
    gpb::DevBuf<double> yexp;        // [M]
    gpb::DevBuf<double> Cexp;        // [M][M]
    gpb::DevBuf<double> mvn_ws;      // global fallback for M > 128: [Wcap][M][M]
    gpb::DevBuf<int> notpd;          // device counter
    gpb::DevBuf<long long> n_nan;    // device counter: NaN log-probabilities seen by the stretch move's accept step
    gpb::DevBuf<double> mc_ws;       // gpb_emcee_run: proposals q[nh][d], factor[nh], log-probabilities lpq[nh]
    gpb::DevBuf<double> ptl_ws;      // gpb_chain_ptlmc_run: draws, proposals, their lp / gradient, the other state buffers
    gpb::DevBuf<double> hmc_ws;      // gpb_chain_hmc_run: the trajectory (momenta, positions, gradient, lp), H0, step size, escape flags
    gpb::DevBuf<double> smc_ws;      // gpb_chain_smc_*: weights, their scan, the gathered / proposed particles, moments
    int sim_ranks = 0;             // measurement hook: gpb_emcee_run evaluates 1/sim_ranks of every batch (one rank's share)
    int num_cu = 256;               // multiprocessor count of the device
    int64_t narrow_switch = 1280;   // 64x64 tiles when at least this many of them exist per 256 CUs, else 64x32
    int chain_batch = 1;            // tune key 40: a chain's emulators of equal padded size share one predict launch
    gpb::DevBuf<unsigned> tile_counter;   // 8 ticket queues (stride 16) + done counter [128]; re-armed by the kernel
    int64_t chol_outer = 0;        // outer panel width of the two-level blocked Cholesky (0 = chosen by size, gpb_chol.hip)
    int chol_pair = 1;             // option key 47: column pairs — every second trailing update by two columns at once (k_chol_update2):
                                   // 1 = where measured faster (1024 <= Np <= 3072), 2 = always, 0 = never
    int chol_lookahead = 1;        // far part of a panel's trailing update on a side stream, under the next panel's chain
    // ls / amp / noise / gpform / gpmap are carved out of ONE device block (thblk) so that a new theta goes up in ONE asynchronous
    // copy from its page-locked twin (h_thblk) — round 5: an LML evaluation made 6 blocking copies and 5 synchronisations
    gpb::DevBuf<double> thblk;
    double* h_thblk = nullptr;
    size_t thblk_bytes = 0;
    double* h_res = nullptr;       // page-locked: [lmlbuf doubles | info ints] of an LML evaluation's read-back
    hipStream_t side_stream = nullptr;
    std::vector<hipEvent_t> chol_events;
    int syrk_tile = 0;              // tile of the end-of-panel trailing updates (0 = by fill, 64, 128)
    int trtri_tile = 0;            // tile of the triangular-inverse levels (0 = by fill, 64, 128)
    int kinv_tile = 0;             // option key 50: tile of K^-1 = L^-T L^-1 (LML gradient; 0 = by fill, 64, 128)
    int chol_inner_tile = 64;      // tile of the K=64 trailing updates inside an outer panel (64 or 128)
    int resident_order = 2;         // static 64-row predict launches: order of the tiles over the CUs, 1-3 (2 = snake)
    gpb::DevBuf<unsigned> tile_trace; // debug hook: [count, capacity, pad x6][capacity][8] records of k_predict tiles
    int tile_priority = 1;         // k_predict: wave priority by K-loop length (s_setprio)
    int kcross_chunks = 0;         // 64-row chunks of the design per k_kcross workgroup (0 = by grid size)
    int kcross_wpl = 2;            // walkers per lane of k_kcross (1 or 2)
    int kcross_dot = 1;            // tune key 18: distance form of k_kcross / K(X,X): 1 = per GP by theta (see gpform), 0 = every GP the
                                   // difference form, 2 = every GP the Gram form (tests: what the rule protects against)
    int tri_skip = 1;              // k_predict: skip the all-zero half of the diagonal block's second half
    int force_tile = 0;           // test hook: 0 = auto, 64 / 128 / 32 (= 64x32) force the k_predict tile
    int force_xcd = -1;             // tuning hook: -1 auto, 0 / 1 = k_predict XCD affinity by walker tile / row block
    int64_t tile_switch = 960;      // use 128x128 tiles when at least this many of them exist per 256 CUs (measured)
    int64_t mid_switch = 1280;      // else 64x128 tiles when at least this many of THEM exist, else 64x64 / 64x32
    int64_t tile_switch_c = 2400, mid_switch_c = 1150, narrow_switch_c = 2400;   // the same for compacted batches (tune keys 33-35)
    bool force_generic_mvn = false; // test hook: bypass the register-resident MVN fast path
    int fuse_finalize = 1;          // block log-likelihood kernels sum the predict partials themselves (P <= 32)
    int64_t mvn_wg_switch = 768;   // batches up to this size use one workgroup per walker (32 < M <= 64)
    // ---- coupled chain likelihood (gpb_coupled.hip; coupled_setup.h has the algebra) ----------------------
    // like_epoch: counts the replacements of this context's transform / likelihood block (gpb_gp_set, gpb_emu_set_transform,
    // gpb_like_set).  cpl: the joint tables of the chain whose FIRST context this is (gpb_chain_like_set) — the member
    // contexts in emuList order with their epochs at set time: a member whose epoch has moved on makes the coupling stale.
    uint64_t like_epoch = 0;
    struct Coupling {
        bool on = false;
        int PT = 0, PP = 0;            // GPs of the chain, and the kernels' padded order (64 or 128)
        std::vector<gpb_ctx*> members;
        std::vector<uint64_t> epochs;
        double cperp = 0.0, logdet0 = 0.0;
        const double *RT = nullptr, *v0 = nullptr;     // pieces of cpl_tab (CoupledWs)
    } cpl;
    gpb::DevBuf<double> cpl_tab;

    // ---- parameterTrafoPCA input map (gpb_pmap.hip) ------------------------------------
    gpb::DevBuf<int> pmap_int;       // col_src[d_out] | group descriptors [G][6]
    gpb::DevBuf<double> pmap_tab;    // [G][4 + maxpc][100]
    int64_t pmap_d_in = 0, pmap_d_out = 0;
    int pmap_groups = 0, pmap_maxpc = 0;

    // ---- profiling (HIP events around k_predict) ------------------------------------
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    double prof_units = 0.0;       // (GP, walker) pairs processed by the timed launches
    double prof_gps = 0.0;         // GPs per timed launch (a chain's batched launch: those of all its emulators)

    // ---- RCCL ---------------------------------------------------------------------
    void* comm = nullptr;
    int rank = 0, nranks = 1;
    struct LoopGroup* loop = nullptr;   // test hook (gpb_debug_loopback_group): R contexts of ONE process as the ranks of a communicator
};

#define GPB_HIP(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);               \
            return GPB_E_HIP;                                                           \
        }                                                                               \
    } while (0)

#define GPB_FAIL(code, msg)                                                             \
    do {                                                                                \
        ctx->err = (msg);                                                               \
        return (code);                                                                  \
    } while (0)

namespace gpb {
// The result of a with_int / with_dpad / with_kind at a launch site (dispatch.h).  NO_CASE: the context holds a value that
// `what` has no instantiation for, which the entry checks rule out: a list in this library is incomplete.
inline int dispatched(gpb_ctx* ctx, int rc, const char* what) {
    if (rc == NO_CASE) GPB_FAIL(GPB_E_STATE, std::string("gpb: internal: no instantiation of ") + what + " for this context");
    return rc;
}

// The device buffers of a context: DevBuf members (dev_buf.h), allocated through these two and given back by `delete ctx`
// once gpb_ctx_destroy has idled the streams.  Before a held buffer goes back to the cache, the context's stream and its
// look-ahead stream are synchronised: nothing enqueued still uses it.  (Nothing is synchronised for an empty buffer or one
// that is large enough — the steady state.)  A failure leaves the buffer empty, never dangling.
// THE RULE for an entry point that replaces buffers: lower the flags and sizes that declare them valid (N, have_*, Wcap,
// pmap_d_in, ...) BEFORE its first allocation and raise them after its last, so a failure half-way leaves a context that
// its checks reject, not one that launches on a null pointer.
// ctx_replace: exactly n elements, now (contents undefined)
template <typename T>
inline int ctx_replace(gpb_ctx* ctx, DevBuf<T>& b, int64_t n) {
    if (b) {
        GPB_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->side_stream) GPB_HIP(hipStreamSynchronize(ctx->side_stream));
    }
    GPB_HIP(b.alloc(n));
    return 0;
}
// ctx_grow: a workspace of at least `need` elements (never shrunk; the contents are not kept) — for a buffer that is ONE array.
// THE RULE for a buffer with more than one piece: it is sized by ctx_carve, and a result that goes to the caller's device
// pointer or to host memory goes through HostOut (both below); no total is summed by hand next to the offsets it must cover.
template <typename T>
inline int ctx_grow(gpb_ctx* ctx, DevBuf<T>& b, int64_t need) {
    return b.cap >= need ? 0 : ctx_replace(ctx, b, need);
}
// ctx_carve: `layout(Carver<T>&)` — a list of take() calls that only assigns pointers (ws_layout.h) — runs once counting, the
// buffer grows to that total, and it runs again over the buffer: the pointers it leaves cannot exceed what was allocated.
template <typename T, typename F>
inline int ctx_carve(gpb_ctx* ctx, DevBuf<T>& b, F&& layout) {
    Carver<T> count;
    layout(count);
    if (const int rc = ctx_grow(ctx, b, count.total())) return rc;
    Carver<T> pieces(b.get());
    layout(pieces);
    return 0;
}

// The results (and staged inputs) of an entry point whose caller passes device pointers (on_device) or host memory.  Device
// mode: every piece is the caller's pointer and finish() does nothing.  Host mode: every piece is a piece of a staging buffer
// (out_stage unless reserve() is given another), finish() copies the results back on the context's stream and synchronises
// it once.  always_staged: the kernels write the stage in device mode too and finish() copies device-to-device.  A null
// caller pointer yields a null piece.
//     HostOut so(ctx, on_device);
//     double *dm, *dv;
//     so.out(dm, mean, n); so.out(dv, var, n);
//     if ((rc = so.reserve())) return rc;
//     ... launch into dm, dv ...
//     return so.finish();
struct HostOut {
    static constexpr int MAX_PIECES = 8;
    struct Piece {
        double** slot;             // where reserve() leaves the piece's pointer (nullptr: a piece placed by the caller, at())
        void* user;
        void* stage;
        int64_t n;                 // doubles to carve
        size_t row_bytes, rows, user_pitch;     // rows > 0: a pitched result, copied back row by row
        bool load, store;
    };
    gpb_ctx* ctx;
    bool on_device, always_staged, overflow = false;
    Piece pc[MAX_PIECES];
    int np = 0;

    HostOut(gpb_ctx* c, bool on_dev, bool always = false) : ctx(c), on_device(on_dev), always_staged(always) {}
    bool staged() const { return !on_device || always_staged; }
    // n doubles of result; load: the stage starts as a copy of the caller's values (an accumulating kernel)
    void out(double*& dev, double* user, int64_t n, bool load = false) {
        dev = user;
        if (user && staged()) add(Piece{&dev, user, nullptr, n, sizeof(double) * (size_t)n, 0, 0, load, true});
    }
    // rows x W doubles of result with the caller's leading dimension ld; returns the leading dimension to write `dev` with
    int64_t out2d(double*& dev, double* user, int64_t rows, int64_t W, int64_t ld) {
        dev = user;
        if (!user || !staged()) return ld;
        add(Piece{&dev, user, nullptr, rows * W, sizeof(double) * (size_t)W, (size_t)rows, sizeof(double) * (size_t)ld, false, true});
        return W;
    }
    // n doubles of input
    void in(const double*& dev, const double* user, int64_t n) {
        dev = user;
        if (user && !on_device)
            add(Piece{const_cast<double**>(&dev), const_cast<double*>(user), nullptr, n, sizeof(double) * (size_t)n, 0, 0, true, false});
    }
    // n doubles of the stage that no caller sees (keeps the pieces behind it where they are)
    void gap(int64_t n) {
        if (staged()) add(Piece{nullptr, nullptr, nullptr, n, 0, 0, 0, false, false});
    }
    // a result of n elements whose stage the caller has placed (a piece of a layout): the pointer to write
    template <typename T>
    T* at(T* user, T* stage, int64_t n) {
        if (!user || !staged()) return user;
        add(Piece{nullptr, user, stage, 0, sizeof(T) * (size_t)n, 0, 0, false, true});
        return stage;
    }
    // the same for an input; enqueues its upload at once
    int in_at(const double*& dev, const double* user, double* stage, int64_t n) {
        dev = user;
        if (!user || on_device) return 0;
        GPB_HIP(hipMemcpyAsync(stage, user, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        dev = stage;
        return 0;
    }
    // places the pieces of out() / out2d() / in() / gap() in `buf` behind what `front(Carver<double>&)` takes (a workspace whose
    // tail is the stage), sizes the buffer for both, and uploads the inputs
    template <typename F>
    int reserve(DevBuf<double>& buf, F&& front) {
        if (overflow) GPB_FAIL(GPB_E_ARG, "gpb: internal: HostOut has more pieces than it has room for");
        if (const int rc = ctx_carve(ctx, buf, [&](Carver<double>& c) {
                front(c);
                for (int i = 0; i < np; ++i) {
                    if (pc[i].n <= 0) continue;
                    pc[i].stage = c.take<double>(pc[i].n);
                    if (pc[i].slot) *pc[i].slot = static_cast<double*>(pc[i].stage);
                }
            }))
            return rc;
        for (int i = 0; i < np; ++i)
            if (pc[i].load) GPB_HIP(hipMemcpyAsync(pc[i].stage, pc[i].user, pc[i].row_bytes, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
    int reserve() {
        return reserve(ctx->out_stage, [](Carver<double>&) {});
    }
    // the copies to the caller, no synchronisation (an entry point that has more to enqueue in front of it)
    int copy_back() {
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        for (int i = 0; i < np; ++i) {
            const Piece& p = pc[i];
            if (!p.store) continue;
            if (p.rows)
                GPB_HIP(hipMemcpy2DAsync(p.user, p.user_pitch, p.stage, p.row_bytes, p.row_bytes, p.rows, kind, ctx->stream));
            else
                GPB_HIP(hipMemcpyAsync(p.user, p.stage, p.row_bytes, kind, ctx->stream));
        }
        return 0;
    }
    int finish() {
        if (const int rc = copy_back()) return rc;
        if (!on_device) GPB_HIP(hipStreamSynchronize(ctx->stream));
        return 0;
    }

 private:
    void add(const Piece& p) {
        if (np == MAX_PIECES) overflow = true;
        else pc[np++] = p;
    }
};
// fit side (gpb_fit.hip)
int launch_scale_design(gpb_ctx* ctx);
int choose_forms(gpb_ctx* ctx, bool upload = true);    // gpb_api.hip: per-GP distance form from h_theta and the design's extents
int launch_kmat(gpb_ctx* ctx);
int launch_potrf(gpb_ctx* ctx);
int launch_trtri(gpb_ctx* ctx);
int launch_alpha(gpb_ctx* ctx);
int launch_lml_value(gpb_ctx* ctx);
int launch_lml_grad(gpb_ctx* ctx, double* grad_host);
// predict side (gpb_predict.hip)
int ensure_wcap(gpb_ctx* ctx, int64_t W);
// finalize = false leaves the mean / variance as partials (mpart, spart) for a consumer that sums them itself
// nrows_dev (device int, optional): the batch was compacted, only its first *nrows_dev rows are live
int launch_predict(gpb_ctx* ctx, const double* Xs_dev, int64_t W, bool need_var, bool finalize = true,
                   const int* nrows_dev = nullptr);
// its three phases, for callers that batch the middle one over several contexts (chains of emulators)
int launch_kcross(gpb_ctx* ctx, const double* Xs_dev, int64_t W, const int* nrows_dev, bool allow_planes = true);
int launch_kcross_group(gpb_ctx* const* ctxs, const double* const* Xs, int E, int64_t W, const int* nrows_dev);
int launch_param_maps(gpb_ctx* const* ctxs, int n, const double* X_dev, int64_t W);      // gpb_pmap.hip
int launch_vsq(gpb_ctx* const* ctxs, int E, int64_t W, const int* nrows_dev);
// rows of a compacted batch the last finished compaction suggests will be live (the tile rules), `rows` when nothing is known
int64_t live_rows_estimate(const gpb_ctx* ctx, int64_t W, const int* nrows_dev, int64_t rows);
int launch_finalize(gpb_ctx* ctx, int64_t W, bool need_var);
// gpb_sliced.hip: the int8 form of launch_vsq's 128 x 128 launch for ONE context (rule: sliced_applies)
int sliced_applies(const gpb_ctx* ctx);             // digit planes per operand (6, 7) the context's batches take, 0: the fp64 kernel
int sliced_prepare(gpb_ctx* ctx, int depth);         // buffers, and the planes of L^-1 after a new factorisation or depth
const double* sliced_colscale(const gpb_ctx* ctx);   // device [P]: the power-of-two scale of each GP's K*^T digits
int launch_vsq_sliced(gpb_ctx* ctx, int64_t W, const int* nrows_dev, int kskip);
int launch_vsq_sliced_multi(gpb_ctx* const* ctxs, int E, int64_t W, const int* nrows_dev, int kskip);   // the GPs of E contexts, one launch
void sliced_free(gpb_ctx* ctx);
int sliced_read_kstar(gpb_ctx* ctx, int64_t p, int64_t pad, int64_t N, int64_t W, double* out);
constexpr int GPB_MAX_MULTI_GP = 96;      // GPs one batched launch can address (its table is a kernel argument)
int launch_predict_cov(gpb_ctx* ctx, const double* Xs_dev, int64_t W, double* cov_dev);
int launch_vmat(gpb_ctx* ctx, double* dst = nullptr);     // gpb_cov.hip: vbuf (or dst [P][Np][Wld]) = L^-1 K*^T of the current (fp64) batch
// closed-form cross-validation (gpb_cv.hip): cv_plan checks the folds (GPB_E_ARG / GPB_E_STATE) and uploads them, launch_cv
// writes element (GP p, position q of idx) of the hold-out mean / variance at [p * sp + q * si] and, when cov_dev is given,
// the fold covariance blocks [P][nf][kmax][kmax]
int cv_plan(gpb_ctx* ctx, const char* who, const int32_t* idx, int64_t n_idx, const int32_t* fold_ptr, int64_t nf, int64_t* kmax);
int launch_cv(gpb_ctx* ctx, double* mean_dev, double* var_dev, int64_t sp, int64_t si, double* cov_dev);
// closed-form Sobol indices (gpb_sobol.hip): sobol_plan checks state and box (GPB_E_STATE / GPB_E_ARG), keeps the box and selects
// the device.  sobol_lay: the front of ctx->sobol_ws (SobolWs: the tables every call needs and, with_part, launch_sobol's tile
// partials); the entry points carve what else they need behind it and size the buffer (ctx_carve / HostOut::reserve)
int sobol_plan(gpb_ctx* ctx, const char* who, const double* lo, const double* hi, bool need_transform);
void sobol_lay(const gpb_ctx* ctx, Carver<double>& c, SobolWs& ws, bool with_part);
int launch_sobol(gpb_ctx* ctx, double* e_dev, double* H_dev);
int launch_sobol_obs(gpb_ctx* ctx, const double* e_dev, const double* H_dev, double* mean, double* var, double* first, double* total);
int launch_sobol_main_effect(gpb_ctx* ctx, int64_t j, const double* t_dev, int64_t G, double* zbuf_dev, double* curve_dev);
// likelihood (gpb_like.hip)
int launch_obs(gpb_ctx* ctx, int64_t W, const double* estd_dev, double* mean_dev, double* cov_dev);
// the same batch's mean and covariance DIAGONAL, observable-major: mean_T / var_T [M][ld] (var_T may be nullptr), columns < W
int launch_obs_diag(gpb_ctx* ctx, int64_t W, const double* estd_dev, double* mean_T, double* var_T, int64_t ld);
// posterior-predictive summaries over the sample axis of [M][ld] arrays (gpb_ppd.hip): one workgroup per row and kernel.
// k [2 nq]: the ranks of the order statistics, (k_i, min(k_i + 1, S - 1)) per level.  Outputs that are nullptr are skipped.
constexpr int PPD_MAX_Q = 16;
struct PpdLevels {
    double q[PPD_MAX_Q];
    long long k[2 * PPD_MAX_Q];
    int nq;
};
int launch_ppd(gpb_ctx* ctx, const double* mu_T, const double* var_T, int64_t M, int64_t S, int64_t ld, const PpdLevels& lv,
               const double* vadd, const double* yobs, double* moments, double* order, double* mixq, double* pit);
// history matching (gpb_hm.hip), checked arguments, everything on the context's stream: candidate rows in a box; the maps of a
// per-row score over the parameters, minima and counts taken onto the caller's device arrays
int launch_hm_uniform(gpb_ctx* ctx, const double* lo_host, const double* hi_host, int d, uint64_t row0, int64_t S, uint64_t seed,
                      double* X, int64_t ld);
int launch_hm_maps(gpb_ctx* ctx, const double* x, int64_t S, int64_t d, int64_t row_stride, const double* score, double cutoff,
                   const double* edges_host, int B, const int32_t* pairs_host, int64_t npairs, int init, double* min1, int64_t* cnt1,
                   int64_t* nroy1, double* min2, int64_t* cnt2, int64_t* nroy2);
// true when launch_loglike will take the block log-likelihood kernels that sum the partials themselves
bool loglike_fuses_finalize(const gpb_ctx* ctx, int64_t W);
// cmp_dev (optional): the batch was compacted by launch_compact: row w of the workspace is row cmp_dev[4 + w] of ll_dev
int launch_loglike(gpb_ctx* ctx, int64_t W, double* ll_dev, bool accumulate, bool from_partials,
                   const double* X_box = nullptr, const double* lo_dev = nullptr, const double* hi_dev = nullptr,
                   double outside = 0.0, double inside_const = 0.0, const int* cmp_dev = nullptr);
// ll[row] = outside for the rows outside the open box; the rows inside are gathered into ctx->cmp_X (in order), their
// indices and count into ctx->cmp_idx
int launch_compact(gpb_ctx* ctx, const double* X_dev, int64_t W, int64_t dx, const double* lo_dev, const double* hi_dev,
                   double outside, double* ll_dev, int premarked = 0);
int ensure_cmp_rows(gpb_ctx* ctx, int64_t dx);
int launch_mvn(gpb_ctx* ctx, const double* dY_dev, const double* cov_dev, int64_t W, int64_t M, double* ll_dev);
// A chain's compacted batch whose every emulator takes the low-rank kernel (chain_batch, 1 < E <= MAX_LR_CTX of gpb_like.hip,
// fused finalize, one Wld): all E blocks added up in emuList order by one launch or two.  *taken = false: not such a chain,
// nothing launched.
int launch_loglike_lowrank_chain(gpb_ctx* const* ctxs, int E, int64_t W, double* ll_dev, const int* cmpv, double inside_const,
                                 bool* taken);
int ensure_lr_blocks(gpb_ctx* ctx, int E);          // its per-emulator blocks [E][Wcap] in the chain's first context
// ---- rows that belong to different data sets (gpb_chain_like_sets' tables; k_loglike_lowrank_sets) ---------------
constexpr int64_t MAX_LIKE_SETS = 65536;
// GPB_E_STATE (message on ctxs[0]) unless every emulator takes the low-rank kernel with the fused sums and the chain
// holds no coupled likelihood: what gpb_chain_like_sets and the calls that read its tables ask
int lowrank_sets_check(gpb_ctx* const* ctxs, int E, const char* who);
// step (3) of chain_rows for such a batch: row w is judged against data set cmpv[4 + w] / rows_per_set (< K, the tables' K)
int launch_loglike_lowrank_sets(gpb_ctx* const* ctxs, int E, int64_t W, int64_t rows_per_set, double* ll_dev, const int* cmpv,
                                double inside_const);
bool compaction_applies(const gpb_ctx* ctx);
// ---- a chain of emulators (gpb_chain.hip) ----------------------------------------------------------------
constexpr int MAX_CHAIN_CTX = 64;         // emulators of one chain: the context lists of the gpb_chain_* entry points
inline bool chain_args_ok(gpb_ctx* const* ctxs, int E) { return ctxs && E >= 1 && E <= MAX_CHAIN_CTX && ctxs[0]; }
// the chain's number of (original) parameters as context c sees it
inline int64_t sampler_ndim(const gpb_ctx* c) { return c->pmap_d_in > 0 ? c->pmap_d_in : c->d; }
// What every entry point that takes a chain asks of its contexts (after chain_args_ok): none null, one device and stream,
// one number of parameters, likelihood installed (need_like), a parameter map's output the GPs' input.  Sets ctxs[0]'s
// message to `who` + the reason.  chain_check: and the compacted chain call admits them (gpb_chain_supported answers 1).
int chain_ctx_check(gpb_ctx* const* ctxs, int E, const char* who, bool need_like = true);
int chain_check(gpb_ctx* const* ctxs, int E, const char* who);
// the compacted chain call of checked contexts.  premarked / cmpv: the caller's proposal kernel has taken the prior-box test
// (1) and gathered the rows inside (2) into ctxs[0]->cmp_X, their count and indices at cmpv (gpb_chain_emcee_run)
int chain_rows(gpb_ctx* const* ctxs, int E, const double* X_dev, int64_t W, double* ll_dev, const double* lo_dev,
               const double* hi_dev, double outside, double inside_const, int premarked = 0, const int* cmpv = nullptr);
// chain_rows with the last stage replaced: row w belongs to data set w / rows_per_set of the tables of gpb_chain_like_sets
// (checked by the caller: sets_check).  Same passes (1)-(2), then k_loglike_lowrank_sets.
int chain_rows_sets(gpb_ctx* const* ctxs, int E, const double* X_dev, int64_t W, int64_t rows_per_set, double* ll_dev,
                    const double* lo_dev, const double* hi_dev, double outside, double inside_const, int premarked = 0,
                    const int* cmpv = nullptr);
// what gpb_chain_logpost_sets and gpb_chain_emcee_sets_run ask before they launch: a chain (chain_check) whose every emulator
// holds tables of the same K >= nsets (GPB_E_STATE without tables, GPB_E_ARG beyond them)
int sets_check(gpb_ctx* const* ctxs, int E, int64_t nsets, const char* who);
// The evaluation of the resident samplers and the gradient: lp of the rows X [W, ndim] of checked contexts on the selected
// device, what Chain.log_prob_device writes: gpb_chain_logpost where gpb_chain_supported answers 1, else the per-emulator
// sequence of gpb_param_map / gpb_loglike / gpb_box_finish / gpb_logpost
int chain_eval(gpb_ctx* const* ctxs, int E, const double* X, int64_t W, double* lp, const double* lo, const double* hi,
               double outside, double inside_const);
// ---- a chain whose experimental covariance couples its emulators (gpb_coupled.hip) -------------------------
inline bool coupling_installed(const gpb_ctx* c0) { return c0->cpl.on; }
// GPB_E_STATE (message on ctxs[0]) when ctxs[0] holds a coupling that is stale or was set for another list of contexts
int coupling_check(gpb_ctx* const* ctxs, int E, const char* who);
// step (3) of chain_rows for a coupled chain, from the emulators' finalised mean_pc / var_pc: ll[cmp[4 + w]] = r + inside_const
int launch_loglike_coupled(gpb_ctx* const* ctxs, int E, int64_t W, double* ll_dev, const int* cmpv, double inside_const);
// the gradient's weights of all W rows: -t and 1/2 t^2 - 1/2 diag(R^T S^-1 R) into the emulators' wmu / wv [W][P_e]
int launch_like_w_coupled(gpb_ctx* const* ctxs, int E, int64_t W, double* const* wmu, double* const* wv);
// test hooks
int launch_test_gemm(gpb_ctx* ctx, int64_t M, int64_t N, int64_t K, const double* A, const double* B,
                     double* C, int b_trans);
int launch_probe(gpb_ctx* ctx, int mode, double* tflops);
}  // namespace gpb
