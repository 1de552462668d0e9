// ws_layout.h — what lies inside every context buffer that holds more than one piece: one struct of pointers per workspace and
// the list of take() calls that places them (ws_carve.h).  Functions of plain integers, so tests/host/ws_carve_check.cpp runs
// every one of them on the host.  The entry points size the buffers through ctx_carve (gpb_internal.h) with these lists and read
// the pieces from the structs: no offset is written down a second time.
#pragma once
#include "ws_carve.h"

namespace gpb {

constexpr int64_t WS_PAD = 128;         // walker-batch padding granule (WPAD of gpb_internal.h)
inline int64_t ws_round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// mc_ws (gpb_chain_emcee_run): two sets of proposals q [nh][d], stretch factors [nh] and their log-probabilities [nh] (the
// fused accept + proposal kernel reads one set and writes the other), then a second log-probability vector [2 nh]
struct McWs {
    double *q[2], *factor[2], *lpq[2], *lp2;
    int64_t n_sets;                 // doubles of the two sets in front of lp2
    void lay(Carver<double>& c, int64_t nh, int64_t d) {
        for (int b = 0; b < 2; ++b) {
            q[b] = c.take<double>(nh * d);
            factor[b] = c.take<double>(nh);
            lpq[b] = c.take<double>(nh);
        }
        n_sets = c.total();
        lp2 = c.take<double>(2 * nh);
    }
};

// bal_ws (balanced shards of gpb_chain_emcee_run), per buffer set: the flags and ranks of all nh rows, this rank's counter +
// index list [4 + chunk], four ints of slice bounds (room for four sets of them)
struct BalWs {
    int *flags[2], *rank[2], *cmp[2], *meta[2];
    int64_t n;                      // ints in all
    void lay(Carver<int>& c, int64_t nh, int64_t chunk) {
        for (int b = 0; b < 2; ++b) flags[b] = c.take<int>(nh);
        for (int b = 0; b < 2; ++b) rank[b] = c.take<int>(nh);
        for (int b = 0; b < 2; ++b) cmp[b] = c.take<int>(4 + chunk);
        meta[0] = c.take<int>(16);
        meta[1] = meta[0] ? meta[0] + 4 : nullptr;
        n = c.total();
    }
};

// ptl_ws (gpb_chain_ptlmc_run): draws, proposals, their gradient, the other theta / dfval buffers [T][nd] each; the proposals'
// lp and the other fval [T] each; the accept flags [T] (int)
struct PtlWs {
    double *rvalo, *thetap, *grad, *thetaB, *dfvalB, *lp, *fvalB;
    int* acc;
    void lay(Carver<double>& c, int64_t T, int64_t nd) {
        rvalo = c.take<double>(T * nd);
        thetap = c.take<double>(T * nd);
        grad = c.take<double>(T * nd);
        thetaB = c.take<double>(T * nd);
        dfvalB = c.take<double>(T * nd);
        lp = c.take<double>(T);
        fvalB = c.take<double>(T);
        acc = c.take<int>(T);
    }
};

// hmc_ws (gpb_chain_hmc_run): the trajectory's momenta, positions and gradient [C][nd] each; its lp and the start's energy H0
// [C] each; the step size of the step (eps, eps / 2); the escape flags [C] (int)
struct HmcWs {
    double *p, *xt, *gt, *lpt, *h0, *eps;
    int* esc;
    void lay(Carver<double>& c, int64_t C, int64_t nd) {
        p = c.take<double>(C * nd);
        xt = c.take<double>(C * nd);
        gt = c.take<double>(C * nd);
        lpt = c.take<double>(C);
        h0 = c.take<double>(C);
        eps = c.take<double>(2);
        esc = c.take<int>(C);
    }
};

// smc_ws (gpb_chain_smc_*): weights, their scan, log-probabilities [N] each; one particle buffer [N][nd] (the gathered rows of
// a reweighting — with their log-likelihoods in lp —, the proposals of a move step); cov [nd][nd]; mean [nd]
struct SmcWs {
    double *wgt, *cum, *lp, *xp, *cov, *mean;
    void lay(Carver<double>& c, int64_t N, int64_t nd) {
        wgt = c.take<double>(N);
        cum = c.take<double>(N);
        lp = c.take<double>(N);
        xp = c.take<double>(N * nd);
        cov = c.take<double>(nd * nd);
        mean = c.take<double>(nd);
    }
};

// design_ws (gpb_design_begin's block): x_c [C][d] | x_r [R][d] | w [Rp] | g [P] | s(c,c) [P][Cp] | V_c [P][Np][Cp] |
// V_r [P][Np][Rp] | S_rc [P][Rp][Cp] | the candidates' simulation noise [P][Cp] (Cp, Rp: C, R padded to 128).  Every part
// starts on an even offset: the GEMM's operands are read two at a time.
struct DesignWs {
    int64_t Cp, Rp;
    double *xc, *xr, *w, *g, *dg, *vc, *vr, *s, *sc;
    void lay(Carver<double>& c, int64_t C, int64_t R, int64_t d, int64_t P, int64_t Np) {
        Cp = ws_round_up(C, WS_PAD);
        Rp = ws_round_up(R, WS_PAD);
        xc = c.take<double>(C * d, 2);
        xr = c.take<double>(R * d, 2);
        w = c.take<double>(Rp);
        g = c.take<double>(P, 2);
        dg = c.take<double>(P * Cp);
        vc = c.take<double>(P * Np * Cp);
        vr = c.take<double>(P * Np * Rp);
        s = c.take<double>(P * Rp * Cp);
        sc = c.take<double>(P * Cp);
    }
};

// design_run (gpb_chain_design_run), per context: the picks' scaled rows U [T][P][Cp] | the pending u_r [P][Rp] | chunk
// partials [P][nch][Cp] | scores J [Cp] | denominators [P]; the chain's first context also the pick (int) and the eligibility
// flags [Cp] (bytes) of a run that was given none
struct DesignRun {
    double *U, *ur, *part, *J, *den;
    int* pick;
    uint8_t* elig;
    void lay(Carver<double>& c, int64_t T, int64_t P, int64_t Cp, int64_t Rp, int64_t nch, bool first) {
        U = c.take<double>(T * P * Cp);
        ur = c.take<double>(P * Rp);
        part = c.take<double>(P * nch * Cp);
        J = c.take<double>(Cp);
        den = c.take<double>(P, 2);
        pick = c.take<int>(first ? 1 : 0, 2);
        elig = c.take<uint8_t>(first ? Cp : 0);
    }
};

// gpb_mcmc_diag's results in out_stage: rho [d][max_lag + 1] (n_rho doubles, 0 without the autocorrelation) | tau [d] |
// moments [d][3] | rhat [d] | window [d] | nconst [d] (int, back to back)
struct DiagStage {
    double *rho, *tau, *moments, *rhat;
    int *window, *nconst;
    void lay(Carver<double>& c, int64_t n_rho, int64_t d) {
        rho = c.take<double>(n_rho);
        tau = c.take<double>(d);
        moments = c.take<double>(3 * d);
        rhat = c.take<double>(d);
        window = c.take<int>(2 * d);
        nconst = window ? window + d : nullptr;
    }
};

// diag_ws (launch_mcmc_diag), G parameters at a time: Y [G][nsp][nwp] | lag partials [G][nband][128] | walker statistics
// [G][nwp][nstats]
struct DiagWs {
    double *Y, *part, *stats;
    void lay(Carver<double>& c, int64_t G, int64_t nsp, int64_t nwp, int64_t nband, int64_t nstats) {
        Y = c.take<double>(G * nsp * nwp);
        part = c.take<double>(G * nband * 128);
        stats = c.take<double>(G * nwp * nstats);
    }
};

// gpb_chain_rank_diag's results in out_stage, 8-byte units: median [d] | quant [d][nq] | rhat [d][2] | ess [d][K] | sd [d] | stop
// [d][K] (int) | rank2 [d][n] (int64; n_rank2 = 0 unless asked for)
struct RankStage {
    double *median, *quant, *rhat, *ess, *sd;
    int* stop;
    int64_t* rank2;
    void lay(Carver<double>& c, int64_t d, int64_t nq, int64_t n_rank2) {
        const int64_t K = 2 + nq;
        median = c.take<double>(d);
        quant = c.take<double>(d * nq);
        rhat = c.take<double>(2 * d);
        ess = c.take<double>(d * K);
        sd = c.take<double>(d);
        stop = c.take<int>(d * K);
        rank2 = c.take<int64_t>(n_rank2);
    }
};

// rank_ws (launch_rank_diag), 8-byte units.  One parameter's sort: keys [2][n] (u64) and positions [2][n] (u32), ping and pong |
// per sort block the digit counts, then offsets [nsb][256] (u32) | the digits' bases [256] (u32) | the plan of the eight passes
// [32] (u32: the OR of key differences in [0..1], skipped [8 + p], source buffer [16 + p]) | 2 r of the values and of the folded
// values in (step, walker) order [n] each (u32).  Then G parameters at a time: Y [G][K][hp][mp] | lag partials [G][K][nband][128]
// | A(t) [G][K][L + 1] | the scan's R [G][K][L + 3] | per split chain (mean, variance) [G][K + 1][mp][2] | per series (W, variance
// of the chain means) [G][K + 1][2]
struct RankWs {
    uint64_t* keys[2];
    unsigned *pos[2], *counts, *base, *plan, *r2b, *r2f;
    double *Y, *part, *acov, *R, *cstat, *mom;
    int64_t n_sort;                 // units of the sort's pieces in front of Y
    void lay(Carver<int64_t>& c, int64_t n, int64_t nsb, int64_t G, int64_t K, int64_t hp, int64_t mp, int64_t nband, int64_t L) {
        for (int b = 0; b < 2; ++b) keys[b] = c.take<uint64_t>(n);
        for (int b = 0; b < 2; ++b) pos[b] = c.take<unsigned>(n);
        counts = c.take<unsigned>(nsb * 256);
        base = c.take<unsigned>(256);
        plan = c.take<unsigned>(32);
        r2b = c.take<unsigned>(n);
        r2f = c.take<unsigned>(n);
        n_sort = c.total();
        Y = c.take<double>(G * K * hp * mp);
        part = c.take<double>(G * K * nband * 128);
        acov = c.take<double>(G * K * (L + 1));
        R = c.take<double>(G * K * (L + 3));
        cstat = c.take<double>(G * (K + 1) * mp * 2);
        mom = c.take<double>(G * (K + 1) * 2);
    }
};

// marg_ws (launch_chain_marginals), 8-byte units: edges | h1 | outside [d] | h2 | pairs [n_pairs][2] (int) | integer weights |
// one code byte per (sample, parameter) of a sample group.  h1 | outside | h2 are zeroed and copied out as one run of counts.
struct MargWs {
    double* edges;
    uint64_t *h1, *out, *h2, *qw;
    int* pairs;
    unsigned char* codes;
    void lay(Carver<int64_t>& c, int64_t n_edges, int64_t n_h1, int64_t d, int64_t n_h2, int64_t n_pairs, int64_t n_qw,
             int64_t n_code_bytes) {
        edges = c.take<double>(n_edges);
        h1 = c.take<uint64_t>(n_h1);
        out = c.take<uint64_t>(d);
        h2 = c.take<uint64_t>(n_h2);
        pairs = c.take<int>(2 * n_pairs);
        qw = c.take<uint64_t>(n_qw);
        codes = c.take<unsigned char>(n_code_bytes);
    }
};

// hm_ws (gpb_hm.hip), 8-byte units: the box lo [d] | hi [d] of gpb_hm_uniform, or gpb_hm_maps' edges [d][B + 1] | pairs
// [npairs][2] (int) | one code byte per (sample, parameter) of a sample group
struct HmWs {
    double *box, *edges;
    int* pairs;
    unsigned char* codes;
    void lay(Carver<int64_t>& c, int64_t n_box, int64_t n_edges, int64_t n_pairs, int64_t n_code_bytes) {
        box = c.take<double>(n_box);
        edges = c.take<double>(n_edges);
        pairs = c.take<int>(2 * n_pairs);
        codes = c.take<unsigned char>(n_code_bytes);
    }
};

// curves_ws (gpb_chain_curves), 8-byte units, R = ncurves G rows and nr = 2 nq ranks per row: grid [R] | aux [2 d] | per
// (row, rank) the digits found so far, the rank among the keys that share them and the distinct prefixes of the row's ranks
// [R][nr] each | the digit histograms [R][nr][256] (u32) | curve descriptors [ncurves][5], every rank's group [R][nr] and the
// groups per row [R] (int).  Nothing in it grows with the number of samples.  gpb_chain_trace_hist keeps its edges here.
struct CurvesWs {
    double *grid, *aux;
    uint64_t *prefix, *gprefix;
    int64_t* rem;
    unsigned* hist;
    int *desc, *grp, *ngrp;
    void lay(Carver<int64_t>& c, int64_t ncurves, int64_t R, int64_t nr, int64_t d2) {
        grid = c.take<double>(R);
        aux = c.take<double>(d2);
        prefix = c.take<uint64_t>(R * nr);
        gprefix = c.take<uint64_t>(R * nr);
        rem = c.take<int64_t>(R * nr);
        hist = c.take<unsigned>(R * nr * 256);
        desc = c.take<int>(ncurves * 5);
        grp = c.take<int>(R * nr);
        ngrp = c.take<int>(R);
    }
};

// kmeans_ws (gpb_chain_kmeans), 8-byte units.  A run that is zeroed at the start of a call (state0, state_bytes): counters [4] |
// centres [R][k][d] | shift [R] | integer sums acc [R][k][d], wq [R][k], cnt [R][k], iner [R] | seed rows [R][k] | changed, done,
// conv, niter, fi [R] each (int, back to back).  Behind it: mean | scale [2 d] | moment sums [5 d + 1] and their workgroup
// partials [nb][5 d + 1] | with seeding the uniforms [R][k], the range sums [R][nb], the chosen range [R] (int) and (sum in
// front, target) [R][2] | effective weights [S] | one label byte per (restart, row).
struct KmeansWs {
    int64_t *state0, state_bytes;
    int64_t *counters, *acc, *wq, *cnt, *iner, *seed;
    double *cen, *shift, *ms, *mom, *part, *u, *bs, *selv, *weff;
    int *changed, *done, *conv, *niter, *fi, *selb;
    unsigned char* lab;
    void lay(Carver<int64_t>& c, int64_t S, int64_t R, int64_t k, int64_t d, int64_t nb, int seeding) {
        const int64_t at0 = c.total();
        state0 = counters = c.take<int64_t>(4);
        cen = c.take<double>(R * k * d);
        shift = c.take<double>(R);
        acc = c.take<int64_t>(R * k * d);
        wq = c.take<int64_t>(R * k);
        cnt = c.take<int64_t>(R * k);
        iner = c.take<int64_t>(R);
        seed = c.take<int64_t>(R * k);
        changed = c.take<int>(5 * R);
        done = changed ? changed + R : nullptr;
        conv = changed ? changed + 2 * R : nullptr;
        niter = changed ? changed + 3 * R : nullptr;
        fi = changed ? changed + 4 * R : nullptr;
        state_bytes = 8 * (c.total() - at0);
        ms = c.take<double>(2 * d);
        mom = c.take<double>(5 * d + 1);
        part = c.take<double>(nb * (5 * d + 1));
        u = c.take<double>(seeding ? R * k : 0);
        bs = c.take<double>(seeding ? R * nb : 0);
        selb = c.take<int>(seeding ? R : 0);
        selv = c.take<double>(seeding ? 2 * R : 0);
        weff = c.take<double>(S);
        lab = c.take<unsigned char>(R * S);
    }
};

// knn_ws (gpb_chain_knn), 8-byte units, the sizes from knn_plan.h: counters [2] | inv_scale [dp] | the scaled rows of B (of A
// in self mode) [nZ][dp] | per slab of A: its scaled rows [slab][dp] (cross mode only) | the ranges' partial lists, r2 and idx
// [splits][slab][kp] each and zeros [splits][slab] | with staged results (a caller that wants host memory) r2, idx [slab][kmax]
// and zeros [slab]
struct KnnWs {
    int64_t* counters;
    double *inv, *zb, *za, *pr2, *fr2;
    int *pidx, *pzeros, *fidx, *fzeros;
    void lay(Carver<int64_t>& c, int64_t nZ, int64_t slab, int64_t dp, int64_t kp, int64_t kmax, int64_t splits, int cross,
             int staged) {
        counters = c.take<int64_t>(2);
        inv = c.take<double>(dp);
        zb = c.take<double>(nZ * dp);
        za = c.take<double>(cross ? slab * dp : 0);
        pr2 = c.take<double>(splits * slab * kp);
        pidx = c.take<int>(splits * slab * kp);
        pzeros = c.take<int>(splits * slab);
        fr2 = c.take<double>(staged ? slab * kmax : 0);
        fidx = c.take<int>(staged ? slab * kmax : 0);
        fzeros = c.take<int>(staged ? slab : 0);
    }
};

// eig_ws (gpb_eig_lse), doubles, every piece an even count (the panels are read two doubles at a time), the sizes from eig_plan.h:
// the centres c [M] | the inner panel (t, u) [2M][sin_p] | the outer panel (q, l) [2M][sout_p] | the bias [G][sin_p] | the ranges'
// partial maxima and sums [G][splits][sout_p] each | the groups' table [G][4] (int) | the count of bad outer indices (int) | with
// staged results (a caller that wants host memory) lse_excl and self [G][S_out] each
struct EigWs {
    double *cen, *bop, *aop, *bias, *pm, *ps, *flse, *fself;
    int *ranges, *bad;
    void lay(Carver<double>& c, int64_t M, int64_t S_out, int64_t sin_p, int64_t sout_p, int64_t G, int64_t splits, int staged) {
        cen = c.take<double>(M, 2);
        bop = c.take<double>(2 * M * sin_p, 2);
        aop = c.take<double>(2 * M * sout_p, 2);
        bias = c.take<double>(G * sin_p, 2);
        pm = c.take<double>(G * splits * sout_p, 2);
        ps = c.take<double>(G * splits * sout_p, 2);
        ranges = c.take<int>(4 * G, 2);
        bad = c.take<int>(2, 2);
        flse = c.take<double>(staged ? G * S_out : 0, 2);
        fself = c.take<double>(staged ? G * S_out : 0, 2);
    }
};

// maxpro_ws (gpb_maxpro.hip), 8-byte units: the pair matrices T [R][n][n] | row sums [R][n] | per restart (sum, best sum, start
// sum, sum of the best levels) [R][4] | (accepted, consumed) [R][2] | levels and best levels [R][d][n] each (int, a column
// contiguous) | the trace [R][n_trace] (int; none without a trace) | for a real design (R == 1): x [d][n], the scores [n] and the
// run order [n] (int)
struct MaxproWs {
    double *T, *rowsum, *sums, *x, *score;
    int64_t* counts;
    int *lev, *best, *trace, *order;
    void lay(Carver<int64_t>& c, int64_t n, int64_t d, int64_t R, int64_t n_trace, int real) {
        T = c.take<double>(R * n * n);
        rowsum = c.take<double>(R * n);
        sums = c.take<double>(R * 4);
        counts = c.take<int64_t>(R * 2);
        lev = c.take<int>(real ? 0 : R * d * n);
        best = c.take<int>(real ? 0 : R * d * n);
        trace = c.take<int>(real ? 0 : R * n_trace);
        x = c.take<double>(real ? d * n : 0);
        score = c.take<double>(real ? n : 0);
        order = c.take<int>(real ? n : 0);
    }
};

// sl_scale (gpb_sliced.hip): row scales [P][Np128] | column scales [P] | row exponents [P][Np128] (int)
struct SlScale {
    double *rowscale, *colscale;
    int* rowexp;
    void lay(Carver<double>& c, int64_t P, int64_t Np128) {
        rowscale = c.take<double>(P * Np128);
        colscale = c.take<double>(P);
        rowexp = c.take<int>(P * Np128);
    }
};

// cv_ws (gpb_cv.hip): the folds of the planned call, idx [n_idx] | fold_ptr [nf + 1] (n_folds ints in all, none for plain
// leave-one-out; padded to an even count: the doubles behind them stay aligned), then the leave-one-out path's partials
struct CvWs {
    int* folds;
    double* part;
    void lay(Carver<int>& c, int64_t n_folds, int64_t n_part) {
        folds = c.take<int>(n_folds, 2);
        part = c.take<double>(n_part);
    }
};

// the front of sobol_ws (gpb_sobol.hip): the I and E tables [P][N][dpad] each | e partials [P][nB] | launch_sobol's tile
// partials [P (P + 1) / 2][nB][nB][2d + 1] (n_part doubles; none for a call that only needs the tables).  What else a call needs
// (scratch, staged results) it carves behind these.
struct SobolWs {
    double *Itab, *Etab, *epart, *part;
    void lay(Carver<double>& c, int64_t P, int64_t N, int64_t dpad, int64_t nB, int64_t n_part) {
        Itab = c.take<double>(P * N * dpad);
        Etab = c.take<double>(P * N * dpad);
        epart = c.take<double>(P * nB);
        part = c.take<double>(n_part);
    }
};

// cpl_tab (gpb_coupled.hip): the joint tables of a coupled chain likelihood, R^T [PP][PP] (row p: column p of R, zero beyond
// the chain's PT GPs) | v0 [PP]
struct CoupledWs {
    double *RT, *v0;
    void lay(Carver<double>& c, int64_t PP) {
        RT = c.take<double>(PP * PP, 2);
        v0 = c.take<double>(PP, 2);
    }
};

// gbuf (gpb_grad.hip), the pieces of one gradient evaluation of W rows, 32 doubles the granule: beta^T [P][Wld][Np] | dmean,
// dvar [W][P][d] | the likelihood's weights of mean and variance [W][P] | mapped rows [W][d] | the map's Jacobian [W][d][din] |
// the likelihood's global scratch | staged input rows | staged results
struct GradWs {
    double *bt, *dm, *dv, *wmu, *wv, *xg, *jm, *lw, *xin, *out;
    void lay(Carver<double>& c, bool need_beta, int64_t P, int64_t Wld, int64_t Np, int64_t W, int64_t d, int64_t din, bool mapped,
             int64_t lw_doubles, int64_t n_out) {
        bt = c.take<double>(need_beta ? P * Wld * Np : 0, 32);
        dm = c.take<double>(W * P * d, 32);
        dv = c.take<double>(need_beta ? W * P * d : 0, 32);
        wmu = c.take<double>(W * P, 32);
        wv = c.take<double>(W * P, 32);
        xg = c.take<double>(W * d, 32);
        jm = c.take<double>(mapped ? W * d * din : 0, 32);
        lw = c.take<double>(lw_doubles, 32);
        xin = c.take<double>(W * (din > d ? din : d), 32);
        out = c.take<double>(n_out, 32);
    }
};

}  // namespace gpb
