// ws_carve_check.cpp — stand-alone host check of the buffer carver (csrc/ws_carve.h) and of every workspace layout built on it
// (csrc/ws_layout.h).  For each layout at two shapes: the counting pass and the carving pass report the same total; on a malloc
// of exactly that many bytes every element of every piece is written with the piece's tag and read back (the sanitizer watches
// the bounds, the tags an overlap); every offset equals the expression the entry points used before the layouts existed,
// written out here as independent arithmetic.  Built with the address and undefined-behaviour sanitizers by
// tests/test_ws_carve_host.py; exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <vector>
#include "../../gpbayestools_hic_amd/csrc/ws_carve.h"
#include "../../gpbayestools_hic_amd/csrc/ws_layout.h"

using namespace gpb;

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++g_failed; } \
    } while (0)

struct Piece {
    const char* name;
    const void* p;
    int64_t bytes;              // what the consumer may touch
    int64_t offset;             // expected, in bytes from the base; -1: the piece must be null
};

static int64_t ru(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// lay: the layout over a carver; pieces: what it left, with the expected offsets; total: expected, in elements of B
template <typename B>
static void check_layout(const char* what, const std::function<void(Carver<B>&)>& lay, const std::function<std::vector<Piece>()>& pieces,
                         int64_t total) {
    Carver<B> count;
    lay(count);
    for (const Piece& q : pieces())
        if (q.p) { fprintf(stderr, "%s: %s is not null after the counting pass\n", what, q.name); ++g_failed; }
    if (count.total() != total) {
        fprintf(stderr, "%s: total %lld, expected %lld\n", what, (long long)count.total(), (long long)total);
        ++g_failed;
    }
    const size_t bytes = sizeof(B) * (size_t)count.total();
    unsigned char* mem = static_cast<unsigned char*>(malloc(bytes ? bytes : 1));
    Carver<B> real(reinterpret_cast<B*>(mem));
    lay(real);
    if (real.total() != count.total()) { fprintf(stderr, "%s: the carving pass reports another total\n", what); ++g_failed; }
    const std::vector<Piece> pc = pieces();
    for (size_t i = 0; i < pc.size(); ++i) {
        const Piece& q = pc[i];
        if (q.offset < 0) {
            if (q.p) { fprintf(stderr, "%s: %s should be null\n", what, q.name); ++g_failed; }
            continue;
        }
        const int64_t off = static_cast<const unsigned char*>(q.p) - mem;
        if (!q.p || off != q.offset) {
            fprintf(stderr, "%s: %s at byte %lld, expected %lld\n", what, q.name, q.p ? (long long)off : -1LL, (long long)q.offset);
            ++g_failed;
            continue;
        }
        memset(const_cast<void*>(q.p), (int)(i + 1), (size_t)q.bytes);      // (past the end: the sanitizer stops the program)
    }
    for (size_t i = 0; i < pc.size(); ++i) {
        const Piece& q = pc[i];
        if (q.offset < 0 || !q.p) continue;
        const unsigned char* b = static_cast<const unsigned char*>(q.p);
        for (int64_t k = 0; k < q.bytes; ++k)
            if (b[k] != (unsigned char)(i + 1)) {
                fprintf(stderr, "%s: %s overlaps another piece at byte %lld\n", what, q.name, (long long)k);
                ++g_failed;
                break;
            }
    }
    free(mem);
}

static void check_carver() {
    Carver<double> c;                                   // counting: null pieces, sizes add up
    CHECK(c.take<double>(3) == nullptr && c.total() == 3);
    CHECK(c.take<double>(0) == nullptr && c.total() == 3);            // nothing asked: null, no size
    CHECK(c.take<double>(0, 32) == nullptr && c.total() == 3);        // ... whatever the granule
    CHECK(c.take<double>(5, 32) == nullptr && c.total() == 35);       // rounded up to the granule
    CHECK(c.take<double>(64, 32) == nullptr && c.total() == 99);      // a multiple stays
    CHECK(c.take<int>(3) == nullptr && c.total() == 101);             // 12 bytes: two doubles
    CHECK(c.take<unsigned char>(17) == nullptr && c.total() == 104);  // 17 bytes: three
    CHECK(c.take<int>(1, 2) == nullptr && c.total() == 106);          // one int, then the granule
    double buf[16];
    Carver<double> r(buf);
    CHECK(r.take<double>(0) == nullptr);
    int* a = r.take<int>(3);
    CHECK((void*)a == (void*)buf && r.total() == 2);
    unsigned char* b = r.take<unsigned char>(9, 4);
    CHECK((void*)b == (void*)(buf + 2) && r.total() == 6);
    double* d = r.take<double>(10);
    CHECK(d == buf + 6 && r.total() == 16);
    Carver<int> ci;                                     // a 4-byte base: doubles take two, the granule counts ints
    CHECK(ci.take<int>(3, 2) == nullptr && ci.total() == 4);
    CHECK(ci.take<double>(3) == nullptr && ci.total() == 10);
    Carver<int64_t> c8;                                 // mixed element types on an 8-byte base
    CHECK(c8.take<double>(2) == nullptr && c8.take<int>(2 * 3) == nullptr && c8.total() == 5);
    CHECK(c8.take<unsigned char>(8) == nullptr && c8.total() == 6 && c8.take<unsigned char>(9) == nullptr && c8.total() == 8);
}

#define D8(n) ((int64_t)8 * (n))

static void check_mc(int64_t nh, int64_t d) {
    McWs w;
    check_layout<double>("mc_ws", [&](Carver<double>& c) { w.lay(c, nh, d); }, [&] {
        return std::vector<Piece>{{"q0", w.q[0], D8(nh * d), 0}, {"factor0", w.factor[0], D8(nh), D8(nh * d)},
                                  {"lpq0", w.lpq[0], D8(nh), D8(nh * d + nh)}, {"q1", w.q[1], D8(nh * d), D8(nh * (d + 2))},
                                  {"factor1", w.factor[1], D8(nh), D8(nh * (d + 2) + nh * d)},
                                  {"lpq1", w.lpq[1], D8(nh), D8(nh * (d + 2) + nh * d + nh)},
                                  {"lp2", w.lp2, D8(2 * nh), D8(2 * nh * (d + 2))}};
    }, 2 * nh * (d + 3));
    CHECK(w.n_sets == 2 * nh * (d + 2));
}

static void check_bal(int64_t nh, int64_t chunk) {
    BalWs w;
    const int64_t total = 4 * nh + 2 * (4 + chunk) + 16;
    check_layout<int>("bal_ws", [&](Carver<int>& c) { w.lay(c, nh, chunk); }, [&] {
        std::vector<Piece> v;
        for (int b = 0; b < 2; ++b) {
            v.push_back({"flags", w.flags[b], 4 * nh, 4 * (b * nh)});
            v.push_back({"rank", w.rank[b], 4 * nh, 4 * (2 * nh + b * nh)});
            v.push_back({"cmp", w.cmp[b], 4 * (4 + chunk), 4 * (4 * nh + b * (4 + chunk))});
            v.push_back({"meta", w.meta[b], 4 * 4, 4 * (4 * nh + 2 * (4 + chunk) + 4 * b)});
        }
        return v;
    }, total);
    CHECK(w.n == total);
}

static void check_ptl(int64_t T, int64_t nd) {
    PtlWs w;
    // (the accept flags took a double each before: 5 T nd + 3 T)
    check_layout<double>("ptl_ws", [&](Carver<double>& c) { w.lay(c, T, nd); }, [&] {
        return std::vector<Piece>{{"rvalo", w.rvalo, D8(T * nd), 0}, {"thetap", w.thetap, D8(T * nd), D8(T * nd)},
                                  {"grad", w.grad, D8(T * nd), D8(2 * T * nd)}, {"thetaB", w.thetaB, D8(T * nd), D8(3 * T * nd)},
                                  {"dfvalB", w.dfvalB, D8(T * nd), D8(4 * T * nd)}, {"lp", w.lp, D8(T), D8(5 * T * nd)},
                                  {"fvalB", w.fvalB, D8(T), D8(5 * T * nd + T)}, {"acc", w.acc, 4 * T, D8(5 * T * nd + 2 * T)}};
    }, 5 * T * nd + 2 * T + (T + 1) / 2);
}

static void check_smc(int64_t N, int64_t nd) {
    SmcWs w;
    check_layout<double>("smc_ws", [&](Carver<double>& c) { w.lay(c, N, nd); }, [&] {
        return std::vector<Piece>{{"wgt", w.wgt, D8(N), 0}, {"cum", w.cum, D8(N), D8(N)}, {"lp", w.lp, D8(N), D8(2 * N)},
                                  {"xp", w.xp, D8(N * nd), D8(3 * N)}, {"cov", w.cov, D8(nd * nd), D8(3 * N + N * nd)},
                                  {"mean", w.mean, D8(nd), D8(3 * N + N * nd + nd * nd)}};
    }, 3 * N + N * nd + nd * nd + nd);
}

static void check_design(int64_t C, int64_t R, int64_t d, int64_t P, int64_t Np) {
    DesignWs w;
    const int64_t Cp = ru(C, 128), Rp = ru(R, 128);
    const int64_t xr = ru(C * d, 2), ww = xr + ru(R * d, 2), g = ww + Rp, dg = g + ru(P, 2), vc = dg + P * Cp, vr = vc + P * Np * Cp,
                  s = vr + P * Np * Rp, sc = s + P * Rp * Cp;
    check_layout<double>("design_ws", [&](Carver<double>& c) { w.lay(c, C, R, d, P, Np); }, [&] {
        return std::vector<Piece>{{"xc", w.xc, D8(C * d), 0}, {"xr", w.xr, D8(R * d), D8(xr)}, {"w", w.w, D8(Rp), D8(ww)},
                                  {"g", w.g, D8(P), D8(g)}, {"dg", w.dg, D8(P * Cp), D8(dg)}, {"vc", w.vc, D8(P * Np * Cp), D8(vc)},
                                  {"vr", w.vr, D8(P * Np * Rp), D8(vr)}, {"s", w.s, D8(P * Rp * Cp), D8(s)},
                                  {"sc", w.sc, D8(P * Cp), D8(sc)}};
    }, sc + P * Cp);
    CHECK(w.Cp == Cp && w.Rp == Rp);
}

static void check_design_run(int64_t T, int64_t P, int64_t C, int64_t R, bool first) {
    DesignRun w;
    const int64_t Cp = ru(C, 128), Rp = ru(R, 128), nch = Rp / 64;
    const int64_t nU = T * P * Cp, nur = P * Rp, npart = P * nch * Cp, nden = ru(P, 2);
    check_layout<double>("design_run", [&](Carver<double>& c) { w.lay(c, T, P, Cp, Rp, nch, first); }, [&] {
        return std::vector<Piece>{{"U", w.U, D8(nU), 0}, {"ur", w.ur, D8(nur), D8(nU)}, {"part", w.part, D8(npart), D8(nU + nur)},
                                  {"J", w.J, D8(Cp), D8(nU + nur + npart)}, {"den", w.den, D8(P), D8(nU + nur + npart + Cp)},
                                  {"pick", w.pick, 4, first ? D8(nU + nur + npart + Cp + nden) : -1},
                                  {"elig", w.elig, Cp, first ? D8(nU + nur + npart + Cp + nden + 2) : -1}};
    }, nU + nur + npart + Cp + nden + (first ? 2 + Cp / 8 : 0));
}

static void check_diag_stage(int64_t n_rho, int64_t d) {
    DiagStage w;
    // (the two int vectors took a double per element before: n_rho + 7 d)
    check_layout<double>("diag stage", [&](Carver<double>& c) { w.lay(c, n_rho, d); }, [&] {
        return std::vector<Piece>{{"rho", w.rho, D8(n_rho), n_rho ? 0 : -1}, {"tau", w.tau, D8(d), D8(n_rho)},
                                  {"moments", w.moments, D8(3 * d), D8(n_rho + d)}, {"rhat", w.rhat, D8(d), D8(n_rho + 4 * d)},
                                  {"window", w.window, 4 * d, D8(n_rho + 5 * d)}, {"nconst", w.nconst, 4 * d, D8(n_rho + 5 * d) + 4 * d}};
    }, n_rho + 6 * d);
}

static void check_diag_ws(int64_t G, int64_t nsp, int64_t nwp, int64_t nband) {
    DiagWs w;
    const int64_t nstats = 6;
    check_layout<double>("diag_ws", [&](Carver<double>& c) { w.lay(c, G, nsp, nwp, nband, nstats); }, [&] {
        return std::vector<Piece>{{"Y", w.Y, D8(G * nsp * nwp), 0}, {"part", w.part, D8(G * nband * 128), D8(G * nsp * nwp)},
                                  {"stats", w.stats, D8(G * nwp * nstats), D8(G * nsp * nwp + G * nband * 128)}};
    }, (nsp * nwp + nband * 128 + nwp * nstats) * G);
}

static void check_marg(int64_t d, int64_t B, int64_t npairs, int64_t Sg, bool weights) {
    MargWs w;
    const int64_t n_edges = d * (B + 1), n_h1 = d * B, n_h2 = npairs * B * B, n_qw = weights ? Sg : 0,
                  n_codes = npairs ? (Sg * d + 7) / 8 : 0;
    check_layout<int64_t>("marg_ws", [&](Carver<int64_t>& c) { w.lay(c, n_edges, n_h1, d, n_h2, npairs, n_qw, npairs ? Sg * d : 0); }, [&] {
        return std::vector<Piece>{{"edges", w.edges, D8(n_edges), 0}, {"h1", w.h1, D8(n_h1), D8(n_edges)},
                                  {"out", w.out, D8(d), D8(n_edges + n_h1)}, {"h2", w.h2, D8(n_h2), npairs ? D8(n_edges + n_h1 + d) : -1},
                                  {"pairs", w.pairs, 4 * 2 * npairs, npairs ? D8(n_edges + n_h1 + d + n_h2) : -1},
                                  {"qw", w.qw, D8(n_qw), weights ? D8(n_edges + n_h1 + d + n_h2 + npairs) : -1},
                                  {"codes", w.codes, npairs ? Sg * d : 0, npairs ? D8(n_edges + n_h1 + d + n_h2 + npairs + n_qw) : -1}};
    }, n_edges + n_h1 + d + n_h2 + npairs + n_qw + n_codes);
}

static void check_sl_scale(int64_t P, int64_t Np128) {
    SlScale w;
    check_layout<double>("sl_scale", [&](Carver<double>& c) { w.lay(c, P, Np128); }, [&] {
        return std::vector<Piece>{{"rowscale", w.rowscale, D8(P * Np128), 0}, {"colscale", w.colscale, D8(P), D8(P * Np128)},
                                  {"rowexp", w.rowexp, 4 * P * Np128, D8(P * Np128 + P)}};
    }, P * Np128 + P + (P * Np128 + 1) / 2);
}

static void check_cv(int64_t n_idx, int64_t nf, bool has_idx, bool loo, int64_t P, int64_t Np) {
    CvWs w;
    const int64_t ints = ru(has_idx ? n_idx + nf + 1 : 0, 2), nI = Np / 64;
    check_layout<int>("cv_ws", [&](Carver<int>& c) { w.lay(c, has_idx ? n_idx + nf + 1 : 0, loo ? P * nI * Np : 0); }, [&] {
        return std::vector<Piece>{{"folds", w.folds, 4 * (n_idx + nf + 1), has_idx ? 0 : -1},
                                  {"part", w.part, D8(P * nI * Np), loo ? 4 * ints : -1}};
    }, ints + (loo ? 2 * P * nI * Np : 0));
}

static void check_sobol(int64_t P, int64_t N, int64_t dpad, int64_t Np, int64_t d, bool with_part) {
    SobolWs w;
    const int64_t nB = Np / 64, tab = 2 * P * N * dpad + P * nB, np = with_part ? P * (P + 1) / 2 * nB * nB * (2 * d + 1) : 0;
    check_layout<double>("sobol_ws", [&](Carver<double>& c) { w.lay(c, P, N, dpad, nB, np); }, [&] {
        return std::vector<Piece>{{"Itab", w.Itab, D8(P * N * dpad), 0}, {"Etab", w.Etab, D8(P * N * dpad), D8(P * N * dpad)},
                                  {"epart", w.epart, D8(P * nB), D8(2 * P * N * dpad)}, {"part", w.part, D8(np), with_part ? D8(tab) : -1}};
    }, tab + np);
}

static void check_grad(bool need_beta, int64_t P, int64_t W, int64_t Np, int64_t d, int64_t din, bool mapped, int64_t lw, int64_t n_out) {
    GradWs w;
    const int64_t Wld = ru(W, 128);
    const int64_t sz[10] = {need_beta ? P * Wld * Np : 0, W * P * d, need_beta ? W * P * d : 0, W * P, W * P, W * d,
                            mapped ? W * d * din : 0, lw, W * (din > d ? din : d), n_out};
    int64_t off[11] = {0};
    for (int i = 0; i < 10; ++i) off[i + 1] = off[i] + ru(sz[i], 32);
    check_layout<double>("gbuf", [&](Carver<double>& c) { w.lay(c, need_beta, P, Wld, Np, W, d, din, mapped, lw, n_out); }, [&] {
        const double* p[10] = {w.bt, w.dm, w.dv, w.wmu, w.wv, w.xg, w.jm, w.lw, w.xin, w.out};
        const char* nm[10] = {"bt", "dm", "dv", "wmu", "wv", "xg", "jm", "lw", "xin", "out"};
        std::vector<Piece> v;
        for (int i = 0; i < 10; ++i) v.push_back({nm[i], p[i], D8(sz[i]), sz[i] ? D8(off[i]) : -1});
        return v;
    }, off[10]);
}

int main() {
    check_carver();
    // the smallest shapes
    check_mc(1, 1);
    check_bal(1, 1);
    check_ptl(2, 1);
    check_smc(2, 1);
    check_design(1, 1, 1, 1, 64);
    check_design_run(1, 1, 1, 1, true);
    check_diag_stage(0, 1);
    check_diag_ws(1, 64, 16, 1);
    check_marg(1, 1, 0, 1, false);
    check_sl_scale(1, 128);
    check_cv(2, 2, false, true, 1, 64);
    check_sobol(1, 2, 8, 64, 1, false);
    check_grad(false, 1, 1, 64, 1, 1, false, 0, 0);
    // odd ones
    check_mc(9, 5);
    check_bal(9, 3);
    check_ptl(7, 5);
    check_smc(37, 5);
    check_design(40, 30, 3, 3, 128);
    check_design_run(4, 3, 40, 30, true);
    check_design_run(4, 3, 40, 30, false);
    check_diag_stage(3 * 6, 3);
    check_diag_stage(5 * 8, 5);
    check_diag_ws(3, 128, 16, 5);
    check_marg(3, 5, 3, 37, true);
    check_marg(5, 7, 10, 33, false);
    check_sl_scale(3, 384);
    check_cv(7, 3, true, false, 3, 128);
    check_cv(5, 5, true, true, 3, 128);
    check_sobol(3, 37, 8, 128, 3, true);
    check_grad(true, 3, 7, 128, 3, 5, true, 7 * 41, 2 * 7 * 3 * 3);
    check_grad(false, 3, 7, 128, 3, 3, false, 0, 7 * 4 * 3);
    if (g_failed) return 1;
    puts("ws_carve_check: ok");
    return 0;
}
