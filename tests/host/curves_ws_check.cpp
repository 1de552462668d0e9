// curves_ws_check.cpp — stand-alone host check of gpb_chain_curves' workspace layout (CurvesWs, csrc/ws_layout.h), in the manner of
// kmeans_ws_check.cpp: the counting pass and the carving pass report the same total; on a malloc of exactly that many bytes every
// byte of every piece is written with the piece's tag and read back (the sanitizer watches the bounds, the tags an overlap); the
// total does not depend on a number of samples — the layout takes none.  Built with the address and undefined-behaviour
// sanitizers by tests/test_curves_ws_host.py; exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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
    void* p;
    int64_t bytes;
};

static void check(int64_t ncurves, int64_t G, int64_t nq, int64_t d2) {
    const int64_t R = ncurves * G, nr = 2 * nq;
    CurvesWs count;
    Carver<int64_t> c0;
    count.lay(c0, ncurves, R, nr, d2);
    CHECK(count.grid == nullptr && count.hist == nullptr && count.desc == nullptr);
    const size_t bytes = 8 * (size_t)c0.total();
    unsigned char* mem = static_cast<unsigned char*>(malloc(bytes));
    CurvesWs w;
    Carver<int64_t> c1(reinterpret_cast<int64_t*>(mem));
    w.lay(c1, ncurves, R, nr, d2);
    CHECK(c1.total() == c0.total());
    std::vector<Piece> pc = {{"grid", w.grid, 8 * R}, {"desc", w.desc, 4 * 5 * ncurves}};
    if (d2) pc.push_back({"aux", w.aux, 8 * d2});
    else CHECK(!w.aux);
    if (nr) {                                           // (a values-only call has no ranks: none of the select's pieces)
        pc.push_back({"prefix", w.prefix, 8 * R * nr});
        pc.push_back({"gprefix", w.gprefix, 8 * R * nr});
        pc.push_back({"rem", w.rem, 8 * R * nr});
        pc.push_back({"hist", w.hist, 4 * R * nr * 256});
        pc.push_back({"grp", w.grp, 4 * R * nr});
        pc.push_back({"ngrp", w.ngrp, 4 * R});
    } else {
        CHECK(!w.prefix && !w.gprefix && !w.rem && !w.hist && !w.grp);
        pc.push_back({"ngrp", w.ngrp, 4 * R});
    }
    for (size_t i = 0; i < pc.size(); ++i) {
        CHECK(pc[i].p != nullptr);
        if (!pc[i].p) continue;
        memset(pc[i].p, (int)(i + 1), (size_t)pc[i].bytes);                      // (past the end: the sanitizer stops the program)
    }
    for (size_t i = 0; i < pc.size(); ++i) {
        if (!pc[i].p) continue;
        const unsigned char* b = static_cast<const unsigned char*>(pc[i].p);
        for (int64_t t = 0; t < pc[i].bytes; ++t)
            if (b[t] != (unsigned char)(i + 1)) {
                fprintf(stderr, "%s overlaps another piece at byte %lld\n", pc[i].name, (long long)t);
                ++g_failed;
                break;
            }
    }
    free(mem);
}

int main() {
    check(1, 1, 1, 0);
    check(1, 1, 0, 2);
    check(3, 100, 7, 0);
    check(4, 129, 16, 40);
    check(8, 1024, 1, 10);
    check(3, 7, 0, 0);
    check(5, 33, 3, 6);
    if (g_failed) return 1;
    puts("curves_ws_check: ok");
    return 0;
}
