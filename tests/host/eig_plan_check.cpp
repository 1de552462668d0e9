// eig_plan_check.cpp — stand-alone host check of gpb_eig_lse's plan (csrc/eig_plan.h) and workspace layout (EigWs,
// csrc/ws_layout.h), in the manner of knn_plan_check.cpp: over a grid of sizes the padded widths are whole tiles that cover the
// samples, the ranges of the inner axis cover every tile once and none is empty, the counting pass and the carving pass agree,
// every piece starts on a 16-byte boundary (the panels are read two doubles at a time), and on a malloc of exactly that many
// bytes every byte of every piece is written with the piece's tag and read back (overrun: the sanitizer; overlap: the tags).
// Built with the address and undefined-behaviour sanitizers by tests/test_eig_plan_host.py; exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../gpbayestools_hic_amd/csrc/eig_plan.h"
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

static EigPlan check_plan(int64_t S_out, int64_t S_in, int G, int splits, int num_cu) {
    const EigPlan p = eig_plan(S_out, S_in, G, splits, num_cu);
    CHECK(p.sout_p % EIG_TILE_OUT == 0 && p.sout_p >= S_out && p.sout_p - S_out < EIG_TILE_OUT);
    CHECK(p.sin_p % EIG_TILE_IN == 0 && p.sin_p >= S_in && p.sin_p - S_in < EIG_TILE_IN);
    CHECK(p.out_tiles * EIG_TILE_OUT == p.sout_p && p.in_tiles * EIG_TILE_IN == p.sin_p);
    CHECK(p.sout_p <= 0x7fffffffLL && p.sin_p <= 0x7fffffffLL);                       // (the kernels' int columns)
    CHECK(p.splits >= 1 && p.splits <= EIG_MAX_SPLITS && (splits == 0 || p.splits <= splits));
    CHECK(p.tiles_per_split >= 1);
    CHECK((int64_t)p.splits * p.tiles_per_split >= p.in_tiles);                       // the ranges cover the inner axis ...
    CHECK((int64_t)(p.splits - 1) * p.tiles_per_split < p.in_tiles);                  // ... and the last one is not empty
    return p;
}

static void check_layout(int64_t M, int64_t S_out, int64_t S_in, int G, int splits, int staged) {
    const EigPlan p = check_plan(S_out, S_in, G, splits, 256);
    EigWs count;
    Carver<double> c0;
    count.lay(c0, M, S_out, p.sin_p, p.sout_p, G, p.splits, staged);
    CHECK(count.cen == nullptr && count.bop == nullptr);
    const int64_t bytes = 8 * c0.total();
    // what the header promises: the two panels dominate
    CHECK(bytes >= 16 * M * (p.sin_p + p.sout_p));
    unsigned char* mem = static_cast<unsigned char*>(aligned_alloc(16, (size_t)((bytes + 15) / 16 * 16)));
    EigWs w;
    Carver<double> c1(reinterpret_cast<double*>(mem));
    w.lay(c1, M, S_out, p.sin_p, p.sout_p, G, p.splits, staged);
    CHECK(c1.total() == c0.total());
    std::vector<Piece> pc = {{"cen", w.cen, 8 * M},
                             {"bop", w.bop, 16 * M * p.sin_p},
                             {"aop", w.aop, 16 * M * p.sout_p},
                             {"bias", w.bias, 8 * G * p.sin_p},
                             {"pm", w.pm, 8 * G * p.splits * p.sout_p},
                             {"ps", w.ps, 8 * G * p.splits * p.sout_p},
                             {"ranges", w.ranges, 16 * G},
                             {"bad", w.bad, 8}};
    if (staged) {
        pc.push_back({"flse", w.flse, 8 * G * S_out});
        pc.push_back({"fself", w.fself, 8 * G * S_out});
    } else {
        CHECK(!w.flse && !w.fself);
    }
    for (size_t i = 0; i < pc.size(); ++i) {
        CHECK(pc[i].p != nullptr);
        CHECK(((uintptr_t)pc[i].p & 15) == 0);
        if (pc[i].p) memset(pc[i].p, (int)(i + 1), (size_t)pc[i].bytes);          // (past the end: the sanitizer stops the program)
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
    const int64_t ns[] = {1, 2, 63, 64, 65, 127, 128, 129, 257, 1000, 4096, 100000, EIG_MAX_S};
    const int gs[] = {1, 2, 10, 64}, sps[] = {0, 1, 2, 3, 7, 64};
    for (int64_t so : ns)
        for (int64_t si : ns)
            for (int g : gs)
                for (int sp : sps)
                    for (int cu : {1, 256, 304}) check_plan(so, si, g, sp, cu);
    // automatic ranges: few outer rows are spread over the device, the full-size call is not cut
    CHECK(eig_plan(1, 100000, 1, 0, 256).splits == 63);                  // (1563 tiles, 25 per range)
    CHECK(eig_plan(1, 100000, 1, 0, 256).tiles_per_split == 25);
    CHECK(eig_plan(8192, 100000, 10, 0, 256).splits == 1);
    CHECK(eig_plan(128, 1000, 2, 0, 256).splits == 16);                  // (16 tiles: one per range)
    CHECK(eig_plan(1000, 63, 1, 7, 256).splits == 1);
    CHECK(eig_plan(1000, 1000, 3, 3, 256).splits == 3 && eig_plan(1000, 1000, 3, 64, 256).splits == 16);
    for (int staged = 0; staged < 2; ++staged) {
        check_layout(1, 1, 1, 1, 0, staged);
        check_layout(7, 65, 129, 3, 2, staged);
        check_layout(91, 257, 1000, 4, 64, staged);
        check_layout(17, 1000, 63, 64, 0, staged);
        check_layout(4096, 64, 64, 10, 1, staged);
    }
    if (g_failed) return 1;
    puts("eig_plan_check: ok");
    return 0;
}
