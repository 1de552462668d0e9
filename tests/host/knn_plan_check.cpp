// knn_plan_check.cpp — stand-alone host check of gpb_chain_knn's plan (csrc/knn_plan.h) and workspace layout (KnnWs,
// csrc/ws_layout.h), in the manner of kmeans_ws_check.cpp: over a grid of sizes the ranges of B cover every row once and none is
// empty, the slabs cover A in whole tiles, what grows with a slab stays under the budget whenever one tile fits, the counting
// pass and the carving pass agree, and on a malloc of exactly that many bytes every byte of every piece is written with the
// piece's tag and read back (overrun: the sanitizer; overlap: the tags).  Built with the address and undefined-behaviour
// sanitizers by tests/test_knn_plan_host.py; exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../gpbayestools_hic_amd/csrc/knn_plan.h"
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

static KnnPlan check_plan(int64_t nA, int64_t nB, int dp, int kmax, int self, int splits, int num_cu, int64_t budget) {
    const KnnPlan p = knn_plan(nA, nB, dp, kmax, self, splits, num_cu, budget);
    CHECK(p.kp >= kmax && (p.kp == 4 || p.kp == 8 || p.kp == 16));
    CHECK(p.splits >= 1 && p.splits <= KNN_MAX_SPLITS && (splits == 0 || p.splits <= splits));
    CHECK(p.per_split % KNN_TILE_B == 0 && p.per_split >= KNN_TILE_B);
    CHECK((int64_t)p.splits * p.per_split >= nB);                       // the ranges cover B ...
    CHECK((int64_t)(p.splits - 1) * p.per_split < nB);                  // ... and the last one is not empty
    CHECK(p.slab % KNN_TILE_A == 0 && p.slab >= KNN_TILE_A);
    CHECK(p.n_slabs * p.slab >= nA && (p.n_slabs - 1) * p.slab < nA);
    CHECK(p.slab <= knn_ceil(nA, KNN_TILE_A) * KNN_TILE_A);
    return p;
}

static void check_layout(int64_t nA, int64_t nB, int dp, int kmax, int self, int splits, int staged, int64_t budget) {
    const KnnPlan p = check_plan(nA, nB, dp, kmax, self, splits, 256, budget);
    KnnWs count;
    Carver<int64_t> c0;
    count.lay(c0, nB, p.slab, dp, p.kp, kmax, p.splits, self ? 0 : 1, staged);
    CHECK(count.zb == nullptr && count.pr2 == nullptr);
    const int64_t bytes = 8 * c0.total();
    if (p.fixed_bytes + 4096 + KNN_TILE_A * p.row_bytes <= budget) CHECK(bytes <= budget);      // under the budget where one tile fits
    unsigned char* mem = static_cast<unsigned char*>(malloc((size_t)bytes));
    KnnWs w;
    Carver<int64_t> c1(reinterpret_cast<int64_t*>(mem));
    w.lay(c1, nB, p.slab, dp, p.kp, kmax, p.splits, self ? 0 : 1, staged);
    CHECK(c1.total() == c0.total());
    std::vector<Piece> pc = {{"counters", w.counters, 16}, {"inv", w.inv, 8 * dp}, {"zb", w.zb, 8 * nB * dp},
                             {"pr2", w.pr2, 8 * p.splits * p.slab * p.kp}, {"pidx", w.pidx, 4 * p.splits * p.slab * p.kp},
                             {"pzeros", w.pzeros, 4 * p.splits * p.slab}};
    if (!self) pc.push_back({"za", w.za, 8 * p.slab * dp});
    else CHECK(!w.za);
    if (staged) {
        pc.push_back({"fr2", w.fr2, 8 * p.slab * kmax});
        pc.push_back({"fidx", w.fidx, 4 * p.slab * kmax});
        pc.push_back({"fzeros", w.fzeros, 4 * p.slab});
    } else {
        CHECK(!w.fr2 && !w.fidx && !w.fzeros);
    }
    for (size_t i = 0; i < pc.size(); ++i) {
        CHECK(pc[i].p != nullptr);
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
    const int64_t budget = (int64_t)256 << 20;
    const int64_t ns[] = {1, 63, 64, 65, 255, 256, 257, 1000, 4096, 100000, 2147483647LL};
    const int dps[] = {8, 20, 64}, ks[] = {1, 4, 5, 8, 9, 16}, sps[] = {0, 1, 2, 7, 64, 1000};
    for (int64_t nA : ns)
        for (int64_t nB : ns)
            for (int dp : dps)
                for (int k : ks)
                    for (int sp : sps)
                        for (int cu : {1, 256, 304}) {
                            check_plan(nA, nB, dp, k, 0, sp, cu, budget);
                            if (nA == nB) check_plan(nA, nB, dp, k, 1, sp, cu, budget);
                        }
    // automatic ranges: a small A is spread over the device, a large one is not cut
    CHECK(knn_plan(1, 100000, 20, 8, 0, 0, 256, budget).splits == 63);          // (1563 tiles, 25 per range)
    CHECK(knn_plan(1, 64 * 64, 20, 8, 0, 0, 256, budget).splits == KNN_MAX_SPLITS);
    CHECK(knn_plan(100000, 100000, 20, 8, 1, 0, 256, budget).splits == 2);
    CHECK(knn_plan(1000000, 1000000, 20, 8, 1, 0, 256, budget).splits == 1);
    CHECK(knn_plan(1000, 63, 20, 8, 0, 7, 256, budget).splits == 1);
    // the sizes at which tests/test_gpu_knn.py relies on more than one slab, and on one
    CHECK(knn_plan(50000, 4096, 8, 16, 0, 64, 256, budget).n_slabs == 3);
    CHECK(knn_plan(30000, 30000, 8, 16, 1, 64, 256, budget).n_slabs == 2);
    CHECK(knn_plan(50000, 4096, 8, 16, 0, 1, 256, budget).n_slabs == 1);
    CHECK(knn_plan(30000, 30000, 8, 16, 1, 1, 256, budget).n_slabs == 1);
    CHECK(knn_plan(100000, 100000, 20, 8, 1, 0, 256, budget).n_slabs == 1);
    // a scaled copy above the budget: one tile at a time
    CHECK(knn_plan(5000, 10000000, 64, 16, 0, 0, 256, budget).slab == KNN_TILE_A);
    for (int staged = 0; staged < 2; ++staged)
        for (int self = 0; self < 2; ++self) {
            check_layout(1, 1, 8, 1, self, 0, staged, budget);
            check_layout(257, 257, 20, 5, self, 2, staged, budget);
            check_layout(1000, 1000, 64, 16, self, 7, staged, budget);
            check_layout(3000, 3000, 48, 9, self, 0, staged, 1 << 20);        // a small budget: several slabs
            check_layout(4099, 4099, 8, 3, self, 64, staged, 1 << 22);
        }
    check_layout(1, 777, 24, 8, 0, 0, 1, budget);
    if (g_failed) return 1;
    puts("knn_plan_check: ok");
    return 0;
}
