// stein_plan_check.cpp — stand-alone host check of the plans and workspace layouts of gpb_stein_thin and gpb_stein_ksd
// (csrc/stein_plan.h), in the manner of knn_plan_check.cpp: over a grid of sizes up to 2^31 - 1 rows the workgroups of a thinning
// pass cover every row once and none is empty, the column ranges cover every chunk once and none is empty, the slabs cover the
// query rows in whole tiles and their chunk partials stay under the budget whenever one tile fits; the counting pass and the
// carving pass agree, and on a malloc of exactly that many bytes every byte of every piece is written with the piece's tag and
// read back (overrun: the sanitizer; overlap: the tags).  Built with the address and undefined-behaviour sanitizers by
// tests/test_stein_plan_host.py; exit status 0 = every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../gpbayestools_hic_amd/csrc/stein_plan.h"

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

static void check_pieces(unsigned char* mem, int64_t bytes, std::vector<Piece>& pc) {
    int64_t sum = 0;
    for (size_t i = 0; i < pc.size(); ++i) {
        CHECK(pc[i].p != nullptr);
        if (pc[i].p) memset(pc[i].p, (int)(i + 1), (size_t)pc[i].bytes);          // (past the end: the sanitizer stops the program)
        sum += pc[i].bytes;
    }
    CHECK(sum <= bytes);
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
    (void)mem;
}

static void check_thin(int64_t n) {
    const SteinThinPlan p = stein_thin_plan(n);
    CHECK(p.blocks >= 1 && p.blocks <= STEIN_MAX_BLOCKS);
    CHECK(p.per_block % STEIN_THREADS == 0 && p.per_block >= STEIN_THREADS);
    CHECK((int64_t)p.blocks * p.per_block >= n);                        // the workgroups cover the rows ...
    CHECK((int64_t)(p.blocks - 1) * p.per_block < n);                   // ... and the last one is not empty
}

static void check_thin_layout(int64_t n, int64_t d, int64_t dp, int64_t m) {
    const SteinThinPlan p = stein_thin_plan(n);
    SteinThinWs count;
    Carver<int64_t> c0;
    count.lay(c0, n, d, dp, p.blocks, m);
    CHECK(count.x == nullptr && count.obj == nullptr);
    const int64_t bytes = 8 * c0.total();
    unsigned char* mem = static_cast<unsigned char*>(malloc((size_t)bytes));
    SteinThinWs w;
    Carver<int64_t> c1(reinterpret_cast<int64_t*>(mem));
    w.lay(c1, n, d, dp, p.blocks, m);
    CHECK(c1.total() == c0.total());
    CHECK(reinterpret_cast<unsigned char*>(w.S) == reinterpret_cast<unsigned char*>(w.counter) + 8);   // one memset clears both
    std::vector<Piece> pc = {{"counter", w.counter, 8}, {"S", w.S, 8}, {"ginv", w.ginv, 8 * d * d}, {"x", w.x, 8 * n * dp},
                             {"b", w.b, 8 * n * dp}, {"g", w.g, 8 * n * dp}, {"obj", w.obj, 8 * n},
                             {"pmin0", w.pmin[0], 8 * p.blocks}, {"prow0", w.prow[0], 4 * p.blocks},
                             {"pmin1", w.pmin[1], 8 * p.blocks}, {"prow1", w.prow[1], 4 * p.blocks},
                             {"fidx", w.fidx, 4 * m}, {"fksd", w.fksd, 8 * m}};
    check_pieces(mem, bytes, pc);
    free(mem);
}

static SteinKsdPlan check_ksd(int64_t n, int splits, int num_cu, int64_t budget) {
    const SteinKsdPlan p = stein_ksd_plan(n, splits, num_cu, budget);
    CHECK(p.chunks == stein_ceil(n, STEIN_CHUNK));
    CHECK(p.splits >= 1 && p.splits <= STEIN_MAX_SPLITS && (splits == 0 || p.splits <= splits));
    CHECK(p.chunks_per >= 1 && (int64_t)p.splits * p.chunks_per >= p.chunks);      // the ranges cover the chunks ...
    CHECK((int64_t)(p.splits - 1) * p.chunks_per < p.chunks);                      // ... and the last one is not empty
    CHECK(p.slab % STEIN_THREADS == 0 && p.slab >= STEIN_THREADS);
    CHECK(p.n_slabs * p.slab >= n && (p.n_slabs - 1) * p.slab < n);
    CHECK(p.slab <= stein_ceil(n, STEIN_THREADS) * STEIN_THREADS);
    if (8 * p.chunks * STEIN_THREADS <= budget) CHECK(8 * p.chunks * p.slab <= budget);
    return p;
}

static void check_ksd_layout(int64_t n, int64_t d, int64_t dp, int splits, int64_t budget) {
    const SteinKsdPlan p = check_ksd(n, splits, 256, budget);
    SteinKsdWs count;
    Carver<int64_t> c0;
    count.lay(c0, n, d, dp, p.chunks, p.slab);
    CHECK(count.x == nullptr && count.part == nullptr);
    const int64_t bytes = 8 * c0.total();
    unsigned char* mem = static_cast<unsigned char*>(malloc((size_t)bytes));
    SteinKsdWs w;
    Carver<int64_t> c1(reinterpret_cast<int64_t*>(mem));
    w.lay(c1, n, d, dp, p.chunks, p.slab);
    CHECK(c1.total() == c0.total());
    std::vector<Piece> pc = {{"counter", w.counter, 8}, {"ginv", w.ginv, 8 * d * d}, {"x", w.x, 8 * n * dp}, {"b", w.b, 8 * n * dp},
                             {"g", w.g, 8 * n * dp}, {"part", w.part, 8 * p.chunks * p.slab}, {"rs", w.rs, 8 * n},
                             {"csum", w.csum, 8 * stein_ceil(n, STEIN_ROW_CHUNK)}, {"fksd2", w.fksd2, 8}};
    check_pieces(mem, bytes, pc);
    free(mem);
}

int main() {
    const int64_t budget = (int64_t)16 << 20;
    const int64_t ns[] = {1, 63, 255, 256, 257, 1000, 1024, 1025, 4096, 70001, 102400, 262144, 262145, 1000000, 2147483647LL};
    for (int64_t n : ns) {
        check_thin(n);
        for (int sp : {0, 1, 2, 7, 64})
            for (int cu : {1, 256, 304}) check_ksd(n, sp, cu, budget);
    }
    CHECK(stein_thin_plan(1).blocks == 1 && stein_thin_plan(256).blocks == 1 && stein_thin_plan(257).blocks == 2);
    CHECK(stein_thin_plan(70001).blocks == 274);                                   // more partials than one wave holds
    CHECK(stein_thin_plan(262144).blocks == 1024 && stein_thin_plan(262145).per_block == 512);
    // automatic ranges: a small set is spread over the device, no range without a chunk
    CHECK(stein_ksd_plan(1000, 0, 256, budget).splits == 1);
    CHECK(stein_ksd_plan(5000, 0, 256, budget).splits == 5 && stein_ksd_plan(5000, 2, 256, budget).splits == 2);
    CHECK(stein_ksd_plan(5000, 7, 256, budget).splits == 5);
    CHECK(stein_ksd_plan(102400, 0, 256, budget).n_slabs == 5);
    // the size at which tests/test_gpu_stein.py relies on three slabs with the boundaries 30208 and 60416
    CHECK(stein_ksd_plan(70001, 0, 256, budget).n_slabs == 3 && stein_ksd_plan(70001, 1, 256, budget).slab == 30208);
    CHECK(stein_ksd_plan(70001, 64, 256, budget).splits == 35);                    // (69 chunks, 2 per range)
    CHECK(stein_ksd_plan(5000, 0, 256, budget).n_slabs == 1);
    check_thin_layout(1, 1, 8, 1);
    check_thin_layout(257, 20, 20, 40);
    check_thin_layout(1000, 33, 48, 64);
    check_thin_layout(70001, 5, 8, 8);
    check_ksd_layout(1, 1, 8, 0, budget);
    check_ksd_layout(257, 20, 20, 2, budget);
    check_ksd_layout(5000, 64, 64, 7, budget);
    check_ksd_layout(70001, 5, 8, 0, budget);
    check_ksd_layout(9000, 3, 8, 0, 1 << 16);                                      // a small budget: several slabs
    if (g_failed) return 1;
    puts("stein_plan_check: ok");
    return 0;
}
