// maxpro_ws_check.cpp — stand-alone host check of the MaxPro generator's workspace layout (MaxproWs, csrc/ws_layout.h), in the
// manner of kmeans_ws_check.cpp: the counting pass and the carving pass report the same total, which is the sum of the pieces
// rounded to 8 bytes each; on a malloc of exactly that many bytes every byte of every piece is written with the piece's tag and
// read back (the sanitizer watches the bounds, the tags an overlap); the pieces a call does not use are null.  The largest shape
// (4096 x 64, 16 restarts: 2.1 GB of pair matrices) is counted and summed only, the largest single restart is written as well.
// Built with the address and undefined-behaviour sanitizers by tests/test_maxpro_host.py; exit status 0 = every check held.
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

static int64_t up8(int64_t b) { return (b + 7) / 8 * 8; }

static void check(int64_t n, int64_t d, int64_t R, int64_t n_trace, int real, bool write) {
    MaxproWs count;
    Carver<int64_t> c0;
    count.lay(c0, n, d, R, n_trace, real);
    CHECK(!count.T && !count.rowsum && !count.lev && !count.x && !count.order);
    const int64_t want = real ? up8(8 * R * n * n) + up8(8 * R * n) + up8(32 * R) + up8(16 * R) + up8(8 * d * n) + up8(8 * n) + up8(4 * n)
                              : up8(8 * R * n * n) + up8(8 * R * n) + up8(32 * R) + up8(16 * R) + 2 * up8(4 * R * d * n) + up8(4 * R * n_trace);
    CHECK(8 * c0.total() == want);
    if (!write) return;
    const size_t bytes = 8 * (size_t)c0.total();
    unsigned char* mem = static_cast<unsigned char*>(malloc(bytes));
    MaxproWs w;
    Carver<int64_t> c1(reinterpret_cast<int64_t*>(mem));
    w.lay(c1, n, d, R, n_trace, real);
    CHECK(c1.total() == c0.total());
    std::vector<Piece> pc;
    if (R > 0) {
        pc.push_back({"T", w.T, 8 * R * n * n});
        pc.push_back({"rowsum", w.rowsum, 8 * R * n});
        pc.push_back({"sums", w.sums, 32 * R});
        pc.push_back({"counts", w.counts, 16 * R});
    } else {
        CHECK(!w.T && !w.rowsum && !w.sums && !w.counts);
    }
    if (real) {
        CHECK(!w.lev && !w.best && !w.trace);
        pc.push_back({"x", w.x, 8 * d * n});
        pc.push_back({"score", w.score, 8 * n});
        pc.push_back({"order", w.order, 4 * n});
    } else {
        CHECK(!w.x && !w.score && !w.order);
        pc.push_back({"lev", w.lev, 4 * R * d * n});
        pc.push_back({"best", w.best, 4 * R * d * n});
        if (n_trace) pc.push_back({"trace", w.trace, 4 * R * n_trace});
        else CHECK(!w.trace);
    }
    for (size_t i = 0; i < pc.size(); ++i) {
        CHECK(pc[i].p != nullptr);
        if (pc[i].p) memset(pc[i].p, (int)(i + 1), (size_t)pc[i].bytes);         // (past the end: the sanitizer stops the program)
    }
    for (size_t i = 0; i < pc.size(); ++i) {
        if (!pc[i].p) continue;
        const unsigned char* b = static_cast<const unsigned char*>(pc[i].p);
        std::vector<unsigned char> tag((size_t)pc[i].bytes, (unsigned char)(i + 1));
        if (memcmp(b, tag.data(), (size_t)pc[i].bytes) != 0) {
            fprintf(stderr, "%s overlaps another piece\n", pc[i].name);
            ++g_failed;
        }
    }
    free(mem);
}

int main() {
    check(4, 2, 1, 0, 0, true);                  // the smallest
    check(4, 2, 1, 1, 0, true);
    check(4, 2, 0, 0, 1, true);                  // the criterion of a real design: no pair matrix
    check(4, 2, 1, 0, 1, true);                  // the run order: one
    check(1101, 21, 3, 77, 0, true);             // odd everywhere
    check(1101, 21, 1, 0, 1, true);
    check(4096, 64, 1, 33, 0, true);             // the largest restart
    check(4096, 64, 1, 0, 1, true);
    check(4096, 64, 16, 1000003, 0, false);      // the largest call
    if (g_failed) return 1;
    puts("maxpro_ws_check: ok");
    return 0;
}
