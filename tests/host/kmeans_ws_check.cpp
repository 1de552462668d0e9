// kmeans_ws_check.cpp — stand-alone host check of gpb_chain_kmeans' workspace layout (KmeansWs, csrc/ws_layout.h), in the manner of
// ws_carve_check.cpp: the counting pass and the carving pass report the same total; on a malloc of exactly that many bytes every
// byte of every piece is written with the piece's tag and read back (the sanitizer watches the bounds, the tags an overlap); the
// zeroed run covers the state pieces and nothing else; the pieces of a call without seeding are null.  Built with the address and
// undefined-behaviour sanitizers by tests/test_kmeans_ws_host.py; exit status 0 = every check held.
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
    bool state;                 // inside the run that is zeroed at the start of a call
};

static void check(int64_t S, int64_t R, int64_t k, int64_t d, int64_t nb, int seeding) {
    KmeansWs count;
    Carver<int64_t> c0;
    count.lay(c0, S, R, k, d, nb, seeding);
    CHECK(count.weff == nullptr && count.lab == nullptr && count.cen == nullptr);
    const size_t bytes = 8 * (size_t)c0.total();
    unsigned char* mem = static_cast<unsigned char*>(malloc(bytes));
    KmeansWs w;
    Carver<int64_t> c1(reinterpret_cast<int64_t*>(mem));
    w.lay(c1, S, R, k, d, nb, seeding);
    CHECK(c1.total() == c0.total() && w.state_bytes == count.state_bytes);
    const int64_t nm = 5 * d + 1;
    std::vector<Piece> pc = {{"counters", w.counters, 8 * 4, true}, {"cen", w.cen, 8 * R * k * d, true}, {"shift", w.shift, 8 * R, true},
                             {"acc", w.acc, 8 * R * k * d, true}, {"wq", w.wq, 8 * R * k, true}, {"cnt", w.cnt, 8 * R * k, true},
                             {"iner", w.iner, 8 * R, true}, {"seed", w.seed, 8 * R * k, true}, {"changed", w.changed, 4 * R, true},
                             {"done", w.done, 4 * R, true}, {"conv", w.conv, 4 * R, true}, {"niter", w.niter, 4 * R, true},
                             {"fi", w.fi, 4 * R, true}, {"ms", w.ms, 8 * 2 * d, false}, {"mom", w.mom, 8 * nm, false},
                             {"part", w.part, 8 * nb * nm, false}, {"weff", w.weff, 8 * S, false}, {"lab", w.lab, R * S, false}};
    if (seeding) {
        pc.push_back({"u", w.u, 8 * R * k, false});
        pc.push_back({"bs", w.bs, 8 * R * nb, false});
        pc.push_back({"selb", w.selb, 4 * R, false});
        pc.push_back({"selv", w.selv, 8 * 2 * R, false});
    } else {
        CHECK(!w.u && !w.bs && !w.selb && !w.selv);
    }
    CHECK(reinterpret_cast<unsigned char*>(w.state0) == mem && w.done == w.changed + R && w.fi == w.changed + 4 * R);
    for (size_t i = 0; i < pc.size(); ++i) {
        CHECK(pc[i].p != nullptr);
        if (!pc[i].p) continue;
        const int64_t off = static_cast<unsigned char*>(pc[i].p) - mem;
        CHECK(pc[i].state == (off + pc[i].bytes <= w.state_bytes));              // wholly inside the zeroed run, or wholly behind it
        CHECK(pc[i].state || off >= w.state_bytes);
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
    check(1, 1, 1, 1, 1, 0);
    check(1, 1, 1, 1, 1, 1);
    check(257, 1, 2, 3, 2, 1);
    check(4099, 10, 10, 20, 17, 0);
    check(3000, 16, 32, 64, 12, 1);
    check(1023, 3, 7, 5, 4, 1);
    if (g_failed) return 1;
    puts("kmeans_ws_check: ok");
    return 0;
}
