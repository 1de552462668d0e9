// sl_index_check.cpp — stand-alone host check of csrc/sl_index.h, the index arithmetic of the int8 predict kernel's K loop
// (csrc/gpb_sliced.hip): the DMA source of every (wave, piece, K-step) in its closed and its incremental form.
// The kernel's walk over a tile is replayed here with the header's own functions —
// sources set once per tile, moved by the stride after every stage — and held against the plane layout restated from its
// description (plane[t][k / 16][row][16 bytes]), inside the buffers as sliced_prepare sizes them.  This is the check that finds an
// out-of-range DMA before a kernel issues it.  Built with the address and undefined-behaviour sanitizers by
// tests/test_sl_index_host.py; exit status 0 = every check held.
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "../../gpbayestools_hic_amd/csrc/sl_index.h"

using namespace gpb;

static long g_failed = 0;
// where a failing check stood (-1: not inside that loop)
static struct Where {
    int D, WTN;
    long long Np, Wld;
    int kskip, ib, wt, wave, piece, step;
} g_at;
#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            if (g_failed < 20)                                                                                               \
                fprintf(stderr, "line %d: %s   [D %d WTN %d Np %lld Wld %lld kskip %d: row block %d walker tile %d wave %d " \
                        "piece %d step %d]\n", __LINE__, #cond, g_at.D, g_at.WTN, g_at.Np, g_at.Wld, g_at.kskip, g_at.ib,     \
                        g_at.wt, g_at.wave, g_at.piece, g_at.step);                                                          \
            ++g_failed;                                                                                                      \
        }                                                                                                                    \
    } while (0)

// restated, not read from the kernel: 8 waves of a workgroup, 128-row block tile, 1-KB pieces (64 granules of 16 bytes)
static const int WAVES = 8, BM = 128, DMAX = 7;

struct Totals { long dmas = 0, steps = 0; };

static Totals check_geometry(int D, int WTN, int64_t Np, int64_t Wld, int kskip) {
    Totals tot;
    g_at = Where{D, WTN, (long long)Np, (long long)Wld, kskip, -1, -1, -1, -1, -1};
    const int64_t Np128 = (Np + 127) / 128 * 128;
    const int BN = 64 * WTN;
    const int a_chunks = D * 2 * (BM / 64), b_chunks = D * 2 * WTN, chunks = a_chunks + b_chunks;
    const int npw = (chunks + WAVES - 1) / WAVES, rem = chunks % WAVES;
    const int64_t a_plane = (Np / 16) * Np128 * 16, b_plane = (Np / 16) * Wld * 16;
    // one GP's share of the buffers: sliced_prepare allocates P x DMAX x Np x Np128 and P x DMAX x Np x Wcap bytes (Wcap >= Wld), and
    // GP p's planes begin at p x D x plane: its D planes lie inside the allocation for every p < P
    const int64_t a_bytes = (int64_t)D * a_plane, b_bytes = (int64_t)D * b_plane;
    CHECK(a_bytes <= (int64_t)DMAX * Np * Np128 && b_bytes <= (int64_t)DMAX * Np * Wld);
    const int nI = (int)(Np128 / BM), nW = (int)(Wld / BN);
    const int64_t ks = (kskip / 32) * 32;
    for (int ib = 0; ib < nI; ++ib) {
        g_at.ib = ib; g_at.wt = g_at.wave = g_at.piece = g_at.step = -1;
        const int64_t mb = (int64_t)ib * BM;
        const int64_t k_end = mb + BM < Np ? mb + BM : Np;
        const int64_t k_begin = ks <= mb ? ks : 0;
        const int nsteps = (int)((k_end - k_begin) / 32);
        const int64_t kb_first = k_begin / 16;
        CHECK(nsteps >= 1 && k_begin % 32 == 0 && (k_end - k_begin) % 32 == 0);
        tot.steps += nsteps;
        // ---- the DMA sources
        for (int wt = 0; wt < nW; ++wt) {
            const int64_t nb = (int64_t)wt * BN;
            std::vector<int> seen_a, seen_b;                               // per stage: every (plane, k-block, 64-row piece) once
            for (int wave = 0; wave < WAVES; ++wave) {
                for (int c = 0; c < npw; ++c) {
                    if (c == npw - 1 && rem != 0 && wave >= rem) break;
                    const int ch = WAVES * c + wave;
                    g_at.wt = wt; g_at.wave = wave; g_at.piece = ch; g_at.step = -1;
                    CHECK(ch < chunks);
                    const SlChunk k = sl_chunk(ch, D, WTN);
                    const int64_t ld = k.is_a ? Np128 : Wld, off = k.is_a ? mb : nb, plane = k.is_a ? a_plane : b_plane;
                    const int64_t bytes = k.is_a ? a_bytes : b_bytes;
                    CHECK(k.t >= 0 && k.t < D && (k.q == 0 || k.q == 1) && k.h >= 0 && k.h < (k.is_a ? BM / 64 : WTN));
                    // pieces are dealt in the order the LDS stage is laid out: piece ch lands at ch x 1 KB, where the fragment
                    // reads expect (plane t, k-block q, rows 64 h ..)
                    CHECK(ch == (k.is_a ? 0 : a_chunks) + (k.t * 2 + k.q) * (k.is_a ? BM / 64 : WTN) + k.h);
                    int64_t inc = sl_src_offset(k, plane, ld, off, kb_first, 0);      // the kernel: once per tile ...
                    for (int s = 0; s < nsteps; ++s) {
                        const int64_t closed = sl_src_offset(k, plane, ld, off, kb_first, s);
                        // the layout, restated: plane[t][k / 16][row][16 bytes], k = k_begin + 32 s + 16 q, row = off + 64 h (+ lane)
                        const int64_t kb = (k_begin + 32 * (int64_t)s) / 16 + k.q;
                        const int64_t want = ((k.t * (Np / 16) + kb) * ld + off + 64 * k.h) * 16;
                        g_at.step = s;
                        CHECK(closed == want);
                        CHECK(inc == closed);
                        CHECK(kb < Np / 16 && off + 64 * k.h + 63 < ld);         // inside the plane's k-blocks and rows
                        CHECK(inc >= 0 && inc % 16 == 0);                         // lane 0's granule ...
                        CHECK(inc + 63 * 16 + 16 <= bytes);                       // ... and lane 63's last byte: inside the GP's planes
                        CHECK(inc + 63 * 16 < ((int64_t)1 << 40));
                        inc += sl_src_stride(ld);                                  // ... then moved after every stage
                        ++tot.dmas;
                    }
                    (k.is_a ? seen_a : seen_b).push_back((k.t * 2 + k.q) * 4 + k.h);
                }
            }
            CHECK((int)seen_a.size() == a_chunks && (int)seen_b.size() == b_chunks);
            for (int op = 0; op < 2; ++op) {
                std::vector<int>& v = op ? seen_b : seen_a;
                std::vector<char> hit(DMAX * 2 * 4, 0);
                for (int id : v) { CHECK(!hit[id]); hit[id] = 1; }
            }
        }
    }
    return tot;
}

int main() {
    const int64_t NPS[] = {64, 128, 192, 256, 320, 1024, 2048};
    const int64_t WLDS[] = {64, 128, 192, 2048};
    const int KSKIPS[] = {0, 16, 32, 48, 96};
    const int DEPTHS[] = {7, 6}, WTNS[] = {1, 2};
    long geometries = 0, dmas = 0;
    for (int D : DEPTHS)
        for (int WTN : WTNS)
            for (int64_t Np : NPS)
                for (int64_t Wld : WLDS)
                    for (int kskip : KSKIPS) {
                        if (Wld % (64 * WTN)) continue;                  // (a batch is padded to whole walker tiles)
                        const Totals t = check_geometry(D, WTN, Np, Wld, kskip);
                        ++geometries; dmas += t.dmas;
                        g_at.ib = -1;                                      // (the totals of the geometry)
                        // K-steps of all row blocks: the triangle's 4 (ib + 1) per block, less what the front padding skips
                        if (Np == 2048 && kskip == 0) CHECK(t.steps == 544);
                        if (Np == 2048 && kskip == 96) CHECK(t.steps == 544 - 3 * 15);
                        if (Np == 64) CHECK(t.steps == 2);                 // ragged: K ends at row 64
                    }
    if (g_failed) {
        fprintf(stderr, "sl_index_check: %ld checks failed\n", g_failed);
        return 1;
    }
    printf("sl_index_check: ok (%ld geometries, %ld DMAs)\n", geometries, dmas);
    return 0;
}
