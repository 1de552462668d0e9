// maxpro_index_check.cpp — stand-alone host check of csrc/maxpro_index.h, the header that gpb_maxpro.hip and
// tests/maxpro_reference.py share: a decoded proposal lies in range with a != b at every corner of the word range and over a
// sweep of words; every row and column is reached; the strided row loop of a group of `width` lanes covers the rows 0 .. n - 1
// once each for n around the widths the kernels use (64: a wave of k_mp_anneal; 256: k_mp_build; 1024: k_mp_anneal's update and
// k_mp_order); ln psi agrees with its definition.  Built with the address and undefined-behaviour sanitizers by
// tests/test_maxpro_host.py; exit status 0 = every check held.
#include <math.h>
#include <stdio.h>
#include <vector>
#include "../../gpbayestools_hic_amd/csrc/maxpro_index.h"

using namespace gpb;

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++g_failed; } \
    } while (0)

static void decode_checks(int n, int d) {
    const uint32_t corner[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    std::vector<int> seen_a((size_t)n, 0), seen_b((size_t)n, 0), seen_c((size_t)d, 0);
    auto one = [&](uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
        const MpProposal p = mp_decode(x, y, z, w, n, d);
        const bool ok = p.c >= 0 && p.c < d && p.a >= 0 && p.a < n && p.b >= 0 && p.b < n && p.a != p.b && p.u > 0.0 && p.u < 1.0;
        CHECK(ok);
        if (ok) seen_a[(size_t)p.a] = seen_b[(size_t)p.b] = seen_c[(size_t)p.c] = 1;
    };
    for (uint32_t x : corner)
        for (uint32_t y : corner)
            for (uint32_t z : corner)
                for (uint32_t w : corner) one(x, y, z, w);
    const uint32_t step = 0xffffffffu / 20011u;                // a sweep of the word range, all words alike and then spread
    for (uint32_t k = 0; k <= 20011u; ++k) {
        one(k * step, k * step, k * step, k * step);
        one(k * step, 0xffffffffu - k * step, k * 2654435761u, k * 40503u);
    }
    for (int i = 0; i < n; ++i) CHECK(seen_a[(size_t)i] && seen_b[(size_t)i]);
    for (int c = 0; c < d; ++c) CHECK(seen_c[(size_t)c]);
    // b is drawn from the n - 1 other rows: with a fixed, z runs through every one of them exactly
    const MpProposal lo = mp_decode(0, 0, 0, 0, n, d), hi = mp_decode(0, 0xffffffffu, 0xffffffffu, 0, n, d);
    CHECK(lo.a == 0 && lo.b == 1 && hi.a == n - 1 && hi.b == n - 2);
}

static void stride_checks(int width, int n) {
    std::vector<int> hits((size_t)n, 0);
    for (int lane = 0; lane < width; ++lane) {
        const int rows = mp_rows_of(lane, width, n);
        for (int k = 0; k < rows; ++k) {
            const int j = mp_row(lane, width, k);
            CHECK(j >= 0 && j < n);
            if (j >= 0 && j < n) ++hits[(size_t)j];
        }
        CHECK(mp_row(lane, width, rows) >= n);                 // the loop `for (j = lane; j < n; j += width)` ends here
    }
    for (int j = 0; j < n; ++j) CHECK(hits[(size_t)j] == 1);
}

int main() {
    const int shapes[][2] = {{4, 2}, {5, 3}, {7, 2}, {64, 64}, {65, 3}, {1100, 4}, {4095, 63}, {4096, 64}};
    for (const auto& s : shapes) decode_checks(s[0], s[1]);
    const int widths[] = {64, 256, 1024};
    for (int w : widths)
        for (int n : {4, 5, w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1, 4095, 4096})
            if (n >= MP_MIN_N && n <= MP_MAX_N) stride_checks(w, n);
    CHECK(MP_MAX_N / 1024 * 1024 == MP_MAX_N);                  // k_mp_order keeps MP_MAX_N / 1024 rows per lane
    CHECK(fabs(MP_E15 - exp(1.5)) < 1e-15 && fabs(mp_scale(8) * 8.0 - MP_E15) < 1e-15);
    // two points at distance 1/2 in each of two columns: psi = ((1/4 1/4)^-1)^(1/2) = 4; f = ln((e^1.5 / 2)^-4)
    CHECK(fabs(mp_lnpsi(-4.0 * log(MP_E15 * 0.5), 2, 2) - log(4.0)) < 1e-14);
    if (g_failed) return 1;
    puts("maxpro_index_check: ok");
    return 0;
}
