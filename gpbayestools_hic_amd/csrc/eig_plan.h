// eig_plan.h — how gpb_eig_lse (gpb_eig.hip) cuts its work: the tile of the main kernel, the padded panel widths, the ranges of
// the inner axis ("splits") and the doubles of workspace.  Functions of plain integers, host only and free of HIP:
// tests/host/eig_plan_check.cpp runs them alone.  The ranges are merged in range order, so a plan changes a result only within
// the rounding of the log-sum-exp; the same plan gives the same bits.
#pragma once
#include <stdint.h>

namespace gpb {

constexpr int EIG_TILE_OUT = 64;      // outer rows per workgroup
constexpr int EIG_TILE_IN = 64;       // inner samples per tile of the walk
constexpr int EIG_KB = 16;            // K step: 8 observables, a (q, t) and a (l, u) row each
constexpr int EIG_MAX_SPLITS = 64;
constexpr int EIG_MAX_GROUPS = 64;
constexpr int EIG_MAX_M = 4096;
constexpr int64_t EIG_MAX_S = 0x7fffffffLL - EIG_TILE_IN;      // samples of either set: the padded widths stay ints

inline int64_t eig_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct EigPlan {
    int64_t sout_p, sin_p;        // widths of the operand panels: S_out, S_in rounded up to whole tiles
    int64_t out_tiles, in_tiles;
    int splits;                   // ranges of the inner axis, every one with at least one tile
    int64_t tiles_per_split;
};

// splits_arg as the caller gave it (0: automatic: two workgroups per compute unit where the inner axis has the tiles for it)
inline EigPlan eig_plan(int64_t S_out, int64_t S_in, int G, int splits_arg, int num_cu) {
    EigPlan p;
    p.out_tiles = eig_ceil(S_out, EIG_TILE_OUT);
    p.in_tiles = eig_ceil(S_in, EIG_TILE_IN);
    p.sout_p = p.out_tiles * EIG_TILE_OUT;
    p.sin_p = p.in_tiles * EIG_TILE_IN;
    int64_t want = splits_arg > 0 ? splits_arg : eig_ceil(2 * (int64_t)(num_cu > 0 ? num_cu : 1), p.out_tiles * (G > 0 ? G : 1));
    if (want > EIG_MAX_SPLITS) want = EIG_MAX_SPLITS;
    if (want > p.in_tiles) want = p.in_tiles;
    if (want < 1) want = 1;
    p.tiles_per_split = eig_ceil(p.in_tiles, want);
    p.splits = (int)eig_ceil(p.in_tiles, p.tiles_per_split);      // (no range is empty)
    return p;
}

}  // namespace gpb
