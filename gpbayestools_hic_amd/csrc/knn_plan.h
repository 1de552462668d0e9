// knn_plan.h — how gpb_chain_knn (gpb_knn.hip) cuts its work: the padded list length, the ranges of B ("splits") and the slabs
// of A.  Functions of plain integers, host only and free of HIP: tests/host/knn_plan_check.cpp runs them alone.  Nothing here
// can change a result — the lists of the ranges are merged in (distance, row number) order and a slab is a set of query rows —,
// only how much of the device a call fills and how much workspace it holds.
#pragma once
#include <stdint.h>

namespace gpb {

constexpr int KNN_TILE_A = 256;       // query rows per workgroup, one per lane
constexpr int KNN_TILE_B = 64;        // candidate rows per LDS tile
constexpr int KNN_MAX_SPLITS = 64;
constexpr int KNN_MAX_K = 16;

// the list length the kernels are instantiated for: the first kmax entries of the KP nearest are the kmax nearest
constexpr int knn_kpad(int kmax) { return kmax <= 4 ? 4 : kmax <= 8 ? 8 : 16; }

struct KnnPlan {
    int kp;               // padded list length
    int splits;           // ranges of B, every one with at least one row
    int64_t per_split;    // rows of B per range, whole tiles
    int64_t slab;         // query rows per pass, whole tiles of KNN_TILE_A (the last pass may hold fewer)
    int64_t n_slabs;
    int64_t fixed_bytes;  // the scaled copy of B (of A in self mode)
    int64_t row_bytes;    // what a query row of a slab holds: its scaled copy (cross mode), a list per range, the staged results
};

inline int64_t knn_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

// nA, nB rows (self mode: nB == nA), dp the padded width, splits_arg as the caller gave it (0: automatic), budget in bytes
inline KnnPlan knn_plan(int64_t nA, int64_t nB, int dp, int kmax, int self, int splits_arg, int num_cu, int64_t budget) {
    KnnPlan p;
    p.kp = knn_kpad(kmax);
    const int64_t atiles = knn_ceil(nA, KNN_TILE_A), btiles = knn_ceil(nB, KNN_TILE_B);
    int64_t want = splits_arg > 0 ? splits_arg : knn_ceil(2 * (int64_t)(num_cu > 0 ? num_cu : 1), atiles);
    if (want > KNN_MAX_SPLITS) want = KNN_MAX_SPLITS;
    if (want > btiles) want = btiles;
    if (want < 1) want = 1;
    const int64_t tiles_per = knn_ceil(btiles, want);
    p.per_split = tiles_per * KNN_TILE_B;
    p.splits = (int)knn_ceil(btiles, tiles_per);              // (no range is empty)
    p.fixed_bytes = nB * dp * 8;
    const int64_t list = (int64_t)p.kp * 12 + 4;              // r2 | idx | zeros of one list
    p.row_bytes = (self ? 0 : (int64_t)dp * 8) + (int64_t)p.splits * list + list;
    const int64_t head = 4096;                                // counters, inv_scale and the pieces' rounding to 8 bytes
    const int64_t avail = budget > p.fixed_bytes + head ? budget - p.fixed_bytes - head : 0;
    int64_t slab = avail / p.row_bytes / KNN_TILE_A * KNN_TILE_A;
    if (slab < KNN_TILE_A) slab = KNN_TILE_A;                 // (a scaled copy above the budget: one tile at a time)
    if (slab > atiles * KNN_TILE_A) slab = atiles * KNN_TILE_A;
    p.slab = slab;
    p.n_slabs = knn_ceil(nA, slab);
    return p;
}

}  // namespace gpb
