// stein_plan.h — how gpb_stein_thin and gpb_stein_ksd (gpb_stein.hip) cut their work and lay out their workspace: the workgroups of
// a thinning pass, the column ranges ("splits") and the slabs of query rows of the full discrepancy.  Functions of plain integers,
// host only and free of HIP: tests/host/stein_plan_check.cpp runs them alone.  Nothing here can change a result — a row's sum is
// formed chunk of STEIN_CHUNK columns by chunk and the chunk partials are added in ascending order whatever range computed them,
// and the argmin of a thinning pass compares (value, row number) —, only how much of the device a call fills and what it holds.
#pragma once
#include <stdint.h>
#include "ws_carve.h"

namespace gpb {

constexpr int STEIN_THREADS = 256;          // lanes per workgroup; query rows per workgroup of the full discrepancy
constexpr int STEIN_CHUNK = 1024;           // GPB_STEIN_CHUNK of include/gpbayes.h: columns summed in ascending order into one partial
constexpr int STEIN_ROW_CHUNK = 256;        // rows per block_sum tree of the sum over i (block_reduce.h)
constexpr int STEIN_MAX_BLOCKS = 1024;      // workgroups of a thinning pass (their partials are reduced by every workgroup of the next)
constexpr int STEIN_MAX_SPLITS = 64;
constexpr int64_t STEIN_MAX_M = (int64_t)1 << 20;

inline int64_t stein_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- thinning: workgroup b owns the rows [b per_block, (b + 1) per_block), whole tiles of STEIN_THREADS
struct SteinThinPlan {
    int blocks;
    int64_t per_block;
};

inline SteinThinPlan stein_thin_plan(int64_t n) {
    SteinThinPlan p;
    const int64_t tiles = stein_ceil(n, STEIN_THREADS);
    const int64_t tiles_per = stein_ceil(tiles, STEIN_MAX_BLOCKS);
    p.per_block = tiles_per * STEIN_THREADS;
    p.blocks = (int)stein_ceil(tiles, tiles_per);                 // (no workgroup is without a row)
    return p;
}

// stein_ws of gpb_stein_thin, 8-byte units: counter | S | Ginv [d][d] | the packed rows x, b, g [n][dp] each | obj [n] | two sets
// of workgroup partials (min [blocks], row [blocks] int) | idx [m] (int) and ksd [m] as the passes write them
struct SteinThinWs {
    int64_t* counter;
    double *S, *ginv, *x, *b, *g, *obj, *pmin[2], *fksd;
    int *prow[2], *fidx;
    void lay(Carver<int64_t>& c, int64_t n, int64_t d, int64_t dp, int64_t blocks, int64_t m) {
        counter = c.take<int64_t>(1);
        S = c.take<double>(1);
        ginv = c.take<double>(d * d);
        x = c.take<double>(n * dp);
        b = c.take<double>(n * dp);
        g = c.take<double>(n * dp);
        obj = c.take<double>(n);
        for (int k = 0; k < 2; ++k) {
            pmin[k] = c.take<double>(blocks);
            prow[k] = c.take<int>(blocks);
        }
        fidx = c.take<int>(m);
        fksd = c.take<double>(m);
    }
};

// ---- full discrepancy
struct SteinKsdPlan {
    int64_t chunks;        // column chunks of STEIN_CHUNK
    int splits;            // ranges of columns, every one with at least one chunk
    int64_t chunks_per;    // chunks per range
    int64_t slab;          // query rows per pass, whole tiles of STEIN_THREADS (the last pass may hold fewer)
    int64_t n_slabs;
};

// splits_arg as the caller gave it (0: automatic); part_budget: bytes the chunk partials [chunks][slab] of one slab may take
inline SteinKsdPlan stein_ksd_plan(int64_t n, int splits_arg, int num_cu, int64_t part_budget) {
    SteinKsdPlan p;
    const int64_t tiles = stein_ceil(n, STEIN_THREADS);
    p.chunks = stein_ceil(n, STEIN_CHUNK);
    int64_t slab = part_budget / (8 * p.chunks) / STEIN_THREADS * STEIN_THREADS;
    if (slab < STEIN_THREADS) slab = STEIN_THREADS;
    if (slab > tiles * STEIN_THREADS) slab = tiles * STEIN_THREADS;
    p.slab = slab;
    p.n_slabs = stein_ceil(n, slab);
    const int64_t slab_tiles = slab / STEIN_THREADS;
    int64_t want = splits_arg > 0 ? splits_arg : stein_ceil(2 * (int64_t)(num_cu > 0 ? num_cu : 1), slab_tiles);
    if (want > STEIN_MAX_SPLITS) want = STEIN_MAX_SPLITS;
    if (want > p.chunks) want = p.chunks;
    if (want < 1) want = 1;
    p.chunks_per = stein_ceil(p.chunks, want);
    p.splits = (int)stein_ceil(p.chunks, p.chunks_per);          // (no range is empty)
    return p;
}

// stein_ws of gpb_stein_ksd, 8-byte units: counter | Ginv [d][d] | the packed rows x, b, g [n][dp] each | the chunk partials of a
// slab [chunks][slab] | the row sums [n] | their chunk sums [n / 256] | ksd2
struct SteinKsdWs {
    int64_t* counter;
    double *ginv, *x, *b, *g, *part, *rs, *csum, *fksd2;
    void lay(Carver<int64_t>& c, int64_t n, int64_t d, int64_t dp, int64_t chunks, int64_t slab) {
        counter = c.take<int64_t>(1);
        ginv = c.take<double>(d * d);
        x = c.take<double>(n * dp);
        b = c.take<double>(n * dp);
        g = c.take<double>(n * dp);
        part = c.take<double>(chunks * slab);
        rs = c.take<double>(n);
        csum = c.take<double>(stein_ceil(n, STEIN_ROW_CHUNK));
        fksd2 = c.take<double>(1);
    }
};

}  // namespace gpb
