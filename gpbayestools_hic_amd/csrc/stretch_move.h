// stretch_move.h — the device functions of the emcee-equivalent stretch move (src/mcmc.py:68-92,372-412): the red/blue split,
// a walker slot's proposal, its gather into the compacted batch and its accept decision.  Shared by the kernels of one ensemble
// (gpb_stretch.hip) and of K independent ensembles in one batch (gpb_sets.hip): one copy of the arithmetic and of the draws.
#pragma once
#include "gpb_internal.h"
#include "philox.h"
#include <math.h>

namespace gpb {

// ---- red/blue split ----------------------------------------------------------------------------------
// emcee's RedBlueMove shuffles which walkers form the two halves at every step (randomize_split=True,
// its default).  Here the shuffle is a keyed pseudo-random permutation pi_step of [0, n) that every
// thread (and every rank) can evaluate for a single index without communication or sorting: a 4-round
// Feistel network on 2*hb >= log2(n) bits with cycle walking.  Walker k of half h is pi(2k + h); with
// randomize = 0, pi is the identity (emcee's inds = arange(n) % 2).
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
struct SplitPerm {
    uint32_t n, hb, k0, k1, on;
    __device__ __forceinline__ int64_t operator()(int64_t i) const {
        if (!on) return i;
        const uint32_t mask = (1u << hb) - 1u;
        uint32_t x = (uint32_t)i;
        do {
            uint32_t L = x >> hb, R = x & mask;
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) {
                const uint32_t F = mix32(R ^ (k0 + r * 0x9E3779B9u)) ^ mix32(k1 + r);
                const uint32_t t = L ^ (F & mask);
                L = R;
                R = t;
            }
            x = (L << hb) | R;
        } while (x >= n);                      // cycle walking keeps it a bijection on [0, n)
        return (int64_t)x;
    }
    // the inverse map: rounds backwards (a round takes (L, R) to (R, L ^ F(R))), cycle walking likewise
    __device__ __forceinline__ int64_t inv(int64_t i) const {
        if (!on) return i;
        const uint32_t mask = (1u << hb) - 1u;
        uint32_t x = (uint32_t)i;
        do {
            uint32_t L = x >> hb, R = x & mask;
#pragma unroll
            for (int r = 3; r >= 0; --r) {
                const uint32_t F = mix32(L ^ (k0 + (uint32_t)r * 0x9E3779B9u)) ^ mix32(k1 + (uint32_t)r);
                const uint32_t t = R ^ (F & mask);
                R = L;
                L = t;
            }
            x = (L << hb) | R;
        } while (x >= n);
        return (int64_t)x;
    }
};
__device__ __forceinline__ SplitPerm make_perm(uint64_t seed, uint32_t step, int64_t n, int hb, int randomize) {
    const U4 k = philox(seed, 0xFFFFFFFFu, step, 0u, 7u);
    return SplitPerm{(uint32_t)n, (uint32_t)hb, k.x, k.y, (uint32_t)randomize};
}

// A slot of the compacted batch for every walker of the workgroup that asks for one (`want`, set in the walker's lane t0 = 0):
// ONE atomic per workgroup — 2048 walkers taking their slots from one counter one by one serialised on the atomic's return
// (k_accept_propose 18 us at 2048 rows a batch against 8 at 256).  The order of the slots does not matter (a row's result
// does not depend on its place in the batch).  Barriers: only in workgroups whose every thread has a walker (`full`, uniform
// per workgroup); the ensemble's last, partly filled workgroup takes the slots walker by walker.  Returns the slot in the
// lane t0 = 0 that asked (-1 elsewhere).
__device__ __forceinline__ int take_slot(bool want, bool full, int* __restrict__ cmp) {
    __shared__ int s_want[32], s_base;                 // up to 1024 threads = 32 walkers per workgroup
    if (!full) return want ? atomicAdd(cmp, 1) : -1;
    const int wl = (int)(threadIdx.x >> 5), nw = (int)(blockDim.x >> 5);
    if ((threadIdx.x & 31) == 0) s_want[wl] = want ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int i = 0; i < nw; ++i) tot += s_want[i];
        s_base = tot ? atomicAdd(cmp, tot) : 0;
    }
    __syncthreads();
    if (!want) return -1;
    int off = 0;
    for (int i = 0; i < wl; ++i) off += s_want[i];
    return s_base + off;
}

// The walkers and the generator of an ensemble: what every kernel of the move needs.
struct Ensemble {
    int64_t nhalf;
    int d;
    uint64_t seed;
    int hb, randomize;                 // make_perm
};

// Optional prior-box test in the proposal kernels; a zero-initialised instance (lo == nullptr): none.  The C-driven loop over
// a compacted chain takes the test of the rows [r0, r0 + chunk) — this rank's rows of the batch — on the proposal still in
// registers (strict inequalities, src/mcmc.py:275): ll[k] = outside for the rows outside, and either flags[k - r0] = 1 inside /
// 0 outside (k_compact_gather or k_balance_gather then ranks the flags and k_compact_mark's launch is saved: 7.6 of a sharded
// half-step's 166 us), or, with Xc, the rows inside are gathered here as well: a slot from a counter (cmp[0], zeroed by the
// accept kernel), in whatever order the walkers arrive — a row's result does not depend on its place in the batch.
struct ProposeBox {
    const double *lo, *hi;             // [d]
    double outside;
    double* ll;                        // [nhalf], optional
    int* flags;                        // [chunk], optional
    int64_t r0, chunk;
    double* Xc;                        // [chunk][d] gathered rows, optional; with cmp: [0] = count, [4..] = rows
    int* cmp;
};

// The row of walker slot k, found inside the box, goes to a slot of the compacted batch: the two parameters a lane holds
// (all of them for d <= 64) from registers.  Chains with more than 64 parameters (parameterTrafoPCA: the chain's ndim is the
// map's d_in, which only the GPs' reduced d bounds): the same arithmetic again, operation for operation.
__device__ __forceinline__ void gather_inside(bool want, bool full, int row, int t0, int d, const double (&v2)[2],
                                              const double* c, const double* s, double zz, double* Xc, int* cmp) {
#pragma clang fp contract(off)
    int slot = take_slot(want, full, cmp);
    if (slot >= 0) cmp[4 + slot] = row;
    slot = __shfl(slot, (int)(threadIdx.x & 32), 64);
    if (slot < 0) return;
    if (t0 < d) Xc[(int64_t)slot * d + t0] = v2[0];
    if (t0 + 32 < d) Xc[(int64_t)slot * d + t0 + 32] = v2[1];
    for (int t = t0 + 64; t < d; t += 32) Xc[(int64_t)slot * d + t] = c[t] - (c[t] - s[t]) * zz;
}

// The proposal of walker slot k for (step, half); current(w) = the position of walker w the proposal starts from.
// (box by value: through a reference k_accept_propose spills two scalar registers)
// 32 lanes per walker (one parameter each): these kernels sit between the log-probability batches of a
// step, so they are organised for latency, not for thread economy — every lane redoes the walker's draws
template <class Current>
__device__ __forceinline__ void propose_slot(const Ensemble& en, int64_t k, int t0, int half, uint32_t step, double a,
                                             double* q, double* factor, const ProposeBox box, Current current) {
#pragma clang fp contract(off)       // emcee's arithmetic rounds every product: no fused multiply-adds in here
    const int64_t nhalf = en.nhalf;
    const int d = en.d;
    const bool full = ((int64_t)(blockIdx.x + 1) * blockDim.x) >> 5 <= nhalf;      // every thread of this workgroup has a walker
    const SplitPerm pi = make_perm(en.seed, step, 2 * nhalf, en.hb, en.randomize);
    const U4 r = philox(en.seed, (uint32_t)k, step, (uint32_t)half, 0u);
    const double u = u01(r.x, r.y);
    // emcee StretchMove.get_proposal, operation for operation:
    //   zz = ((a - 1) * u + 1) ** 2 / a ;  q = c - (c - s) * zz ;  factor = (ndim - 1) * log(zz)
    const double zs = (a - 1.0) * u + 1.0;
    const double zz = (zs * zs) / a;
    const int64_t j = (int64_t)(((uint64_t)r.z * (uint64_t)nhalf) >> 32);
    const double* s = current(pi(2 * k + half));
    const double* c = current(pi(2 * j + (1 - half)));
    int ok = 1;
    double v2[2] = {0.0, 0.0};                         // the first two parameters of this lane (all of them for d <= 64)
    int nv = 0;
    for (int t = t0; t < d; t += 32) {
        const double v = c[t] - (c[t] - s[t]) * zz;
        q[k * d + t] = v;
        if (box.lo) ok &= (int)(v > box.lo[t]) & (int)(v < box.hi[t]);
        if (nv < 2) v2[nv] = v;
        ++nv;
    }
    if (t0 == 0) factor[k] = (d - 1.0) * log(zz);
    if (!box.lo) return;                               // wave-uniform; a walker's 32 lanes are one half of a wave
    const unsigned long long out = __ballot(!ok);
    const bool in = (((threadIdx.x & 32) ? (out >> 32) : out) & 0xffffffffull) == 0ull;
    const bool mine = k >= box.r0 && k < box.r0 + box.chunk;
    if (t0 == 0 && mine) {
        if (box.flags) box.flags[k - box.r0] = in ? 1 : 0;
        if (!in && box.ll) box.ll[k] = box.outside;
    }
    if (box.Xc) gather_inside(t0 == 0 && mine && in, full, (int)(k - box.r0), t0, d, v2, c, s, zz, box.Xc, box.cmp);
}

// Where the accept step finds a proposal's log-probability.  Plain (rank_of == nullptr): lpq[slot].  Balanced sharding (see
// k_balance_gather): lpq is the all-gathered array of the ranks' padded slices, a proposal inside the box is found through
// its position g in the ordered list of all live rows — slice g / per, entry g % per — and one outside the box has
// `outside` without a memory access.
struct LpSource {
    const double* lpq;
    const int* rank_of;                // null: plain
    const int* meta;                   // [0] = live rows in the whole batch, [1] = rows per slice
    int64_t chunk;                     // slice stride in lpq
    double outside;
    __device__ __forceinline__ double at(int64_t slot) const {
        if (!rank_of) return lpq[slot];
        const int g = rank_of[slot];
        if (g < 0) return outside;
        const int per = meta[1];
        return lpq[(int64_t)(g / per) * chunk + (g % per)];
    }
};

// The counter of a finished batch's rows inside the box (premark 2; cmp == nullptr: none).  The batch's kernels are done
// with it (stream order): the accept kernel reports it (tile-shape rule of the next launches, profile counter) and re-arms
// it for the next proposal kernel.
struct BatchCount {
    int* cmp;
    unsigned long long* hint;          // optional
    int64_t W_batch;
    unsigned long long* rows_live;     // optional
    __device__ __forceinline__ void report_and_rearm() const {
        const int cnt = cmp[0];
        if (hint) __hip_atomic_store(hint, ((unsigned long long)W_batch << 32) | (unsigned long long)cnt, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_SYSTEM);
        if (rows_live) atomicAdd(rows_live, (unsigned long long)cnt);
        cmp[0] = 0;
    }
};

// The accept decision of walker slot `slot` (walker idx) of a half-step whose proposals q / factor / lpq are in: every lane
// that asks takes the same decision from lp_in[idx].
struct PendingAccept {
    const double *q, *factor, *lp_in;
    LpSource lpq;
    uint64_t seed;
    uint32_t step;
    int half;
};
__device__ __forceinline__ bool accept_decision(const PendingAccept& A, int64_t slot, int64_t idx, double& lpq_k) {
#pragma clang fp contract(off)
    const U4 r = philox(A.seed, (uint32_t)slot, A.step, (uint32_t)A.half, 1u);
    const double u = u01(r.x, r.y);
    lpq_k = A.lpq.at(slot);
    const double diff = (A.factor[slot] + lpq_k) - A.lp_in[idx];
    return diff > log(u);                                            // emcee RedBlueMove.propose: f + nlp - lp[j] > log(rand)
}

// bits of one half of the Feistel network over [0, n) (make_perm's hb)
inline int half_bits(int64_t n) {
    int b = 1;
    while ((1ll << b) < n) ++b;
    return (b + 1) / 2;
}

}  // namespace gpb
