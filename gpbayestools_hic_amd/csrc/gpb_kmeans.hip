// gpb_kmeans.hip — posterior clusters of a resident chain (gpb_chain_kmeans): weighted k-means (Lloyd's iteration, sklearn's loop
// and stopping rule) of the standardised rows of a chain that lies in HBM, R restarts in lock-step, read through its strides as
// gpb_chain_marginals reads it.  z = (x - mean) / scale is formed on the fly in every pass; no standardised copy is stored.
//   k_km_weff        a lane per row: its effective weight (-1 a row with a non-finite coordinate, else its weight, 1 without)
//   k_km_moments     a lane per (row, column), the column fixed per lane: sum w (x - m), sum w (x - m)^2, sum w |x - m|, min, max
//                    per column and workgroup, compensated and in a fixed order; k_km_moments_final adds the workgroups in order
//   k_km_seed_sums   k-means++: per workgroup and restart the sum of w D (D = squared distance to the nearest centre chosen so
//                    far), strictly sequential inside a wave, then over the waves of a tile, the tiles of a workgroup
//   k_km_seed_pick   one thread per restart: the workgroups in order, the first whose running sum exceeds u * total
//   k_km_seed_find   a workgroup per restart rescans that range in the same order and takes the first row that exceeds
//   k_km_assign      a pass of Lloyd's iteration for a group of restarts whose centres fit the LDS: a lane per row finds the nearest
//                    centre of every restart (the row in registers, the centres broadcast from LDS); then a lane per (row, column)
//                    adds llrint(z w 2^F) to its centre's 64-bit LDS sum — the lanes of a wave spread over the columns, so equal
//                    labels meet in one address 64 / d times at most —, flushed once per workgroup with global integer atomics
//   k_km_update      a workgroup per restart: the centres from the integer sums, the summed squared shift in a fixed order, the
//                    stopping rule, the counters of the next pass
// Every sum that reaches a result is an integer add or runs in an order fixed by S alone: equal inputs give equal bits, a
// restart's bits do not depend on the restarts that share the call, and (seeding apart, which counts the rows in their order)
// not on the layout.  DESIGN.md section 23 has the error bound of the quantisation.
#include "block_reduce.h"
#include "gpb_internal.h"

namespace gpb {

namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_MAX_K = 32, KM_MAX_R = 16;
constexpr int KM_LDS_BYTES = 56 << 10;           // dynamic LDS of an assignment workgroup: centres and integer sums of its restarts
constexpr int KM_NMOM = 5;                       // s1 | s2 | sabs | min | max, then the weight sum
constexpr unsigned char KM_NONE = 255;           // label of a skipped row, and of every row before the first pass
constexpr int KM_CADENCE = 4;                    // iterations between two looks at the done flags (changes no result)
typedef unsigned long long u64;
typedef int64_t i64;
static_assert(KM_THREADS == REDUCE_THREADS, "k_km_update sums with block_sum");

// gpb_marg.hip's MargGeom: sample G (counted outer axis first) is o = G / n_in, i = G % n_in, element j at x[o so + i si + j]
struct KmGeom {
    int64_t so, si;
    unsigned n_in;
};
__device__ __forceinline__ const double* km_row(const double* x, const KmGeom& g, int64_t G) {
    const int64_t o = G / g.n_in, i = G - o * g.n_in;
    return x + o * g.so + i * g.si;
}

__device__ __forceinline__ i64 wave_sum_i64(i64 v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void lds_add(u64* p, i64 v) { atomicAdd(p, (u64)v); }

// counters: [0] rows skipped (a non-finite coordinate) | [1] rows of positive weight | [2] weights that are negative or not finite
__global__ __launch_bounds__(KM_THREADS) void k_km_weff(const double* __restrict__ x, KmGeom g, int d, int64_t S,
                                                        const double* __restrict__ w, double* __restrict__ weff,
                                                        u64* __restrict__ counters) {
    const int64_t G = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
    int skipped = 0, pos = 0, bad = 0;
    if (G < S) {
        const double* p = km_row(x, g, G);
        bool fin = true;
        for (int j = 0; j < d; ++j) fin = fin && isfinite(p[j]);
        const double wi = w ? w[G] : 1.0;
        double e = 0.0;
        if (!(wi >= 0.0) || !isfinite(wi)) bad = 1;
        else if (!fin) { e = -1.0; skipped = 1; }
        else if (wi > 0.0) { e = wi; pos = 1; }
        weff[G] = e;
    }
    const int ns = __popcll(__ballot(skipped)), np = __popcll(__ballot(pos)), nb = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (ns) atomicAdd(&counters[0], (u64)ns);
        if (np) atomicAdd(&counters[1], (u64)np);
        if (nb) atomicAdd(&counters[2], (u64)nb);
    }
}

// part [nb][KM_NMOM d + 1]; shift [d] or nullptr (zeros).  Lane tid < (256 / d) d serves column tid % d of the rows tid / d,
// tid / d + 256 / d, ... of its workgroup's range; the lanes of a column are added in order.
__global__ __launch_bounds__(KM_THREADS) void k_km_moments(const double* __restrict__ x, KmGeom g, int d, int64_t S,
                                                           const double* __restrict__ weff, const double* __restrict__ shift,
                                                           int64_t per_block, double* __restrict__ part) {
    __shared__ double sh[KM_NMOM + 1][KM_THREADS];
    const int tid = threadIdx.x, rp = KM_THREADS / d;
    const int64_t b0 = (int64_t)blockIdx.x * per_block, b1 = imin64(S, b0 + per_block);
    Kahan s1, s2, sa, sw;
    double mn = INFINITY, mx = -INFINITY;
    if (tid < rp * d) {
        const int j = tid % d;
        const double m = shift ? shift[j] : 0.0;
        for (int64_t row = b0 + tid / d; row < b1; row += rp) {
            const double w = weff[row];
            if (!(w > 0.0)) continue;
            const double xv = km_row(x, g, row)[j], v = xv - m;
            s1.add(w * v);
            s2.add(w * v * v);
            sa.add(w * fabs(v));
            mn = fmin(mn, xv);
            mx = fmax(mx, xv);
            if (j == 0) sw.add(w);
        }
    }
    sh[0][tid] = s1.s, sh[1][tid] = s2.s, sh[2][tid] = sa.s, sh[3][tid] = mn, sh[4][tid] = mx, sh[5][tid] = sw.s;
    __syncthreads();
    double* out = part + (int64_t)blockIdx.x * (KM_NMOM * d + 1);
    for (int t = tid; t < KM_NMOM * d + 1; t += KM_THREADS) {
        const int q = t / d, j = t - q * d;                      // (t == 5 d: q = 5, j = 0, the weights)
        double a = sh[q][j];
        for (int m = 1; m < rp; ++m) {
            const double v = sh[q][j + m * d];
            a = q == 3 ? fmin(a, v) : q == 4 ? fmax(a, v) : a + v;
        }
        out[t] = a;
    }
}

__global__ __launch_bounds__(KM_THREADS) void k_km_moments_final(const double* __restrict__ part, int64_t nb, int d,
                                                                 double* __restrict__ mom) {
    const int n = KM_NMOM * d + 1;
    for (int t = threadIdx.x; t < n; t += KM_THREADS) {
        const int q = t / d;
        Kahan a;
        double m = q == 3 ? INFINITY : -INFINITY;
        for (int64_t b = 0; b < nb; ++b) {
            const double v = part[b * n + t];
            if (q == 3) m = fmin(m, v);
            else if (q == 4) m = fmax(m, v);
            else a.add(v);
        }
        mom[t] = (q == 3 || q == 4) ? m : a.s;
    }
}

// the standardised row of a lane, padded with zeros to DP
template <int DP>
__device__ __forceinline__ void km_load_z(const double* __restrict__ p, const double* __restrict__ ms, int d, double (&z)[DP]) {
#pragma unroll
    for (int j = 0; j < DP; ++j) z[j] = j < d ? (p[j] - ms[j]) / ms[d + j] : 0.0;
}

// the nearest of nc centres (LDS, [nc][DP], padded with zeros): the lowest index wins a tie
template <int DP>
__device__ __forceinline__ void km_nearest(const double (&z)[DP], const double* cen, int nc, int& best, double& dmin) {
    best = 0;
    dmin = INFINITY;
    for (int c = 0; c < nc; ++c) {
        const double* cc = cen + c * DP;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < DP; ++j) {
            const double t = z[j] - cc[j];
            s = fma(t, t, s);
        }
        if (s < dmin) {
            dmin = s;
            best = c;
        }
    }
}

// the first nc centres of restarts [r0, r0 + nr) from cen_g [R][k][d] to LDS [nr][k][DP]
template <int DP>
__device__ __forceinline__ void km_load_centres(const double* __restrict__ cen_g, int r0, int nr, int k, int nc, int d, double* cen_s) {
    for (int t = threadIdx.x; t < nr * k * DP; t += KM_THREADS) {
        const int j = t % DP, c = (t / DP) % k, rl = t / (DP * k);
        cen_s[t] = (j < d && c < nc) ? cen_g[((int64_t)(r0 + rl) * k + c) * d + j] : 0.0;
    }
}

// the sum of v over the wave, lane 0 first, one add after the other; pref: the sum up to and including this lane
__device__ __forceinline__ double wave_seq_sum(double v, double& pref) {
    const int lane = threadIdx.x & 63;
    double a = 0.0;
    pref = 0.0;
    for (int l = 0; l < 64; ++l) {
        a += __shfl(v, l, 64);
        if (l == lane) pref = a;
    }
    return a;
}

// ---------------------------------------------------------------------------------------------------------------- seeding
// blockIdx.x: the rows [b per_block, (b + 1) per_block); blockIdx.y: RG restarts.  bs [R][nb]: the range's sum of w D against
// the first nc centres of every restart (nc == 0: D = 1).
template <int DP>
__global__ __launch_bounds__(KM_THREADS) void k_km_seed_sums(const double* __restrict__ x, KmGeom g, int d, int64_t S,
                                                             const double* __restrict__ weff, const double* __restrict__ ms,
                                                             const double* __restrict__ cen_g, int k, int R, int RG, int nc,
                                                             int64_t per_block, double* __restrict__ bs) {
    extern __shared__ double km_lds[];
    __shared__ double sw[KM_MAX_R][4], run[KM_MAX_R];
    double* cen_s = km_lds;
    const int tid = threadIdx.x, r0 = blockIdx.y * RG, nr = min(RG, R - r0);
    km_load_centres<DP>(cen_g, r0, nr, k, nc, d, cen_s);
    if (tid < nr) run[tid] = 0.0;
    __syncthreads();
    const int64_t b0 = (int64_t)blockIdx.x * per_block, b1 = imin64(S, b0 + per_block);
    for (int64_t t0 = b0; t0 < b1; t0 += KM_THREADS) {
        const int64_t row = t0 + tid;
        const double w = row < b1 ? weff[row] : 0.0;
        double z[DP];
        if (w > 0.0 && nc > 0) km_load_z<DP>(km_row(x, g, row), ms, d, z);
        for (int rl = 0; rl < nr; ++rl) {
            double v = 0.0, pref;
            if (w > 0.0) {
                v = w;
                if (nc > 0) {
                    int best;
                    double dmin;
                    km_nearest<DP>(z, cen_s + rl * k * DP, nc, best, dmin);
                    v = w * dmin;
                }
            }
            const double tot = wave_seq_sum(v, pref);
            if ((tid & 63) == 0) sw[rl][tid >> 6] = tot;
        }
        __syncthreads();
        if (tid < nr) run[tid] += ((sw[tid][0] + sw[tid][1]) + sw[tid][2]) + sw[tid][3];
        __syncthreads();
    }
    if (tid < nr) bs[(int64_t)(r0 + tid) * gridDim.x + blockIdx.x] = run[tid];
}

// thread r: target = u[r][c] * total; selb[r] = the first range whose running sum exceeds it (-1: the total is 0), selv[r] =
// (the running sum in front of it, the target)
__global__ void k_km_seed_pick(const double* __restrict__ bs, int64_t nb, int R, int k, int c, const double* __restrict__ u,
                               int* __restrict__ selb, double* __restrict__ selv) {
    const int r = threadIdx.x;
    if (r >= R) return;
    const double* b = bs + (int64_t)r * nb;
    double total = 0.0;
    for (int64_t i = 0; i < nb; ++i) total += b[i];
    if (!(total > 0.0)) {
        selb[r] = -1;
        return;
    }
    const double t = u[r * k + c] * total;
    double cum = 0.0, base = 0.0, lastbase = 0.0;
    int64_t sel = -1, lastpos = -1;
    for (int64_t i = 0; i < nb; ++i) {
        if (b[i] > 0.0) {
            lastpos = i;
            lastbase = cum;
        }
        if (cum + b[i] > t) {
            sel = i;
            base = cum;
            break;
        }
        cum += b[i];
    }
    double tt = t;
    if (sel < 0) {                                  // u * total rounded up to the total: the last range that holds weight,
        sel = lastpos;                              // its first row that adds to the sum
        base = lastbase;
        tt = -1.0;
    }
    selb[r] = (int)sel;
    selv[2 * r] = base;
    selv[2 * r + 1] = tt;
}

// blockIdx.x = r: centre c of restart r is the first row of range selb[r] whose running sum exceeds the target, in
// k_km_seed_sums' order; seed [R][k] takes its index, cen_g [r][c][:] its standardised coordinates.
template <int DP>
__global__ __launch_bounds__(KM_THREADS) void k_km_seed_find(const double* __restrict__ x, KmGeom g, int d, int64_t S,
                                                             const double* __restrict__ weff, const double* __restrict__ ms,
                                                             double* __restrict__ cen_g, int k, int c, int64_t per_block,
                                                             const int* __restrict__ selb, const double* __restrict__ selv,
                                                             i64* __restrict__ seed) {
    extern __shared__ double km_lds[];
    __shared__ double sw[4];
    __shared__ int found;
    __shared__ i64 pick;
    double* cen_s = km_lds;
    const int tid = threadIdx.x, r = blockIdx.x, nc = c;
    const int b = selb[r];
    if (tid == 0) pick = b < 0 ? (c > 0 ? seed[r * k + c - 1] : 0) : -1;      // (no weight left: the centre chosen before, again)
    km_load_centres<DP>(cen_g, r, 1, k, nc, d, cen_s);
    if (tid == 0) found = KM_THREADS;
    __syncthreads();
    if (b >= 0) {
        const double base = selv[2 * r], t = selv[2 * r + 1];
        const int64_t b0 = (int64_t)b * per_block, b1 = imin64(S, b0 + per_block);
        double run = 0.0;
        for (int64_t t0 = b0; t0 < b1; t0 += KM_THREADS) {
            const int64_t row = t0 + tid;
            const double w = row < b1 ? weff[row] : 0.0;
            double v = 0.0, pref;
            if (w > 0.0) {
                v = w;
                if (nc > 0) {
                    double z[DP];
                    int best;
                    double dmin;
                    km_load_z<DP>(km_row(x, g, row), ms, d, z);
                    km_nearest<DP>(z, cen_s, nc, best, dmin);
                    v = w * dmin;
                }
            }
            const double tot = wave_seq_sum(v, pref);
            if ((tid & 63) == 0) sw[tid >> 6] = tot;
            __syncthreads();
            const int wv = tid >> 6;
            const double pw = wv == 0 ? 0.0 : wv == 1 ? sw[0] : wv == 2 ? sw[0] + sw[1] : (sw[0] + sw[1]) + sw[2];
            if (v > 0.0 && base + (run + (pw + pref)) > t) atomicMin(&found, tid);
            run += ((sw[0] + sw[1]) + sw[2]) + sw[3];
            __syncthreads();
            if (found < KM_THREADS) {
                if (tid == 0) pick = t0 + found;
                break;
            }
        }
    }
    __syncthreads();
    const i64 row = pick;
    if (tid == 0) seed[r * k + c] = row;
    if (row >= 0 && tid < d) {
        const double* p = km_row(x, g, row);
        cen_g[((int64_t)r * k + c) * d + tid] = (p[tid] - ms[tid]) / ms[d + tid];
    }
}

// ---------------------------------------------------------------------------------------------------------------- Lloyd
struct KmState {
    double *cen, *shift;           // [R][k][d] standardised centres | [R] the last summed squared shift
    i64 *acc, *wq, *cnt, *iner;    // [R][k][d] sums of llrint(z w 2^F) | [R][k] of llrint(w 2^G) | [R][k] rows | [R] of llrint(w D 2^FI)
    int *changed, *done, *conv, *niter, *fi;      // [R] each
};

// blockIdx.x: a range of rows; blockIdx.y: RG restarts.  final == 0: a pass of the iteration for the restarts that are not done
// (labels, changed, acc, wq, cnt).  final == 1: the last assignment of every restart (labels, wq, cnt, iner).
template <int DP>
__global__ __launch_bounds__(KM_THREADS) void k_km_assign(const double* __restrict__ x, KmGeom g, int d, int64_t S,
                                                          const double* __restrict__ weff, const double* __restrict__ ms, KmState st,
                                                          unsigned char* __restrict__ lab, int k, int R, int RG, int F, int Gq,
                                                          int final, int64_t per_block) {
    extern __shared__ double km_lds[];
    __shared__ u64 iner_s[KM_MAX_R];
    __shared__ int chg_s[KM_MAX_R], act[KM_MAX_R], nact;
    __shared__ unsigned char lab_s[KM_MAX_R][KM_THREADS];
    const int tid = threadIdx.x, r0 = blockIdx.y * RG, nr = min(RG, R - r0);
    double* cen_s = km_lds;                                       // [nr][k][DP]
    u64* acc_s = reinterpret_cast<u64*>(cen_s + nr * k * DP);      // [nr][k][d]
    u64* wq_s = acc_s + nr * k * d;                               // [nr][k]
    u64* cnt_s = wq_s + nr * k;                                   // [nr][k]
    if (tid == 0) nact = 0;
    __syncthreads();
    if (tid < nr) {
        act[tid] = final || !st.done[r0 + tid];
        iner_s[tid] = 0;
        chg_s[tid] = 0;
        if (act[tid]) atomicAdd(&nact, 1);
    }
    __syncthreads();
    if (!nact) return;                                            // (uniform)
    km_load_centres<DP>(st.cen, r0, nr, k, k, d, cen_s);
    for (int t = tid; t < nr * k * (d + 2); t += KM_THREADS) acc_s[t] = 0;
    __syncthreads();
    const int64_t b0 = (int64_t)blockIdx.x * per_block, b1 = imin64(S, b0 + per_block);
    for (int64_t t0 = b0; t0 < b1; t0 += KM_THREADS) {
        {                                                         // a lane per row: the nearest centre of every restart
            const int64_t row = t0 + tid;
            const double w = row < b1 ? weff[row] : -1.0;
            double z[DP];
            if (w >= 0.0) km_load_z<DP>(km_row(x, g, row), ms, d, z);
            for (int rl = 0; rl < nr; ++rl) {
                if (!act[rl]) continue;
                int best = KM_NONE;
                double dmin = 0.0;
                if (w >= 0.0) km_nearest<DP>(z, cen_s + rl * k * DP, k, best, dmin);
                lab_s[rl][tid] = (unsigned char)best;
                if (row < b1) {
                    unsigned char* lp = lab + (int64_t)(r0 + rl) * S + row;
                    if (w > 0.0 && *lp != (unsigned char)best) chg_s[rl] = 1;
                    *lp = (unsigned char)best;
                }
                if (final) {
                    const i64 q = wave_sum_i64(w > 0.0 ? (i64)llrint(ldexp(w * dmin, st.fi[r0 + rl])) : (i64)0);
                    if ((tid & 63) == 0 && q) lds_add(&iner_s[rl], q);
                }
            }
        }
        __syncthreads();
        const int nrows = (int)imin64(KM_THREADS, b1 - t0);
        if (!final) {                                             // a lane per (row, column): the integer sums of the centres
            for (int e = tid; e < nrows * d; e += KM_THREADS) {
                const int row = e / d, j = e - row * d;
                const double w = weff[t0 + row];
                if (!(w > 0.0)) continue;
                const double zz = (km_row(x, g, t0 + row)[j] - ms[j]) / ms[d + j];
                const i64 q = llrint(ldexp(zz * w, F));
                for (int rl = 0; rl < nr; ++rl)
                    if (act[rl]) lds_add(&acc_s[(rl * k + lab_s[rl][row]) * d + j], q);
            }
        }
        if (tid < nrows) {
            const double w = weff[t0 + tid];
            if (w > 0.0) {
                const i64 qw = llrint(ldexp(w, Gq));
                for (int rl = 0; rl < nr; ++rl)
                    if (act[rl]) {
                        const int c = lab_s[rl][tid];
                        lds_add(&wq_s[rl * k + c], qw);
                        lds_add(&cnt_s[rl * k + c], 1);
                    }
            }
        }
        __syncthreads();
    }
    for (int t = tid; t < nr * k * d; t += KM_THREADS) {
        const int rl = t / (k * d);
        if (act[rl] && acc_s[t]) atomicAdd(reinterpret_cast<u64*>(st.acc) + (int64_t)r0 * k * d + t, acc_s[t]);
    }
    for (int t = tid; t < nr * k; t += KM_THREADS) {
        if (!act[t / k]) continue;
        if (wq_s[t]) atomicAdd(reinterpret_cast<u64*>(st.wq) + r0 * k + t, wq_s[t]);
        if (cnt_s[t]) atomicAdd(reinterpret_cast<u64*>(st.cnt) + r0 * k + t, cnt_s[t]);
    }
    if (tid < nr && act[tid]) {
        if (iner_s[tid]) atomicAdd(reinterpret_cast<u64*>(st.iner) + r0 + tid, iner_s[tid]);
        if (chg_s[tid]) atomicOr(&st.changed[r0 + tid], 1);
    }
}

// blockIdx.x = r, not done: centre (c, j) = acc / wq 2^(G - F) where the cluster holds weight, else as it was; the summed squared
// shift in a fixed order; sklearn's stopping rule; the sums and the changed flag are cleared for the next pass.
__global__ __launch_bounds__(KM_THREADS) void k_km_update(KmState st, int k, int d, int F, int Gq, double tolabs, int max_iter) {
    __shared__ double sw[REDUCE_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (st.done[r]) return;                                       // (uniform)
    Kahan s;
    for (int t = tid; t < k * d; t += KM_THREADS) {
        const int64_t at = (int64_t)r * k * d + t;
        const i64 wq = st.wq[r * k + t / d];
        if (wq > 0) {
            const double nv = ldexp((double)st.acc[at] / (double)wq, Gq - F), dv = nv - st.cen[at];
            s.add(dv * dv);
            st.cen[at] = nv;
        }
        st.acc[at] = 0;
    }
    const double shift = block_sum(s.s, sw);
    for (int t = tid; t < k; t += KM_THREADS) st.wq[r * k + t] = 0, st.cnt[r * k + t] = 0;
    if (tid == 0) {
        const int it = ++st.niter[r];
        const bool same = st.changed[r] == 0, small = shift <= tolabs;
        st.shift[r] = shift;
        st.changed[r] = 0;
        if (same || small) st.conv[r] = 1;
        if (same || small || it >= max_iter) st.done[r] = 1;
    }
}

__global__ __launch_bounds__(KM_THREADS) void k_km_labels(const unsigned char* __restrict__ lab, int64_t S, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
    if (i < S) out[i] = lab[i] == KM_NONE ? -1 : (int32_t)lab[i];
}

inline int km_exp(double v) {                                     // e with v < 2^e (v >= 0, finite)
    int e = 0;
    if (v > 0.0) frexp(v, &e);
    return e;
}

}  // namespace

}  // namespace gpb

using namespace gpb;

#define KM_ARG(msg) GPB_FAIL(GPB_E_ARG, "gpb_chain_kmeans: " msg)

extern "C" int gpb_chain_kmeans(gpb_ctx* ctx, const double* x_dev, int64_t nsteps, int64_t nwalkers, int64_t d, int64_t step_stride,
                                int64_t walker_stride, const double* w_dev, int k, int R, int max_iter, double tol, int standardize,
                                const double* init_host, const double* u_host, double* centers, double* inertia, int32_t* n_iter,
                                int32_t* converged, int64_t* size, double* wsum, double* mean, double* scale, int64_t* seed_index,
                                int32_t* best, int64_t* n_skipped, int32_t* labels_dev) {
    if (!ctx || !x_dev) return GPB_E_ARG;
    if (nsteps < 1 || nwalkers < 1 || d < 1) KM_ARG("need nsteps >= 1, nwalkers >= 1 and d >= 1");
    if (d > MAX_D) KM_ARG("d above 64");
    if (nsteps > 0x7fffffffLL || nwalkers > 0x7fffffffLL || (__int128)nsteps * nwalkers > 0x7fffffffLL)
        KM_ARG("more than 2^31 - 1 samples (nsteps nwalkers)");
    if (walker_stride < d || step_stride < d) KM_ARG("a stride below d (elements would alias)");
    const bool steps_outer = (__int128)step_stride >= (__int128)walker_stride * nwalkers;
    const bool walkers_outer = (__int128)walker_stride >= (__int128)step_stride * nsteps;
    if (!steps_outer && !walkers_outer) KM_ARG("neither stride spans the other axis (elements would alias)");
    if (w_dev && nwalkers != 1) KM_ARG("weights (w_dev) need nwalkers == 1 (a flat particle set)");
    if (k < 1 || k > KM_MAX_K) KM_ARG("k outside 1 .. 32");
    if (R < 1 || R > KM_MAX_R) KM_ARG("R outside 1 .. 16");
    if (max_iter < 1) KM_ARG("max_iter below 1");
    if (!(tol >= 0.0) || !isfinite(tol)) KM_ARG("tol must be finite and not negative");
    if (standardize != 0 && standardize != 1) KM_ARG("standardize must be 0 or 1");
    if ((init_host != nullptr) == (u_host != nullptr)) KM_ARG("exactly one of init_host and u_host must be given");
    if (init_host)
        for (int64_t t = 0; t < (int64_t)R * k * d; ++t)
            if (!isfinite(init_host[t])) KM_ARG("init_host must be finite");
    if (u_host)
        for (int t = 0; t < R * k; ++t)
            if (!(u_host[t] >= 0.0 && u_host[t] < 1.0)) KM_ARG("u_host must lie in [0, 1)");
    const int64_t S = nsteps * nwalkers;
    const int D = (int)d, DP = pick_dpad(d);
    GPB_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;

    // rows per workgroup: whole tiles of 256, a few workgroups per CU — a function of S and the device alone
    const int64_t tiles = (S + KM_THREADS - 1) / KM_THREADS;
    const int64_t nb_aim = imin64(tiles, 8 * (int64_t)ctx->num_cu);
    const int64_t per_block = (tiles + nb_aim - 1) / nb_aim * KM_THREADS;
    const int64_t nb = (S + per_block - 1) / per_block;
    // restarts per assignment workgroup: their centres and integer sums in LDS
    const int64_t per_restart = (int64_t)k * DP * 8 + (int64_t)k * (D + 2) * 8;
    const int RG = (int)imin64(R, KM_LDS_BYTES / per_restart);       // (k 64 16 + 32 16 bytes at most: >= 1)
    const int ngroups = (R + RG - 1) / RG;
    const size_t lds_assign = (size_t)(RG * per_restart), lds_seed = (size_t)RG * k * DP * 8, lds_find = (size_t)k * DP * 8;
    const int nmom = KM_NMOM * D + 1;

    KmeansWs ws;
    if (const int rc = ctx_carve(ctx, ctx->kmeans_ws, [&](Carver<int64_t>& c) { ws.lay(c, S, R, k, D, nb, u_host ? 1 : 0); })) return rc;
    KmState st{ws.cen, ws.shift, ws.acc, ws.wq, ws.cnt, ws.iner, ws.changed, ws.done, ws.conv, ws.niter, ws.fi};
    const KmGeom g = steps_outer ? KmGeom{step_stride, walker_stride, (unsigned)nwalkers} : KmGeom{walker_stride, step_stride, (unsigned)nsteps};
    const dim3 thr(KM_THREADS);
    const unsigned row_blocks = (unsigned)((S + KM_THREADS - 1) / KM_THREADS);

    // ---- 1. effective weights, moments
    GPB_HIP(hipMemsetAsync(ws.state0, 0, ws.state_bytes, s));
    hipLaunchKernelGGL(k_km_weff, dim3(row_blocks), thr, 0, s, x_dev, g, D, S, w_dev, ws.weff, reinterpret_cast<u64*>(ws.counters));
    int64_t counters[3];
    std::vector<double> m1(nmom), m2(nmom), ms(2 * D);
    hipLaunchKernelGGL(k_km_moments, dim3((unsigned)nb), thr, 0, s, x_dev, g, D, S, ws.weff, (const double*)nullptr, per_block, ws.part);
    hipLaunchKernelGGL(k_km_moments_final, dim3(1), thr, 0, s, ws.part, nb, D, ws.mom);
    GPB_HIP(hipMemcpyAsync(counters, ws.counters, sizeof(counters), hipMemcpyDeviceToHost, s));
    GPB_HIP(hipMemcpyAsync(m1.data(), ws.mom, sizeof(double) * nmom, hipMemcpyDeviceToHost, s));
    GPB_HIP(hipStreamSynchronize(s));
    if (counters[2]) KM_ARG("w_dev must hold finite, non-negative weights");
    if (counters[1] < k) KM_ARG("k above the number of rows with positive weight");
    const double W = m1[KM_NMOM * D];
    std::vector<double> mu(D), var(D), sc(D);
    for (int j = 0; j < D; ++j) mu[j] = m1[3 * D + j] == m1[4 * D + j] ? m1[3 * D + j] : m1[j] / W;
    GPB_HIP(hipMemcpyAsync(ws.ms, mu.data(), sizeof(double) * D, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_km_moments, dim3((unsigned)nb), thr, 0, s, x_dev, g, D, S, ws.weff, (const double*)ws.ms, per_block, ws.part);
    hipLaunchKernelGGL(k_km_moments_final, dim3(1), thr, 0, s, ws.part, nb, D, ws.mom);
    GPB_HIP(hipMemcpyAsync(m2.data(), ws.mom, sizeof(double) * nmom, hipMemcpyDeviceToHost, s));
    GPB_HIP(hipStreamSynchronize(s));
    double A = 0.0, Q = 0.0, varz = 0.0;       // max_j sum w |z_j| ; sum_ij w z_ij^2 ; sum_j var(z_j)
    for (int j = 0; j < D; ++j) {
        const bool constant = m1[3 * D + j] == m1[4 * D + j];
        const double c1 = m2[j] / W;
        var[j] = constant ? 0.0 : fmax(m2[D + j] / W - c1 * c1, 0.0);
        sc[j] = sqrt(var[j]);
        if (sc[j] == 0.0) sc[j] = 1.0;
        if (!isfinite(mu[j]) || !isfinite(sc[j])) KM_ARG("the moments of x_dev overflow");
        ms[j] = standardize ? mu[j] : 0.0;
        ms[D + j] = standardize ? sc[j] : 1.0;
        const double sabs = standardize ? m2[2 * D + j] : m1[2 * D + j], off = mu[j] - ms[j];
        A = fmax(A, sabs / ms[D + j]);
        Q += W * (var[j] + off * off) / (ms[D + j] * ms[D + j]);
        varz += var[j] / (ms[D + j] * ms[D + j]);
    }
    GPB_HIP(hipMemcpyAsync(ws.ms, ms.data(), sizeof(double) * 2 * D, hipMemcpyHostToDevice, s));
    const int F = 61 - km_exp(A), Gq = w_dev ? 61 - km_exp(W) : 0;
    const double tolabs = tol * (varz / D);

    // ---- 2. the starting centres
    std::vector<double> cen((size_t)R * k * D);
    if (init_host) {
        for (int64_t t = 0; t < (int64_t)R * k * D; ++t) cen[t] = (init_host[t] - ms[t % D]) / ms[D + t % D];
        GPB_HIP(hipMemcpyAsync(ws.cen, cen.data(), sizeof(double) * cen.size(), hipMemcpyHostToDevice, s));
    } else {
        GPB_HIP(hipMemcpyAsync(ws.u, u_host, sizeof(double) * R * k, hipMemcpyHostToDevice, s));
        for (int c = 0; c < k; ++c) {
            const int rc = dispatched(ctx, with_dpad(DP, [&](auto Wd) {
                constexpr int DPAD = decltype(Wd)::value;
                hipLaunchKernelGGL(k_km_seed_sums<DPAD>, dim3((unsigned)nb, (unsigned)ngroups), thr, lds_seed, s, x_dev, g, D, S, ws.weff,
                                   ws.ms, ws.cen, k, R, RG, c, per_block, ws.bs);
                hipLaunchKernelGGL(k_km_seed_pick, dim3(1), dim3(64), 0, s, ws.bs, nb, R, k, c, ws.u, ws.selb, ws.selv);
                hipLaunchKernelGGL(k_km_seed_find<DPAD>, dim3((unsigned)R), thr, lds_find, s, x_dev, g, D, S, ws.weff, ws.ms, ws.cen, k, c,
                                   per_block, ws.selb, ws.selv, ws.seed);
                return 0;
            }), "k_km_seed");
            if (rc) return rc;
        }
    }
    GPB_HIP(hipMemsetAsync(ws.lab, KM_NONE, (size_t)R * S, s));

    // ---- 3. Lloyd's iteration; the done flags are read every KM_CADENCE passes (a pass over done restarts changes nothing)
    auto assign = [&](int final) {
        return dispatched(ctx, with_dpad(DP, [&](auto Wd) {
            constexpr int DPAD = decltype(Wd)::value;
            hipLaunchKernelGGL(k_km_assign<DPAD>, dim3((unsigned)nb, (unsigned)ngroups), thr, lds_assign, s, x_dev, g, D, S, ws.weff, ws.ms,
                               st, ws.lab, k, R, RG, F, Gq, final, per_block);
            return 0;
        }), "k_km_assign");
    };
    std::vector<int> flags(5 * R);
    for (int it = 0; it < max_iter; ++it) {
        if (const int rc = assign(0)) return rc;
        hipLaunchKernelGGL(k_km_update, dim3((unsigned)R), thr, 0, s, st, k, D, F, Gq, tolabs, max_iter);
        if ((it + 1) % KM_CADENCE == 0 && it + 1 < max_iter) {
            GPB_HIP(hipMemcpyAsync(flags.data(), ws.done, sizeof(int) * R, hipMemcpyDeviceToHost, s));
            GPB_HIP(hipStreamSynchronize(s));
            bool all = true;
            for (int r = 0; r < R; ++r) all = all && flags[r];
            if (all) break;
        }
    }

    // ---- 4. the last assignment: labels, sizes, inertia (an integer sum: dmin <= 2 |z|^2 + 2 |c_0|^2 bounds it beforehand)
    GPB_HIP(hipMemcpyAsync(cen.data(), ws.cen, sizeof(double) * cen.size(), hipMemcpyDeviceToHost, s));
    GPB_HIP(hipStreamSynchronize(s));
    std::vector<int> fi(R);
    for (int r = 0; r < R; ++r) {
        double c2 = 0.0;
        for (int j = 0; j < D; ++j) c2 += cen[(size_t)r * k * D + j] * cen[(size_t)r * k * D + j];
        fi[r] = 61 - km_exp(2.0 * Q + 2.0 * W * c2);
    }
    GPB_HIP(hipMemcpyAsync(ws.fi, fi.data(), sizeof(int) * R, hipMemcpyHostToDevice, s));
    if (const int rc = assign(1)) return rc;
    std::vector<int64_t> ints((size_t)R * k * 3 + R);          // wq | cnt | seed | iner
    GPB_HIP(hipMemcpyAsync(ints.data(), ws.wq, sizeof(int64_t) * R * k, hipMemcpyDeviceToHost, s));
    GPB_HIP(hipMemcpyAsync(ints.data() + R * k, ws.cnt, sizeof(int64_t) * R * k, hipMemcpyDeviceToHost, s));
    if (u_host) GPB_HIP(hipMemcpyAsync(ints.data() + 2 * R * k, ws.seed, sizeof(int64_t) * R * k, hipMemcpyDeviceToHost, s));
    GPB_HIP(hipMemcpyAsync(ints.data() + 3 * R * k, ws.iner, sizeof(int64_t) * R, hipMemcpyDeviceToHost, s));
    GPB_HIP(hipMemcpyAsync(flags.data(), ws.changed, sizeof(int) * 5 * R, hipMemcpyDeviceToHost, s));      // changed | done | conv | niter | fi
    GPB_HIP(hipStreamSynchronize(s));
    int bestr = 0;
    double bestv = 0.0;
    for (int r = 0; r < R; ++r) {
        const double v = ldexp((double)ints[3 * R * k + r], -fi[r]);
        if (inertia) inertia[r] = v;
        if (r == 0 || v < bestv) bestr = r, bestv = v;
        if (n_iter) n_iter[r] = flags[3 * R + r];
        if (converged) converged[r] = flags[2 * R + r];
    }
    for (int t = 0; t < R * k; ++t) {
        if (wsum) wsum[t] = ldexp((double)ints[t], -Gq);
        if (size) size[t] = ints[R * k + t];
        if (seed_index) seed_index[t] = u_host ? ints[2 * R * k + t] : -1;
    }
    if (centers)
        for (int64_t t = 0; t < (int64_t)R * k * D; ++t) centers[t] = cen[t] * ms[D + t % D] + ms[t % D];
    for (int j = 0; j < D; ++j) {
        if (mean) mean[j] = ms[j];
        if (scale) scale[j] = ms[D + j];
    }
    if (best) *best = bestr;
    if (n_skipped) *n_skipped = counters[0];
    if (labels_dev) {
        hipLaunchKernelGGL(k_km_labels, dim3(row_blocks), thr, 0, s, ws.lab + (int64_t)bestr * S, S, labels_dev);
        GPB_HIP(hipStreamSynchronize(s));
    }
    GPB_HIP(hipGetLastError());
    return 0;
}
