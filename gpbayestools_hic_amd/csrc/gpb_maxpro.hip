// gpb_maxpro.hip — maximum-projection Latin-hypercube designs (gpb_maxpro_lhd, gpb_maxpro_criterion, gpb_maxpro_run_order): what
// the reference gets from R's MaxProRunOrder(MaxProLHD(n, p)$Design) (src/design.py).  maxpro_index.h has the quantities (pair
// terms t_ij, the objective f = ln sum t_ij, ln psi) and the decoding of a proposal; DESIGN.md section 24 the algorithm.
//   k_mp_build    a workgroup per (row i, restart): t_ij for every j from the columns (levels, or a real design), into the
//                 restart's pair matrix when one is given, and the row's sum over j > i in a fixed order
//   k_mp_total    a workgroup per restart: the row sums in a fixed order, into the slot of the state that the caller names
//   k_mp_anneal   a workgroup per restart runs a range of blocks: a wave per slot evaluates its proposal at the block's starting
//                 state (one pass over the rows a and b of the pair matrix and one column of levels), the first wave takes the first
//                 slot that passes (a lane per slot), the workgroup applies it (rows and columns a and b, the sum, the levels, the best so far)
//   k_mp_order    one workgroup: the greedy run order, a lane per row, the scores in registers
// No workgroup waits on another inside a kernel: the restarts are independent, and what orders the work is the launch boundary
// and __syncthreads.  The number of launches depends on the schedule alone, so the annealing is enqueued without a host sync.
// Every pair term and every ratio is a chain of IEEE multiplications and divisions with contraction off: the host restatement
// (tests/maxpro_reference.py) holds the same bits in its matrix, and differs only in the order of the sums.
#include "block_reduce.h"
#include "gpb_internal.h"
#include "maxpro_index.h"
#include "philox.h"

namespace gpb {

namespace {

constexpr int MP_BUILD_THREADS = REDUCE_THREADS;
constexpr int MP_THREADS = 1024, MP_WAVES = MP_THREADS / MP_WAVE;
constexpr int MP_ROWS_PER_LANE = MP_MAX_N / MP_THREADS;        // k_mp_order: the scores of a lane's rows stay in registers
constexpr int MP_CHUNK = 2048;                                 // blocks per k_mp_anneal launch at most
static_assert(MP_ROWS_PER_LANE * MP_THREADS == MP_MAX_N, "k_mp_order covers MP_MAX_N rows");
static_assert(MP_MAX_BLOCK <= 64 && MP_MAX_D <= MP_BUILD_THREADS, "LDS tables of k_mp_anneal / k_mp_build");

// cols [R][d][n] (a column contiguous); T [R][n][n] or nullptr; rowsum [R][n]
template <typename V>
__global__ __launch_bounds__(MP_BUILD_THREADS) void k_mp_build(const V* __restrict__ cols, int n, int d, double scale,
                                                               double* __restrict__ T, double* __restrict__ rowsum) {
#pragma clang fp contract(off)
    __shared__ V xi[MP_MAX_D];
    __shared__ double sw[REDUCE_WAVES];
    const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const V* c = cols + (int64_t)r * d * n;
    if (tid < d) xi[tid] = c[(int64_t)tid * n + i];
    __syncthreads();
    double acc = 0.0;
    for (int j = tid; j < n; j += MP_BUILD_THREADS) {
        double t = 0.0;
        if (j != i) {
            double p = 1.0;
            for (int l = 0; l < d; ++l) {
                const double q = scale * (double)(xi[l] - c[(int64_t)l * n + j]);
                p *= q * q;
            }
            t = 1.0 / p;
        }
        if (T) T[((int64_t)r * n + i) * n + j] = t;
        if (j > i) acc += t;
    }
    const double s = block_sum(acc, sw);
    if (tid == 0) rowsum[(int64_t)r * n + i] = s;
}

// sums [R][4]: the running sum | the best sum | the start's sum | the sum of the best levels.  what == 0: a start (the first three,
// and the counters cleared); 1: a stage's rebuild (the running sum); 2: the sum of the best levels
__global__ __launch_bounds__(MP_BUILD_THREADS) void k_mp_total(const double* __restrict__ rowsum, int n, int what,
                                                               double* __restrict__ sums, int64_t* __restrict__ counts) {
    __shared__ double sw[REDUCE_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x;
    Kahan a;
    for (int i = tid; i < n; i += MP_BUILD_THREADS) a.add(rowsum[(int64_t)r * n + i]);
    const double s = block_sum(a.s, sw);
    if (tid == 0) {
        double* o = sums + 4 * r;
        if (what == 0) {
            o[0] = o[1] = o[2] = s;
            counts[2 * r] = counts[2 * r + 1] = 0;
        } else if (what == 1) {
            o[0] = s;
        } else {
            o[3] = s;
        }
    }
}

struct MpRun {
    double *T, *sums;
    int64_t* counts;
    int *lev, *best, *trace;           // trace: [R][n_trace] or nullptr
};

// the change of the sum when column c is swapped between the rows a and b: row j's terms with a and b change by
// ((l_a - l_j) / (l_b - l_j))^2 and its inverse
__device__ __forceinline__ void mp_ratios(int la, int lb, int lj, double& ra, double& rb) {
#pragma clang fp contract(off)
    const double qa = (double)(la - lj), qb = (double)(lb - lj);
    const double fa = qa / qb, fb = qb / qa;
    ra = fa * fa;
    rb = fb * fb;
}

// blockIdx.x = r: the blocks [gb0, gb0 + nblocks) of restart restart0 + r at temperature temp
__global__ __launch_bounds__(MP_THREADS) void k_mp_anneal(MpRun st, int n, int d, int B, uint64_t seed, uint32_t restart0,
                                                          uint32_t gb0, int nblocks, int64_t n_trace, double temp) {
#pragma clang fp contract(off)
    __shared__ double sh_delta[MP_MAX_BLOCK], sh_lnu[MP_MAX_BLOCK];
    __shared__ int sh_c[MP_MAX_BLOCK], sh_a[MP_MAX_BLOCK], sh_b[MP_MAX_BLOCK];
    __shared__ int sh_pick, sh_improved;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & (MP_WAVE - 1), wave = tid / MP_WAVE;
    double* T = st.T + (int64_t)r * n * n;
    int* lev = st.lev + (int64_t)r * d * n;
    int* best = st.best + (int64_t)r * d * n;
    double S = 0.0, Sbest = 0.0;                                  // (the first wave's, the same in all its lanes)
    int64_t n_acc = 0, n_cons = 0;
    if (wave == 0) {
        S = st.sums[4 * r];
        Sbest = st.sums[4 * r + 1];
        n_acc = st.counts[2 * r];
        n_cons = st.counts[2 * r + 1];
    }
    for (int k = 0; k < nblocks; ++k) {
        const uint32_t gb = gb0 + (uint32_t)k;
        for (int slot = wave; slot < B; slot += MP_WAVES) {       // a wave per slot, every slot at the block's starting state
            const U4 w = philox(seed, gb, restart0 + (uint32_t)r, (uint32_t)slot, MP_TAG);
            const MpProposal p = mp_decode(w.x, w.y, w.z, w.w, n, d);
            const int* col = lev + (int64_t)p.c * n;
            const int la = col[p.a], lb = col[p.b];
            const double *Ta = T + (int64_t)p.a * n, *Tb = T + (int64_t)p.b * n;
            double acc = 0.0;
#pragma unroll 4
            for (int j = lane; j < n; j += MP_WAVE) {             // (no branch in the body: the loads of several rows are in flight)
                const int lj = col[j];
                const double ta = Ta[j], tb = Tb[j];
                double ra, rb;
                mp_ratios(la, lb, lj, ra, rb);
                const double term = ta * (ra - 1.0) + tb * (rb - 1.0);
                acc += (j == p.a || j == p.b) ? 0.0 : term;
            }
            acc = wave_sum(acc);
            if (lane == 0) {
                sh_delta[slot] = acc;
                sh_lnu[slot] = log(p.u);
                sh_c[slot] = p.c, sh_a[slot] = p.a, sh_b[slot] = p.b;
            }
        }
        __syncthreads();
        if (wave == 0) {                                          // the first slot that passes ln u < -(f' - f) / temp: a lane per slot
            bool pass = false;
            if (lane < B) {
                const double df = log1p(sh_delta[lane] / S);
                pass = sh_lnu[lane] < -df / temp;
            }
            const unsigned long long m = __ballot(pass);
            const int pick = m ? __ffsll((long long)m) - 1 : -1;
            int improved = 0;
            if (pick >= 0) {
                S = S + sh_delta[pick];
                ++n_acc;
                n_cons += pick + 1;
                if (S < Sbest * (1.0 - MP_BEST_EPS)) {
                    Sbest = S;
                    improved = 1;
                }
            } else {
                n_cons += B;
            }
            if (lane == 0) {
                sh_pick = pick;
                sh_improved = improved;
                if (st.trace) st.trace[(int64_t)r * n_trace + gb] = pick;
            }
        }
        __syncthreads();
        const int pick = sh_pick;                                 // (uniform)
        if (pick >= 0) {
            const int a = sh_a[pick], b = sh_b[pick];
            int* col = lev + (int64_t)sh_c[pick] * n;
            const int la = col[a], lb = col[b];
            double *Ta = T + (int64_t)a * n, *Tb = T + (int64_t)b * n;
            for (int j = tid; j < n; j += MP_THREADS) {
                if (j == a || j == b) continue;
                double ra, rb;
                mp_ratios(la, lb, col[j], ra, rb);
                const double ta = Ta[j] * ra, tb = Tb[j] * rb;
                Ta[j] = ta;
                T[(int64_t)j * n + a] = ta;
                Tb[j] = tb;
                T[(int64_t)j * n + b] = tb;
            }
            __syncthreads();
            if (tid == 0) col[a] = lb, col[b] = la;
            __syncthreads();
            if (sh_improved)
                for (int t = tid; t < n * d; t += MP_THREADS) best[t] = lev[t];
        }
    }
    if (tid == 0) {
        st.sums[4 * r] = S;
        st.sums[4 * r + 1] = Sbest;
        st.counts[2 * r] = n_acc;
        st.counts[2 * r + 1] = n_cons;
    }
}

// T [n][n] of a design; order [n]: row `first`, then again and again the row with the smallest sum of its pair terms with the rows
// chosen so far (the lowest index wins a tie).  Lane t holds the scores of the rows t, t + MP_THREADS, ...
__global__ __launch_bounds__(MP_THREADS) void k_mp_order(const double* __restrict__ T, int n, int first, int* __restrict__ order) {
    __shared__ double wv[MP_WAVES];
    __shared__ int wi[MP_WAVES];
    __shared__ int sh_pick;
    const int tid = threadIdx.x, lane = tid & (MP_WAVE - 1), wave = tid / MP_WAVE;
    double sc[MP_ROWS_PER_LANE];
    bool used[MP_ROWS_PER_LANE];
#pragma unroll
    for (int k = 0; k < MP_ROWS_PER_LANE; ++k) sc[k] = 0.0, used[k] = false;
    int pick = first;
    for (int step = 0; step < n; ++step) {
        if (tid == 0) order[step] = pick;
        if (step == n - 1) break;
        const double* Tp = T + (int64_t)pick * n;
        double bv = INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < MP_ROWS_PER_LANE; ++k) {
            const int j = mp_row(tid, MP_THREADS, k);
            if (j >= n) continue;
            if (j == pick) used[k] = true;
            if (used[k]) continue;
            sc[k] += Tp[j];
            if (sc[k] < bv || (sc[k] == bv && j < bi)) bv = sc[k], bi = j;
        }
        for (int o = 32; o >= 1; o >>= 1) {
            const double ov = __shfl_xor(bv, o, MP_WAVE);
            const int oi = __shfl_xor(bi, o, MP_WAVE);
            if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
        }
        if (lane == 0) wv[wave] = bv, wi[wave] = bi;
        __syncthreads();
        if (tid == 0) {
            double v = wv[0];
            int at = wi[0];
            for (int q = 1; q < MP_WAVES; ++q)
                if (wv[q] < v || (wv[q] == v && wi[q] < at)) v = wv[q], at = wi[q];
            sh_pick = at;
        }
        __syncthreads();
        pick = sh_pick;
    }
}

#define MP_FAIL(fn, msg) GPB_FAIL(GPB_E_ARG, fn ": " msg)

int mp_check_shape(gpb_ctx* ctx, const char* fn, int64_t n, int64_t d) {
    if (n < MP_MIN_N || n > MP_MAX_N) GPB_FAIL(GPB_E_ARG, std::string(fn) + ": n outside 4 .. 4096");
    if (d < MP_MIN_D || d > MP_MAX_D) GPB_FAIL(GPB_E_ARG, std::string(fn) + ": d outside 2 .. 64");
    return 0;
}

// a real design X [n][d] (host) as columns x [d][n] on the device, its pair matrix (with_T) and the sum of its pair terms
int mp_real_design(gpb_ctx* ctx, const char* fn, const double* X, int64_t n, int64_t d, bool with_T, MaxproWs& ws, double* sum) {
    if (const int rc = mp_check_shape(ctx, fn, n, d)) return rc;
    for (int64_t t = 0; t < n * d; ++t)
        if (!isfinite(X[t])) GPB_FAIL(GPB_E_ARG, std::string(fn) + ": X must be finite");
    GPB_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (const int rc = ctx_carve(ctx, ctx->maxpro_ws, [&](Carver<int64_t>& c) { ws.lay(c, n, d, with_T ? 1 : 0, 0, 1); })) return rc;
    std::vector<double> cols((size_t)(n * d));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t l = 0; l < d; ++l) cols[(size_t)(l * n + i)] = X[i * d + l];
    GPB_HIP(hipMemcpyAsync(ws.x, cols.data(), sizeof(double) * cols.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_mp_build<double>, dim3((unsigned)n, 1), dim3(MP_BUILD_THREADS), 0, s, (const double*)ws.x, (int)n, (int)d, MP_E15,
                       with_T ? ws.T : (double*)nullptr, ws.score);
    GPB_HIP(hipStreamSynchronize(s));                             // (cols goes out of use; ws.score holds the row sums for now)
    GPB_HIP(hipGetLastError());
    std::vector<double> rows((size_t)n);
    GPB_HIP(hipMemcpy(rows.data(), ws.score, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    double a = 0.0;
    for (int64_t i = 0; i < n; ++i) a += rows[(size_t)i];
    *sum = a;
    return 0;
}

}  // namespace

}  // namespace gpb

using namespace gpb;

extern "C" int gpb_maxpro_lhd(gpb_ctx* ctx, int64_t n, int64_t d, int R, int restart0, const int32_t* init_levels, uint64_t seed,
                              int64_t n_stages, int64_t blocks_per_stage, int block, double temp0, double cool, int32_t* levels_out,
                              double* f_start, double* f_best, int64_t* accepted, int64_t* consumed, int32_t* trace) {
    if (!ctx) return GPB_E_ARG;
    if (const int rc = mp_check_shape(ctx, "gpb_maxpro_lhd", n, d)) return rc;
    if (!init_levels || !levels_out) MP_FAIL("gpb_maxpro_lhd", "init_levels and levels_out must be given");
    if (R < 1 || R > MP_MAX_R) MP_FAIL("gpb_maxpro_lhd", "R outside 1 .. 16");
    if (restart0 < 0) MP_FAIL("gpb_maxpro_lhd", "restart0 below 0");
    if (block < 1 || block > MP_MAX_BLOCK) MP_FAIL("gpb_maxpro_lhd", "block outside 1 .. 64");
    if (n_stages < 1 || blocks_per_stage < 1 || (__int128)n_stages * blocks_per_stage > 0x7fffffffLL)
        MP_FAIL("gpb_maxpro_lhd", "need n_stages >= 1, blocks_per_stage >= 1 and at most 2^31 - 1 blocks in all");
    if (!(temp0 > 0.0) || !isfinite(temp0) || !(cool > 0.0) || !isfinite(cool))
        MP_FAIL("gpb_maxpro_lhd", "temp0 and cool must be positive and finite");
    const int64_t nd = n * d, n_blocks = n_stages * blocks_per_stage;
    std::vector<int32_t> cols((size_t)(R * nd));
    {
        std::vector<char> seen((size_t)n);
        for (int r = 0; r < R; ++r)
            for (int64_t l = 0; l < d; ++l) {
                std::fill(seen.begin(), seen.end(), 0);
                for (int64_t i = 0; i < n; ++i) {
                    const int32_t v = init_levels[(r * n + i) * d + l];
                    if (v < 0 || v >= n || seen[(size_t)v]) MP_FAIL("gpb_maxpro_lhd", "a column of init_levels is not a permutation of 0 .. n - 1");
                    seen[(size_t)v] = 1;
                    cols[(size_t)((r * d + l) * n + i)] = v;
                }
            }
    }
    GPB_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    MaxproWs ws;
    if (const int rc = ctx_carve(ctx, ctx->maxpro_ws, [&](Carver<int64_t>& c) { ws.lay(c, n, d, R, trace ? n_blocks : 0, 0); })) return rc;
    const MpRun st{ws.T, ws.sums, ws.counts, ws.lev, ws.best, trace ? ws.trace : nullptr};
    const double scale = mp_scale((int)n);
    auto rebuild = [&](const int* lev, double* T, int what) {
        hipLaunchKernelGGL(k_mp_build<int>, dim3((unsigned)n, (unsigned)R), dim3(MP_BUILD_THREADS), 0, s, lev, (int)n, (int)d, scale, T, ws.rowsum);
        hipLaunchKernelGGL(k_mp_total, dim3((unsigned)R), dim3(MP_BUILD_THREADS), 0, s, (const double*)ws.rowsum, (int)n, what, ws.sums, ws.counts);
    };

    // ---- the starts: their pair matrices and sums; a start whose sum is not finite is refused
    GPB_HIP(hipMemcpyAsync(ws.lev, cols.data(), sizeof(int32_t) * cols.size(), hipMemcpyHostToDevice, s));
    GPB_HIP(hipMemcpyAsync(ws.best, ws.lev, sizeof(int32_t) * cols.size(), hipMemcpyDeviceToDevice, s));
    rebuild(ws.lev, ws.T, 0);
    std::vector<double> sums((size_t)(4 * R));
    GPB_HIP(hipMemcpyAsync(sums.data(), ws.sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, s));
    GPB_HIP(hipStreamSynchronize(s));
    GPB_HIP(hipGetLastError());
    for (int r = 0; r < R; ++r)
        if (!isfinite(sums[(size_t)(4 * r)]) || !(sums[(size_t)(4 * r)] > 0.0))
            GPB_FAIL(GPB_E_ARG, "gpb_maxpro_lhd: the objective of a start is not finite (two rows adjacent in every column of a wide design)");

    // ---- the annealing: per stage the rebuild (the first stage's stands) and its blocks, in launches of MP_CHUNK at most
    for (int64_t k = 0; k < n_stages; ++k) {
        const double temp = temp0 * pow(cool, (double)k);
        if (!(temp > 0.0) || !isfinite(temp)) MP_FAIL("gpb_maxpro_lhd", "a stage's temperature temp0 cool^k is not positive and finite");
        if (k > 0) rebuild(ws.lev, ws.T, 1);
        for (int64_t b0 = 0; b0 < blocks_per_stage; b0 += MP_CHUNK) {
            const int nb = (int)imin64(MP_CHUNK, blocks_per_stage - b0);
            hipLaunchKernelGGL(k_mp_anneal, dim3((unsigned)R), dim3(MP_THREADS), 0, s, st, (int)n, (int)d, block, seed, (uint32_t)restart0,
                               (uint32_t)(k * blocks_per_stage + b0), nb, n_blocks, temp);
        }
    }
    rebuild(ws.best, (double*)nullptr, 2);                        // f of the best levels, recomputed from them

    // ---- results
    std::vector<int64_t> counts((size_t)(2 * R));
    GPB_HIP(hipMemcpyAsync(sums.data(), ws.sums, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, s));
    GPB_HIP(hipMemcpyAsync(counts.data(), ws.counts, sizeof(int64_t) * counts.size(), hipMemcpyDeviceToHost, s));
    GPB_HIP(hipMemcpyAsync(cols.data(), ws.best, sizeof(int32_t) * cols.size(), hipMemcpyDeviceToHost, s));
    if (trace) GPB_HIP(hipMemcpyAsync(trace, ws.trace, sizeof(int32_t) * (size_t)(R * n_blocks), hipMemcpyDeviceToHost, s));
    GPB_HIP(hipStreamSynchronize(s));
    GPB_HIP(hipGetLastError());
    for (int r = 0; r < R; ++r) {
        if (f_start) f_start[r] = log(sums[(size_t)(4 * r + 2)]);
        if (f_best) f_best[r] = log(sums[(size_t)(4 * r + 3)]);
        if (accepted) accepted[r] = counts[(size_t)(2 * r)];
        if (consumed) consumed[r] = counts[(size_t)(2 * r + 1)];
        for (int64_t l = 0; l < d; ++l)
            for (int64_t i = 0; i < n; ++i) levels_out[(r * n + i) * d + l] = cols[(size_t)((r * d + l) * n + i)];
    }
    return 0;
}

extern "C" int gpb_maxpro_criterion(gpb_ctx* ctx, const double* X, int64_t n, int64_t d, double* lnpsi_out, double* sum_out) {
    if (!ctx) return GPB_E_ARG;
    if (!X || !lnpsi_out) MP_FAIL("gpb_maxpro_criterion", "X and lnpsi_out must be given");
    MaxproWs ws;
    double sum = 0.0;
    if (const int rc = mp_real_design(ctx, "gpb_maxpro_criterion", X, n, d, false, ws, &sum)) return rc;
    *lnpsi_out = mp_lnpsi(log(sum), (int)n, (int)d);
    if (sum_out) *sum_out = sum;
    return 0;
}

extern "C" int gpb_maxpro_run_order(gpb_ctx* ctx, const double* X, int64_t n, int64_t d, int64_t first, int32_t* order_out) {
    if (!ctx) return GPB_E_ARG;
    if (!X || !order_out) MP_FAIL("gpb_maxpro_run_order", "X and order_out must be given");
    if (const int rc = mp_check_shape(ctx, "gpb_maxpro_run_order", n, d)) return rc;
    if (first < -1 || first >= n) MP_FAIL("gpb_maxpro_run_order", "first outside -1 .. n - 1");
    MaxproWs ws;
    double sum = 0.0;
    if (const int rc = mp_real_design(ctx, "gpb_maxpro_run_order", X, n, d, true, ws, &sum)) return rc;
    if (first < 0) {                                              // the row nearest the cube's centre, the lowest index at a tie
#pragma clang fp contract(off)
        double bestv = INFINITY;
        for (int64_t i = 0; i < n; ++i) {
            double a = 0.0;
            for (int64_t l = 0; l < d; ++l) {
                const double v = X[i * d + l] - 0.5;
                a += v * v;
            }
            if (a < bestv) bestv = a, first = i;
        }
    }
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_mp_order, dim3(1), dim3(MP_THREADS), 0, s, (const double*)ws.T, (int)n, (int)first, ws.order);
    GPB_HIP(hipMemcpyAsync(order_out, ws.order, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    GPB_HIP(hipStreamSynchronize(s));
    GPB_HIP(hipGetLastError());
    return 0;
}
