/*
 * gpbayes_debug.h — test and measurement hooks of libgpbayes_debug.so ONLY.
 *
 * NOT part of the drop-in boundary and NOT in the product library: libgpbayes.so exports include/gpbayes.h and nothing
 * else (tests/test_cabi_load.py pins both export lists).  The debug build is the same sources compiled with
 * -DGPB_DEBUG_VARIANTS: every entry point of gpbayes.h, plus the hooks below for tests/ (parity of internal pieces against
 * the oracle, the R > 1 step loop on one GPU) and tools/ (A/B measurements), plus the measured-and-rejected kernel variants
 * behind their gpb_ctx_option keys.
 */
#ifndef GPBAYES_DEBUG_H
#define GPBAYES_DEBUG_H

#include "gpbayes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- sampler internals (tests/test_gpu_sampler_step.py) ----------------------------- */
/* test hook: out_dev[i] = pi_step(i), the keyed permutation that shuffles the red/blue split */
GPB_API int gpb_test_split_perm(gpb_ctx* ctx, int64_t n, uint64_t seed, uint64_t step, int64_t* out_dev);
/* test hook: Philox4x32-10 on the device for n (key, counter) pairs: in_host[n][6] = k0, k1, c0, c1, c2, c3;
 * out_host[n][4].  Checked against Random123's known-answer vectors and the oracle's restatement. */
GPB_API int gpb_test_philox(gpb_ctx* ctx, int64_t n, const uint32_t* in_host, uint32_t* out_host);
/* test hook: every random number gpb_stretch_propose / gpb_stretch_accept use for (seed, step, half): member k of
 * the half gets u_z[k] (stretch factor draw), j[k] (index into the complementary half), u_acc[k] (accept draw);
 * perm[nwalkers] is the split permutation of the step (identity when randomize_split = 0).  Device outputs. */
GPB_API int gpb_test_stretch_draws(gpb_ctx* ctx, int64_t nwalkers, int half, uint64_t seed, uint64_t step,
                           int randomize_split, double* u_z_dev /*[nw/2]*/, int64_t* j_dev /*[nw/2]*/,
                           double* u_acc_dev /*[nw/2]*/, int64_t* perm_dev /*[nw]*/);

/* test hook: every random number of gpb_chain_ptlmc_run's step `step` for T rungs of d parameters: normals [T, d] (the
 * proposal's rvalo), logu_accept [T] (the accept test's log u), picks [5T] (the exchange's rt in 1 .. T - 1, in the order
 * the serial lane takes them) and logu_swap [5T].  Device outputs. */
GPB_API int gpb_test_ptlmc_draws(gpb_ctx* ctx, int64_t T, int64_t d, uint64_t seed, uint64_t step, double* normals_dev,
                         double* logu_accept_dev /*[T]*/, int64_t* picks_dev /*[5T]*/, double* logu_swap_dev /*[5T]*/);
/* test hook: every random number of gpb_chain_smc_reweight's stage `stage` and gpb_chain_smc_move's step `step` for N
 * particles of d parameters: normals [N, d] (the proposal's z), logu_accept [N] (the accept test's log u) and
 * u_resample [1] (the uniform of the systematic resampling).  Device outputs. */
GPB_API int gpb_test_smc_draws(gpb_ctx* ctx, int64_t N, int64_t d, uint64_t seed, uint64_t stage, uint64_t step,
                       double* normals_dev /*[N,d]*/, double* logu_accept_dev /*[N]*/, double* u_resample_dev /*[1]*/);

/* ---- likelihood tables (tests/test_gpu_closure.py) ---------------------------------- */
/* test hook: the data terms of the low-rank likelihood as they lie on the device.  K = 0: the installed experiment's
 * lr_v0 [16] and lr_cperp [1]; K >= 1: the tables of gpb_chain_like_sets, v0 [K][16] and cperp [K] (GPB_E_ARG unless K is the
 * tables' K).  GPB_E_STATE when the context does not hold them.  Synchronises. */
GPB_API int gpb_debug_like_tables(gpb_ctx* ctx, int64_t K, double* v0_host, double* cperp_host);

/* ---- micro-benchmarks / self-tests (device) --------------------------------------- */
/* C[M,N] = A*B through the f64 MFMA tile engine (K%16==0).  b_trans bits 0-1: 0 = A[M,K] B[K,N],
 * 1 = A[M,K] B[N,K]^T, 2 = A[K,M]^T B[K,N]; bit 2: 64x64 tiles instead of 128x128. */
GPB_API int gpb_test_gemm(gpb_ctx* ctx, int64_t M, int64_t N, int64_t K,
                  const double* A_host, const double* B_host, double* C_host, int b_trans);
/* gpb_ctx_option keys 26 / 32 take non-zero values in this build only (the product library returns GPB_E_ARG for them):
 * gpb_emcee_run behaves like rank `32` of `26` ranks on a single GPU (evaluates that rank's share of every batch, still issues
 * the collective of a one-rank communicator): one rank's share of a sharded step, tools/gpu_shard_sim.py. */
/* test hook: make R contexts of ONE process (each with its own stream, each driven by its own host thread) the ranks 0 .. R-1 of
 * a loopback communicator: gpb_dist_allgather / the in-stream all-gathers of gpb_chain_emcee_run are then emulated on the
 * ranks' streams (events + device copies; the host threads meet inside the call, so every rank must make the same calls
 * concurrently).  What a one-GPU box can run of the R > 1 step loop — everything but the RCCL wire.  Release the group
 * (any member) before destroying its contexts. */
GPB_API int gpb_debug_loopback_group(gpb_ctx* const* ctxs, int R);
GPB_API int gpb_debug_loopback_release(gpb_ctx* ctx);
/* debug hook: per-tile placement and timing of the predict kernel.  capacity > 0 arms (and clears) a trace of
 * that many records, 0 disarms; read copies up to max_records records of 8 uint32 {HW_ID register, XCC_ID,
 * GP, row block, walker tile, start, end (100 MHz ticks), blockIdx} to the host and re-arms. */
GPB_API int gpb_debug_tile_trace(gpb_ctx* ctx, int64_t capacity);
GPB_API int gpb_debug_tile_trace_read(gpb_ctx* ctx, uint32_t* records_host, int64_t max_records, int64_t* n_out);
/* debug hook: the device buffers this library's buffer cache has handed out and not yet got back (every context of the
 * process together), their number and their bytes — what a test compares before and after a context's life */
GPB_API int gpb_debug_pool_live(int64_t* buffers, int64_t* bytes);
/* issue-rate probe: returns measured TFLOP/s of back-to-back v_mfma_f64_16x16x4_f64
 * (mode 0), v_fma_f64 (mode 1) or both co-issued (mode 2); mode 3: shader cycles per MFMA (one wave
 * per SIMD); mode 4: shader clock in GHz held during the dense MFMA loop. */
GPB_API int gpb_probe_fp64(gpb_ctx* ctx, int mode, double* tflops_out);

#ifdef __cplusplus
}
#endif
#endif /* GPBAYES_DEBUG_H */
