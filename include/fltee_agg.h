/*
 * fltee_agg.h — C ABI of libfltee_agg.so, the MI355X-native replacement for
 * FL-TEE's SGX aggregation enclave (secure_aggregation/enclave).
 *
 * Drop-in boundary.  The four ECALLs below keep the exact symbol names and
 * argument lists that the Rust host binds in
 *     secure_aggregation/app/src/ecalls.rs:6-64
 * (EDL contract: secure_aggregation/enclave/Enclave.edl:23-84), including the
 * leading (eid, *retval) pair that sgx_edger8r's untrusted bridge adds.  A host
 * that linked the edger8r bridge (app/Enclave_u.c) links this library instead;
 * see INTEGRATION.md for the ecalls.rs / build.rs diff.
 *
 * Conventions:
 *   - return value  = "bridge" status: always FLTEE_SUCCESS for an in-process
 *                     call (the SGX bridge could fail; this one cannot), except
 *                     FLTEE_ERROR_INVALID_ENCLAVE_ID for an unknown eid.
 *   - *retval       = the enclave's status: 0 success, 0x1 unexpected
 *                     (unknown fl_id / missing session key / device failure),
 *                     0x2 invalid parameter (round / alg / id-set / size
 *                     mismatch, and every case where the reference enclave
 *                     would panic: unknown alg (lib.rs:396), out-of-range
 *                     index in non_oblivious (non_oblivious.rs:12), fold
 *                     longer than the payload (advanced.rs:70-72)).
 *   - ownership     : the caller owns every buffer; nothing is retained.
 *   - [out] buffers : zero-filled by the callee before anything else (the SGX
 *                     bridge did this, Enclave_t.c:626); execution_time_results
 *                     is always fully written.
 *   - threading     : calls may arrive from any thread (tokio workers,
 *                     server.rs:241-245); the library serialises them with one
 *                     process-wide mutex (the enclave had one TCS,
 *                     Enclave.config.xml:6) and binds the eid's device per call.
 *                     The device-resident entry points below share per-device
 *                     scratch: calls for one device must not overlap in time on
 *                     different streams (the mutex orders the host calls; the
 *                     kernels of two streams could still interleave).
 */
#ifndef FLTEE_AGG_H
#define FLTEE_AGG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* sgx_status_t subset (sgx_error.h values) */
typedef uint32_t fltee_status_t;
#define FLTEE_SUCCESS 0x0000u
#define FLTEE_ERROR_UNEXPECTED 0x0001u
#define FLTEE_ERROR_INVALID_PARAMETER 0x0002u
#define FLTEE_ERROR_OUT_OF_MEMORY 0x0003u
#define FLTEE_ERROR_INVALID_ENCLAVE_ID 0x2002u
#define FLTEE_ERROR_MAC_MISMATCH 0x3001u /* sgx_error.h SGX_ERROR_MAC_MISMATCH: an upload's
                                            GCM tag did not verify (fltee_set_upload_aead) */

/* sgx_enclave_id_t */
typedef uint64_t fltee_eid_t;

/* aggregation_alg codes, src/option.py:131-145 */
#define FLTEE_ALG_ADVANCED 1u
#define FLTEE_ALG_NIPS19 2u
#define FLTEE_ALG_BASELINE 3u
#define FLTEE_ALG_NON_OBLIVIOUS 4u
#define FLTEE_ALG_PATH_ORAM 5u
#define FLTEE_ALG_OPTIMIZED 6u
/* lib.rs:389 -> bubble_sort_based.rs (the reference bench's `-a bubble`): records ++ (i, 0.0)
 * for i < d sorted STABLY by idx, advanced's fold, a second sort, the first d values.  Each
 * index's run reaches the fold in upload order with its zero entry last, so the result is
 * the in-order client sum ((v1 + v2) + ... + vc) + 0.0 — the bits of non_oblivious and
 * baseline — out of an oblivious sort-based pipeline.  Here the O(L^2) bubble passes are
 * replaced by a data-independent bitonic network on 16-byte records keyed (idx << 32 |
 * upload position) (k_stable.hip): the same output at O(L log^2 L) fixed cost; the fold,
 * compaction and extract are advanced's.
 *   - fold length: n * k_req + d (bubble_sort_based.rs:42); only k_req == k is answered,
 *     anything else (FLTEE_OPT_K_REQ with another k_req) is FLTEE_ERROR_INVALID_PARAMETER;
 *   - opts.fold_halo as for advanced: runs of <= halo + 1 entries bit for bit, longer
 *     ones re-associated at the fold's walk boundaries;
 *   - records with idx >= d are ignored (they sort behind the d zero entries);
 *   - size limit: next_pow2(n * k + d) <= 2^29 records (the network holds 16 B per record,
 *     addressed with 64-bit byte offsets; positions are 32-bit), else INVALID_PARAMETER
 *     before any scratch is reserved;
 *   - FLTEE_OPT_CLIP / _DP / _ACCUMULATE / _NO_AVERAGE and n_avg as for advanced;
 *   - an eid over several GPUs (fltee_device_init_multi) shards the ECALL by position range,
 *     like advanced: the stable network over W ranges of C = M / W 16-byte records (range
 *     sorts, pairwise range exchanges, range merges: the fltee_stable_*_range pieces
 *     below), then advanced's halo fold, compaction and reduce.  The same bits as one GPU. */
#define FLTEE_ALG_BUBBLE 7u

/* ------------------------------------------------------------------------ */
/* Device lifetime — replaces init_enclave() / SgxEnclave::destroy()         */
/* (app/src/ecalls.rs:66-83, server.rs:224-235,257).                          */
/* ------------------------------------------------------------------------ */
fltee_status_t fltee_device_init(int hip_device, fltee_eid_t *eid);
fltee_status_t fltee_device_fini(fltee_eid_t eid);

/* One enclave id over n GPUs of this node (n a power of two): the four ECALLs of that
 * eid shard the aggregation internally and return the same bits as one
 * GPU.  Dense uploads (baseline / non_oblivious / path_oram with k = d): parameter-range
 * shards, each GPU copies and decrypts only its columns of the host ciphertext over its
 * own PCIe link, RCCL gathers the averaged slices on the root (hip_devices[0]).
 * advanced: position-range sharded bitonic network (RCCL all-to-alls), halo fold,
 * compaction and one RCCL reduce.  nips19: the same network (pairwise exchanges), the
 * ranges' selected entries gathered in order to the root.  alg 7 (once switched on,
 * fltee_set_bubble_ecall): the stable network over position ranges of 16-byte records
 * (pairwise range exchanges), then advanced's halo fold, compaction and reduce.  alg 6:
 * the batches split over the GPUs, the batch sums summed in order on the root.  Sparse
 * flat algorithms
 * run on the root.  Devices all distinct: RCCL over xGMI; the same device repeated n
 * times: n virtual ranks on that GPU (exchanges are device copies; for tests). */
fltee_status_t fltee_device_init_multi(const int *hip_devices, int n, fltee_eid_t *eid);
/* GPUs (ranks) behind an eid: 1 for fltee_device_init, n for _multi, 0 if unknown. */
int fltee_device_count(fltee_eid_t eid);

/* ------------------------------------------------------------------------ */
/* The four ECALLs (ecalls.rs:6-64 / Enclave.edl:26-73)                      */
/* ------------------------------------------------------------------------ */

/* lib.rs:113-180 — (re)create the config of fl_id, mock session keys. */
fltee_status_t ecall_fl_init(fltee_eid_t eid, fltee_status_t *retval, uint32_t fl_id,
                             const uint32_t *client_ids, size_t client_size,
                             size_t num_of_parameters, size_t num_of_sparse_parameters,
                             float sigma, float clipping, float alpha, float sampling_ratio,
                             uint32_t aggregation_alg, uint8_t verbose, uint8_t dp);

/* lib.rs:182-219 — sample (|ids| * ratio) clients for `round`.  The EDL types
 * sample_size as uint32_t (Enclave.edl:72) but Rust passes usize
 * (ecalls.rs:29): size_t is accepted. */
fltee_status_t ecall_start_round(fltee_eid_t eid, fltee_status_t *retval, uint32_t fl_id,
                                 uint32_t round, size_t sample_size,
                                 uint32_t *sampled_client_ids);

/* lib.rs:221-423 — load (H2D), decrypt (AES-128-CTR on the GPU), aggregate
 * with `aggregation_alg`, optional DP noise; writes the averaged f32[d] and
 * execution_time_results[3] = {load, decrypt, aggregate} seconds. */
fltee_status_t ecall_secure_aggregation(fltee_eid_t eid, fltee_status_t *retval, uint32_t fl_id,
                                        uint32_t round, const uint32_t *client_ids,
                                        size_t client_size,
                                        const uint8_t *encrypted_parameters_data,
                                        size_t encrypted_parameters_size,
                                        size_t num_of_parameters,
                                        size_t num_of_sparse_parameters,
                                        uint32_t aggregation_alg,
                                        float *updated_parameters_data,
                                        float *execution_time_results);

/* lib.rs:425-592 — alg 6: `advanced` over batches of optimal_num_of_clients
 * clients; the payload pointer is [user_check]: client_size * k * 8 bytes are
 * read. execution_time_results = {load, decrypt+aggregate, 0}. */
fltee_status_t ecall_client_size_optimized_secure_aggregation(
    fltee_eid_t eid, fltee_status_t *retval, uint32_t fl_id, uint32_t round,
    size_t optimal_num_of_clients, const uint32_t *client_ids, size_t client_size,
    const uint8_t *encrypted_parameters_data_ptr, size_t num_of_parameters,
    size_t num_of_sparse_parameters, uint32_t aggregation_alg, float *updated_parameters_data,
    float *execution_time_results);

/* ------------------------------------------------------------------------ */
/* Device-resident entry points: the aggregation below the ECALL, on records */
/* already decrypted into HBM.  Used by the bench (device-resident metric),  */
/* the multi-GPU driver and the parity tests.  All pointers are device       */
/* pointers; `stream` is a hipStream_t (NULL = legacy default stream).       */
/* Calls are asynchronous: errors found on the device are OR-ed into the     */
/* 32-bit status word (opts.d_status, or the library's own word read back by */
/* fltee_device_status()).                                                    */
/* ------------------------------------------------------------------------ */

/* device status bits */
#define FLTEE_DEV_ERR_DENSE_ORDER 0x1u   /* dense input with idx != position */
#define FLTEE_DEV_ERR_INDEX_RANGE 0x2u   /* idx >= d where the reference panics */
#define FLTEE_DEV_ERR_FOLD_OVERFLOW 0x4u /* retired in round 6 (advanced's fold finishes runs
                                           of any length); never set */
#define FLTEE_DEV_ERR_ORAM_STASH 0x8u    /* path_oram tree mode: the stash (20) overflowed */
#define FLTEE_DEV_ERR_AUTH 0x10u          /* an authenticated slice's tag did not verify */
#define FLTEE_DEV_ERR_LAUNCH 0x80000000u

/* option flags */
#define FLTEE_OPT_DENSE 0x1u      /* records are dense: client c, slot j has idx j (k == d, else
                                     INVALID_PARAMETER).  Algs 3, 4, 5 take the dense
                                     accumulate; on algs 1, 2, 6, 7 and the tree it changes
                                     nothing else */
#define FLTEE_OPT_DP 0x2u         /* add N(0, clipping*sigma)/n_avg noise (common.rs:56-72), one
                                     f32 add per parameter after everything else */
#define FLTEE_OPT_CLIP 0x4u       /* server-side per-client L2 clip (update.py:187-204) in front
                                     of every alg and route, whatever FLTEE_OPT_DENSE says:
                                     v * min(1, f32(C) / f32(sqrt(f64 sum of v^2))) in f32, on a
                                     scratch copy (d_records is never written) */
#define FLTEE_OPT_ACCUMULATE 0x8u /* out += sum, on every alg and route: the sum is never
                                     averaged (FLTEE_OPT_NO_AVERAGE and n_avg are ignored) and
                                     what d_out held is never scaled: alg-6 batches, shards */
#define FLTEE_OPT_NO_AVERAGE 0x10u /* skip the 1/n scaling (partial sums for RCCL) */
#define FLTEE_OPT_K_REQ 0x20u      /* advanced: fold over n*k_req+d even if k_req != k
                                      (advanced.rs:70 uses the REQUEST's k; 0 when
                                      fl_main.py sends dense uploads without --alpha) */
#define FLTEE_OPT_ORAM_TREE 0x40u  /* path_oram as a tree Path ORAM (oram.rs:64-118: Z = 4,
                                      stash 20, next_pow2(d) <= 2^22 blocks) running oram.rs's
                                      access sequence (d prepare writes, read + write per
                                      record, d readout reads) instead of the
                                      output-equivalent oblivious sweep */
#define FLTEE_OPT_ORAM_LAZY 0x80u  /* with ORAM_TREE: one read-modify-write access per record,
                                      blocks created on first use, readout by an oblivious
                                      sort of the tree's slots (n*k accesses instead of
                                      2*n*k + 2*d) */
#define FLTEE_OPT_PACKED 0x100u    /* d_records is the packed dense layout (below): n rows of
                                      2 * ceil(d / 2) f32, row c = client c's d values in position
                                      order, then one ignored f32 when d is odd.  k must equal d and
                                      d >= 2, else INVALID_PARAMETER.  Implies FLTEE_OPT_DENSE: algs
                                      3, 4, 5 take the packed accumulate (no scratch; with
                                      FLTEE_OPT_CLIP the coefficients only) and never set
                                      FLTEE_DEV_ERR_DENSE_ORDER (there is no index to check).  Every
                                      other alg, and the tree (FLTEE_OPT_ORAM_TREE / _LAZY), runs as
                                      it does for (n, d, d) on the records (j, v[j]) unpacked into the
                                      record scratch (n * d * 8 bytes more of it;
                                      FLTEE_OPT_CLIP clips that copy in place).  d_records is never
                                      written.  DP, ACCUMULATE, NO_AVERAGE and n_avg mean what they
                                      mean on the dense route */
#define FLTEE_OPT_TRIM 0x200u      /* coordinate-wise trimmed mean of a dense call (k_trim.hip):
                                      algs 3, 4, 5 with FLTEE_OPT_DENSE or FLTEE_OPT_PACKED, k = d,
                                      t = opts.trim.  Per output j, with x_c client c's value at j
                                      (FLTEE_OPT_CLIP: v * coef_c rounded, as the dense routes apply
                                      it) and ord(x) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000) on
                                      b = bits(x) — a total order on every bit pattern, -NaN < -inf
                                      < ... < -0.0 < +0.0 < ... < +inf < +NaN, so a NaN is always an
                                      extreme and the first value trimmed: the t clients smallest by
                                      (ord ascending, c ascending) are removed, then, of the rest,
                                      the t clients largest by (ord descending, c ascending) —
                                      among equal bit patterns the earliest uploads go first on
                                      both sides.  out[j] = sum * (1f32 / (f32)div), sum = the
                                      in-order f32 sum ((+0.0 + x_c1) + x_c2) + ... of the kept
                                      clients, div = n_avg ? n_avg : n - 2 t, which is the DP
                                      noise's divisor too; ACCUMULATE, NO_AVERAGE and DP mean what
                                      they mean on the dense route.  t = 0 is the untrimmed dense
                                      result bit for bit (the dense / packed accumulate runs); odd
                                      n with t = (n - 1) / 2 is the median, even n with
                                      t = n / 2 - 1 the mean of the two middle values.  Oblivious:
                                      every value is read at a fixed address (twice), the launch
                                      shapes depend on (n, d, t) and the pointers' alignment, all
                                      public.  No scratch (with FLTEE_OPT_CLIP the coefficients
                                      only); the records layout raises FLTEE_DEV_ERR_DENSE_ORDER as
                                      the dense route does.  Refused with INVALID_PARAMETER by host
                                      arithmetic, before anything is reserved or launched:
                                      trim > FLTEE_TRIM_MAX, 2 * trim >= n, any other alg, a call
                                      that is not dense, FLTEE_OPT_ORAM_TREE / _LAZY */
#define FLTEE_TRIM_MAX 64
#define FLTEE_OPT_TRIM_SELECT 0x800u /* with FLTEE_OPT_TRIM and t > 0: trim by selection
                                      (k_trim_select.hip) — the same definition, bit for bit, at any
                                      t with 2 t < n; FLTEE_TRIM_MAX is the cap of the list kernel
                                      above and does not apply.  The thresholds of an output (its
                                      t-th smallest and t-th largest ord) come from a bitwise
                                      descent on the 32-bit key, 32 rounds in which every value is
                                      compared, over the call's n x C tile held in LDS: the input is
                                      read once, at fixed addresses, and the launch shape depends on
                                      (n, d) alone.  t <= FLTEE_TRIM_MAX is answered too (the same
                                      bits as without the flag).  No scratch of its own: every
                                      scratch size is that of the same call without the flag (a
                                      FLTEE_OPT_BF16 call trims on its unpacked records, as there).
                                      t = 0 is the untrimmed route.  Refused with INVALID_PARAMETER
                                      by host arithmetic, before anything is reserved or launched:
                                      n > FLTEE_TRIM_SELECT_MAX_N, the flag without FLTEE_OPT_TRIM,
                                      and every refusal of FLTEE_OPT_TRIM other than
                                      trim > FLTEE_TRIM_MAX */
#define FLTEE_TRIM_SELECT_MAX_N 4096
#define FLTEE_OPT_BF16 0x400u      /* d_records is the bf16 dense layout (below): n rows of
                                      4 * ceil(d / 4) bf16, row c = client c's d values in position
                                      order, then ignored padding; a value is widened exactly, f32
                                      bits = (uint32)h << 16.  k must equal d and d >= 3, else
                                      INVALID_PARAMETER; INVALID_PARAMETER also together with
                                      FLTEE_OPT_PACKED and for a d_records that is not 2-byte
                                      aligned.  Implies FLTEE_OPT_DENSE: algs 3, 4, 5 take the bf16
                                      accumulate (no scratch; with FLTEE_OPT_CLIP the coefficients
                                      only) and never set FLTEE_DEV_ERR_DENSE_ORDER.  Every other
                                      alg, the tree (FLTEE_OPT_ORAM_TREE / _LAZY) and a call with
                                      FLTEE_OPT_TRIM (t > 0) runs as it does for (n, d, d) on the
                                      records (j, widen(h[j])) unpacked into the record scratch
                                      (n * d * 8 bytes more of it; FLTEE_OPT_CLIP clips that copy in
                                      place) — FLTEE_OPT_TRIM on algs 3, 4, 5 takes the records trim
                                      there: a bf16 call is trimmed, never refused and never
                                      silently untrimmed.  d_records is never written.  DP,
                                      ACCUMULATE, NO_AVERAGE and n_avg mean what they mean on the
                                      dense route */
#define FLTEE_OPT_FP8 0x1000u      /* d_records is the fp8 dense layout (below): n rows of
                                      8 * (ceil(d / 8) + 1) bytes, row c = client c's d e4m3fn codes
                                      in position order, ignored padding, then the client's f32
                                      scale s and 4 ignored bytes; a value is x = w(q) * s, w exact,
                                      the product rounded once (RN).  k must equal d and d >= 13,
                                      else INVALID_PARAMETER; INVALID_PARAMETER also together with
                                      FLTEE_OPT_PACKED or FLTEE_OPT_BF16 and for a d_records that is
                                      not 4-byte aligned (the scale is read as an f32).  Implies
                                      FLTEE_OPT_DENSE: algs 3, 4, 5 take the fp8 accumulate (no
                                      scratch; with FLTEE_OPT_CLIP the coefficients only, taken
                                      from the x values and applied to x: two roundings, scale
                                      first) and never set FLTEE_DEV_ERR_DENSE_ORDER.  Every other
                                      alg, the tree (FLTEE_OPT_ORAM_TREE / _LAZY) and a call with
                                      FLTEE_OPT_TRIM (with or without _TRIM_SELECT, t > 0) runs as it
                                      does for (n, d, d) on the records (j, x_j) unpacked into the
                                      record scratch, exactly as a FLTEE_OPT_BF16 call does.
                                      d_records is never written.  DP, ACCUMULATE, NO_AVERAGE and
                                      n_avg mean what they mean on the dense route */
#define FLTEE_OPT_KRUM 0x2000u     /* Multi-Krum (Blanchard et al., 2017) of a dense call
                                      (k_krum.hip): algs 3, 4, 5 with FLTEE_OPT_DENSE or
                                      FLTEE_OPT_PACKED, k = d; opts is a fltee_device_opts_krum
                                      (below): f = krum_f assumed Byzantine clients, m = krum_m kept.  A FLTEE_OPT_BF16 / _FP8
                                      call runs on its unpacked records, as a trimmed one does.  With
                                      x_c[j] the value the dense route would add for client c at j
                                      (FLTEE_OPT_CLIP: v * coef_c rounded):
                                        1. G[a][b] = sum_j (f64)x_a[j] * (f64)x_b[j]: every product
                                           exact, the sum in f64 in one order for every entry, a
                                           function of (n, d) alone (f64 MFMA over column chunks, the
                                           chunks' partials added in ascending order; no atomics):
                                           identical rows have identical entries, and a call repeats
                                           its bits;
                                        2. D[a][b] = (G[a][a] + G[b][b]) - 2 G[a][b] in f64, in that
                                           association; NaN and +-inf count as +inf, anything not
                                           above 0 as +0.0 (two identical rows: exactly 0);
                                        3. s_a = the f64 sum of the q = n - f - 2 smallest D[a][b],
                                           b != a, added in ascending order from +0.0;
                                        4. kept: the m clients smallest by (s ascending, client
                                           ascending); clients with s = +inf come last, in upload
                                           order;
                                        5. out[j] = sum * (1f32 / (f32)div), sum = the in-order f32 sum
                                           ((+0.0 + x_c1) + x_c2) + ... of the kept clients in upload
                                           order — a dropped client adds a selected +0.0, never a
                                           product with 0: a dropped NaN reaches no sum — and
                                           div = n_avg ? n_avg : m, which is the DP noise's divisor
                                           too; ACCUMULATE, NO_AVERAGE and DP mean what they mean on
                                           the dense route.  m = n - f with f = 0 keeps every client:
                                           the dense route's result bit for bit.
                                      Oblivious: every value is read at a fixed address (twice), the
                                      sort and the ranking are networks of compares feeding selects,
                                      the launch shapes depend on (n, d) and the pointers' alignment;
                                      q and m are compare constants.  The keep set never leaves the
                                      device.  Scratch: the Gram partials, G, the scores and the keep
                                      words, sized from (n, d) (with FLTEE_OPT_CLIP the coefficients
                                      too); the records layout raises FLTEE_DEV_ERR_DENSE_ORDER as
                                      the dense route does.  Refused with INVALID_PARAMETER by host
                                      arithmetic, before anything is reserved or launched:
                                      n < 2 f + 3, m = 0, m > n - f, n > FLTEE_KRUM_MAX_N, any other
                                      alg, a call that is not dense, FLTEE_OPT_ORAM_TREE / _LAZY, and
                                      the flag together with FLTEE_OPT_TRIM (the two robust aggregates
                                      are alternatives) */
#define FLTEE_KRUM_MAX_N 1024
#define FLTEE_OPT_GMED 0x4000u     /* the geometric median of a dense call (k_gmed.hip): the "RFA" of
                                      Pillutla, Kakade and Harchaoui (2022), R iterations of the smoothed
                                      Weiszfeld iteration.  Algs 3, 4, 5 with FLTEE_OPT_DENSE or
                                      FLTEE_OPT_PACKED, k = d; opts is a fltee_device_opts_gmed (below):
                                      R = gmed_iters, 1 <= R <= FLTEE_GMED_MAX_ITERS, and the smoothing
                                      floor nu = gmed_nu, a finite f64 > 0.  A FLTEE_OPT_BF16 / _FP8 call
                                      runs on its unpacked records, as a Krum call does.  x_c[j] is the
                                      value the dense route would add for client c at j (FLTEE_OPT_CLIP:
                                      v * coef_c rounded).  All f64 arithmetic is round-to-nearest add,
                                      multiply, divide and square root, never contracted.  sum64(v), the
                                      one reduction order, over indices 0 .. n - 1: p_l = the sum of v_i
                                      over i = l (mod 64), ascending, from +0.0; the result is
                                      p_0 ... p_63 added in ascending l, from +0.0.
                                        1. G = FLTEE_OPT_KRUM's step 1: the same kernels, geometry and
                                           summation order;
                                        2. valid_c = G[c][c] is finite: a row of finite f32 values is
                                           always valid, a row that holds an inf or a NaN is not;
                                        3. w_c = valid_c ? 1.0 : 0.0;
                                        4. R times: s = sum64(w);
                                           u_a = sum64 over b of (valid_b ? G[a][b] * w_b : +0.0), a
                                           select, never a product with 0;
                                           q = sum64 over a of (valid_a ? w_a * u_a : +0.0);
                                           inv = s > 0 ? 1 / s : 0;
                                           D_a = (G[a][a] - 2 * (u_a * inv)) + (q * inv) * inv, not
                                           finite -> +inf, not above 0 -> +0.0;
                                           rho_a = sqrt(D_a); w_a = valid_a ? 1 / max(nu, rho_a) : 0;
                                        5. s = sum64(w); alpha_c = (f32)(s > 0 ? w_c / s : 0): one f64
                                           divide, then one rounding to f32;
                                        6. out[j] = (((+0.0 + y_0) + y_1) + ...) in f32 in upload order,
                                           y_c = valid_c ? x_c[j] * alpha_c rounded : +0.0.  The weights
                                           sum to one: no averaging factor.  FLTEE_OPT_ACCUMULATE:
                                           out += that sum.  n_avg only sets the DP noise's divisor
                                           (n_avg ? n_avg : n).  Every client invalid: a vector of +0.0.
                                      The limit of the Gram form: a distance is resolved only down to
                                      about sqrt(n * 2^-52) * max |x_c|; below that D clamps to 0 and the
                                      weight is 1 / nu.  nu is therefore the host's statement of the
                                      smallest distance it cares about, and is taken as given.
                                      Oblivious: every value is read at a fixed address (twice); valid
                                      and the clamps are selects; the launch shapes depend on (n, d, R)
                                      and the pointers' alignment.  The weights never leave the device.
                                      Scratch: Krum's Gram partials and G, then w, u, rho, alpha and
                                      valid, sized from (n, d) alone (R and nu move no byte); the records
                                      layout raises FLTEE_DEV_ERR_DENSE_ORDER as the dense route does
                                      (reported, not followed).  Refused with INVALID_PARAMETER by host
                                      arithmetic, before anything is reserved or launched: any other
                                      alg, a call that is not dense, FLTEE_OPT_ORAM_TREE / _LAZY, n = 0,
                                      n > FLTEE_KRUM_MAX_N, R = 0, R > FLTEE_GMED_MAX_ITERS, a nu that is
                                      not a finite value above 0, and the flag together with
                                      FLTEE_OPT_TRIM, FLTEE_OPT_KRUM or FLTEE_OPT_NO_AVERAGE (a weighted
                                      mean has no partial-sum form) */
#define FLTEE_GMED_MAX_ITERS 64

typedef struct fltee_device_opts {
    uint32_t flags;     /* FLTEE_OPT_* */
    float sigma;        /* DP noise multiplier */
    float clipping;     /* DP / clip norm bound C */
    uint64_t seed;      /* RNG seed for nips19 / DP; 0 = draw from getrandom() */
    size_t k_req;       /* advanced: request num_of_sparse_parameters (with FLTEE_OPT_K_REQ) */
    size_t batch;       /* alg 6: optimal_num_of_clients */
    size_t n_avg;       /* divisor for averaging (0 = n): out = sum * (1f32 / (f32)n_avg), and
                           the DP noise's divisor */
    size_t fold_halo;   /* advanced fold halo H (0 = n): runs of <= H + 1 entries (each client's
                           indices distinct) bit for bit, longer ones re-associated at the
                           fold's walk boundaries */
    uint32_t *d_status; /* optional device status word (never cleared by the library) */
    size_t trim;        /* FLTEE_OPT_TRIM: clients removed on each side of every coordinate.  The
                           last field, read only when the flag is set: a caller built against the
                           struct without it, which never sets the flag, is unaffected */
} fltee_device_opts;

/* The options of a FLTEE_OPT_KRUM call: fltee_device_opts with Multi-Krum's two counts behind
 * `trim`.  A caller that sets FLTEE_OPT_KRUM in base.flags passes &x.base wherever a
 * const fltee_device_opts * is taken, and vouches by the flag that the two fields lie behind it:
 * the library copies a caller's struct up to `trim` and reads each field from there on under its
 * own flag (trim: FLTEE_OPT_TRIM; krum_f, krum_m: FLTEE_OPT_KRUM), so a caller whose struct ends
 * at `trim`, which never sets the flag, is unaffected, and fltee_device_opts itself keeps its
 * size. */
typedef struct fltee_device_opts_krum {
    fltee_device_opts base;
    size_t krum_f;      /* the assumed number of Byzantine clients f, and ... */
    size_t krum_m;      /* ... the number of clients kept m */
} fltee_device_opts_krum;

/* The options of a FLTEE_OPT_GMED call, by the same pattern: fltee_device_opts with the iteration
 * count and the smoothing floor behind `trim`, read only under FLTEE_OPT_GMED. */
typedef struct fltee_device_opts_gmed {
    fltee_device_opts base;
    size_t gmed_iters;  /* the Weiszfeld iterations R, 1 .. FLTEE_GMED_MAX_ITERS */
    double gmed_nu;     /* the smoothing floor nu: a finite value above 0 */
} fltee_device_opts_gmed;

/* Aggregate n clients x k records (8 B each: u32 LE idx, f32 LE val),
 * client-major, into d_out[d] (overwritten, or accumulated with
 * FLTEE_OPT_ACCUMULATE).  With FLTEE_OPT_PACKED d_records is n packed slices
 * (value-only, 8 * ceil(d / 2) bytes each) instead, with FLTEE_OPT_BF16 n bf16
 * slices (8 * ceil(d / 4) bytes each), with FLTEE_OPT_FP8 n fp8 slices
 * (8 * (ceil(d / 8) + 1) bytes each).  Returns
 * FLTEE_ERROR_INVALID_PARAMETER for host-detectable argument errors. */
fltee_status_t fltee_aggregate_device(uint32_t alg, const void *d_records, size_t n, size_t k,
                                      size_t d, float *d_out, const fltee_device_opts *opts,
                                      void *stream);

/* Bytes of scratch HBM the library will hold for this shape (grow-only): the sum over
 * every scratch buffer the call touches, from the same shape plan the call itself runs
 * by.  Not counted, because it depends on the data: nips19's selected list (8 bytes per
 * entry that survives the threshold, and the sort scratch of its ordered fold), sized
 * from a count read back from the device. */
size_t fltee_workspace_bytes(uint32_t alg, size_t n, size_t k, size_t d,
                             const fltee_device_opts *opts);
/* Pre-size that scratch: a later fltee_aggregate_device of the same shape and options
 * (and of any shape needing no more of each buffer) allocates and frees nothing — no
 * hipMalloc, and no hipFree with its device-wide synchronisation, inside a timed call.
 * The one exception is nips19's selected list above, which grows with the largest
 * count seen. */
fltee_status_t fltee_reserve(uint32_t alg, size_t n, size_t k, size_t d,
                             const fltee_device_opts *opts);

/* AES-128-CTR decrypt of n client slices (bytes_per_client each, zero counter
 * block per client, key = session key of client_ids[i]) into compact records
 * (n * (bytes_per_client/8) * 8 bytes).  lib.rs:312-343. */
fltee_status_t fltee_decrypt_device(const uint32_t *client_ids, size_t n, const void *d_cipher,
                                    size_t bytes_per_client, void *d_records, void *stream);

/* ---- client-side producers (fl_main.py:221-238) -------
 * For a GPU-resident client simulator: n clients' flattened updates d_values
 * [n][d] (f32) -> the encrypted payload of the Aggregate request, in HBM. */
/* utils.py:327-354 zero_except_top_k_weights + utils.py:193-209 serialize_sparse:
 * per client the k records (idx, val) of largest |val|, in the reference's order
 * (|val| descending, equal magnitudes by ascending idx; Python's stable sort). */
fltee_status_t fltee_client_topk_device(const float *d_values, size_t n, size_t d, size_t k,
                                        void *d_records, void *stream);
/* utils.py:171-190 serialize_dense: records (i, v[i]), i < d, per client. */
fltee_status_t fltee_client_serialize_dense_device(const float *d_values, size_t n, size_t d,
                                                   void *d_records, void *stream);
/* update.py:187-204 l2clipping on serialized records (n clients x k records, in
 * place): val *= min(1, clipping / ||client's values||_2). */
fltee_status_t fltee_client_clip_device(void *d_records, size_t n, size_t k, float clipping,
                                        void *stream);
/* utils.py:268-290 encrypt_parameters for n clients (ids < 65536: the client's
 * 2-byte key layout), bytes_per_client each; the inverse of fltee_decrypt_device. */
fltee_status_t fltee_encrypt_device(const uint32_t *client_ids, size_t n, const void *d_plain,
                                    size_t bytes_per_client, void *d_cipher, void *stream);

/* ---- packed dense uploads: value-only slices at half the bytes ----------------------------
 * A dense upload (serialize_dense, k = d) sends client c's slot j as the record (j, v[j]); the
 * index says nothing.  With U = ceil(d / 2), a PACKED slice is U units of 8 bytes: the d
 * little-endian f32 values in position order, followed by one f32 of padding when d is odd (the
 * client writes +0.0, the server ignores it).  A slice stays a whole number of 8-byte units, so
 * the CTR / GCM kernels, the chunked load and the survivors gather work on "U records per
 * client" unchanged. */
/* bytes of one packed slice of d parameters: 8 * ceil(d / 2) */
size_t fltee_packed_slice_bytes(size_t d);
/* The packed-call rule, the one place it is decided.  `on`: the switch below; d:
 * num_of_parameters; k_req: the request's num_of_sparse_parameters; ct_bytes: one client's
 * ciphertext bytes (without the 16-byte tag under AEAD), or 0 when the payload is not n equal
 * slices.  Returns 1 when ecall_secure_aggregation reads the payload as packed slices:
 *     on  &&  d >= 2  &&  k_req in {0, d} (the request declares a dense upload)
 *         &&  ct_bytes == 8 * ceil(d / 2).
 * Anything else is read as records exactly as before — a dense 8 * d-byte upload too, so old
 * and new clients share a server.  d = 1 is never packed (there 8 U == 8 d).  Host arithmetic. */
int fltee_upload_is_packed(int on, size_t d, size_t k_req, size_t ct_bytes);
/* Process-wide, like fltee_set_upload_aead; off by default: every call is then read as records,
 * launch for launch as before.  On: an ecall_secure_aggregation call that the rule above accepts
 * is loaded, decrypted, verified and (under FLTEE_AEAD_DROP) gathered as U units per client, and
 * aggregated with FLTEE_OPT_PACKED and k = d: algs 3, 4, 5 by the packed accumulate, algs 1, 2,
 * 7 and the tree on the unpacked records — [out] bit for bit what the same values sent as
 * (j, v[j]) records give.  The existing 0x2 refusals come first; advanced's "fold longer than
 * the payload" refusal counts a packed slice as its d records.  Under AEAD the last AAD word of
 * a packed call is BE32(aggregation_alg | 0x80000000): a slice sealed as records never verifies
 * as packed values, nor the other way round (0x3001).  On an eid over several GPUs a packed call
 * is loaded, verified and unpacked on the root (the dense group path declines it); the
 * position-range routes (algs 1, 2, 7) shard the unpacked records from there: the one-GPU bits.
 * ecall_client_size_optimized_secure_aggregation (alg 6) ignores the switch. */
void fltee_set_upload_packed(int on);
#define FLTEE_AAD_PACKED_BIT 0x80000000u
/* [n][2 U] f32 packed slices -> n * d records (j, v[j]), client-major: what every route other
 * than the packed accumulate runs on.  Asynchronous on `stream`.  d >= 1, d < 2^32. */
fltee_status_t fltee_unpack_dense_device(const void *d_packed, size_t n, size_t d, void *d_records,
                                         void *stream);
/* The client producer: n clients' values [n][d] f32 -> [n][2 U] packed slices (padding +0.0).
 * Sealing is fltee_encrypt_device / fltee_encrypt_auth_device with 8 U bytes per client. */
fltee_status_t fltee_client_pack_dense_device(const float *d_values, size_t n, size_t d,
                                              void *d_packed, void *stream);

/* ---- bf16 dense uploads: value-only slices at a quarter of the bytes ----------------------
 * A client that quantises its update to bf16 sends the 16 bits it has.  With Q = ceil(d / 4), a
 * BF16 slice is Q units of 8 bytes: the d little-endian bf16 values in position order, followed
 * by 4 Q - d bf16 of padding (the client writes +0.0, the server ignores it).  A slice stays a
 * whole number of 8-byte units, so the CTR / GCM kernels, the chunked load and the survivors
 * gather work on "Q records per client" unchanged.
 * Widening (server): f32 bits = (uint32)h << 16, exact for every bit pattern — NaN, +-inf and
 * denormals included: [out] is the in-order f32 sum of the values the clients sent, bit for bit
 * what the same values give as records.  Quantisation is the client's choice and the client's
 * error; the server adds none.
 * Narrowing (the producer below), with u = bits(x), in integer ops:
 *     (u & 0x7FFFFFFF) > 0x7F800000 (NaN):  h = (u >> 16) | 0x0040   (the sign kept, quieted)
 *     otherwise, round to nearest even:      h = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
 * (values just under FLT_MAX round to inf). */
/* bytes of one bf16 slice of d parameters: 8 * ceil(d / 4) */
size_t fltee_bf16_slice_bytes(size_t d);
/* The bf16-call rule, the one place it is decided; the arguments are fltee_upload_is_packed's.
 * Returns 1 when ecall_secure_aggregation reads the payload as bf16 slices:
 *     on  &&  d >= 3  &&  k_req in {0, d} (the request declares a dense upload)
 *         &&  ct_bytes == 8 * ceil(d / 4).
 * For d >= 3 that size differs from a packed slice (8 * ceil(d / 2)) and from records (8 * d):
 * both switches can be on and one server answers all three formats.  d < 3 is never bf16.  Host
 * arithmetic. */
int fltee_upload_is_bf16(int on, size_t d, size_t k_req, size_t ct_bytes);
/* Process-wide, like fltee_set_upload_packed; off by default: every call is then launch for
 * launch what it was.  On: an ecall_secure_aggregation call that the rule above accepts is
 * loaded, decrypted, verified and (under FLTEE_AEAD_DROP) gathered as Q units per client, and
 * aggregated with FLTEE_OPT_BF16 and k = d: algs 3, 4, 5 by the bf16 accumulate, algs 1, 2, 7
 * and the tree on the unpacked records — [out] bit for bit what the widened values sent as
 * (j, v[j]) records give.  The existing 0x2 refusals come first; advanced's "fold longer than
 * the payload" refusal counts a slice as its d records.  fltee_set_dense_trim applies with n'
 * and t as for a packed call (the trim runs on the unpacked records).  Under AEAD the last AAD
 * word of a bf16 call is BE32(aggregation_alg | 0x40000000): a slice sealed for one of the three
 * formats verifies under no other (0x3001).  On an eid over several GPUs the dense group path
 * declines a bf16 call and the root runs it, every alg: the one-GPU bits.
 * ecall_client_size_optimized_secure_aggregation (alg 6) ignores the switch. */
void fltee_set_upload_bf16(int on);
#define FLTEE_AAD_BF16_BIT 0x40000000u
/* [n][4 Q] bf16 slices -> n * d records (j, widen(h[j])), client-major: what every route other
 * than the bf16 accumulate runs on.  Asynchronous on `stream`.  d >= 1, d < 2^32; d_rows 2-byte
 * aligned. */
fltee_status_t fltee_unpack_bf16_device(const void *d_rows, size_t n, size_t d, void *d_records,
                                        void *stream);
/* The client producer: n clients' values [n][d] f32 -> [n][4 Q] bf16 slices, narrowed as above
 * (padding +0.0).  Sealing is fltee_encrypt_device / fltee_encrypt_auth_device with 8 Q bytes
 * per client. */
fltee_status_t fltee_client_pack_bf16_device(const float *d_values, size_t n, size_t d, void *d_rows,
                                             void *stream);

/* ---- fp8 dense uploads: value-only slices at an eighth of the bytes, with a client scale ------
 * A client that compresses its update to 8 bits sends the codes and one scale.  With
 * P = ceil(d / 8), an FP8 slice is P + 1 units of 8 bytes:
 *   values   bytes [0, d): the d codes in position order; bytes [d, 8 P): padding (the client
 *            writes 0x00, the server ignores it);
 *   trailer  the last unit: the client's scale s as a little-endian f32, then 4 bytes the client
 *            writes as zero and the server ignores.
 * The trailer sits at the end so that the values start at the row base; a slice stays a whole
 * number of 8-byte units, so the CTR / GCM kernels, the chunked load and the survivors gather
 * work on "P + 1 records per client" unchanged.
 * Code: OCP e4m3fn — 1 sign bit, 4 exponent bits (bias 7), 3 mantissa bits.  No infinities;
 * S.1111.111 (0x7F, 0xFF) is NaN; the largest finite value is 448 (0x7E), the smallest
 * subnormal 2^-9.
 * Widening (server): w(q) is the exact f32 of the code; a NaN code widens to the bits
 * sign << 31 | 0x7FC00000.  Then x = w(q) * s in f32, round to nearest even: the only rounding
 * the server adds.  Everything else applies to x exactly as to a record's value: FLTEE_OPT_CLIP
 * takes its f64 norm over the x values and rounds x * cc before the add; the sum is the in-order
 * f32 sum.  [out] is bit for bit what the same x values give as records.
 * The scale is taken as sent: NaN, +-inf, 0 and negative values are the client's own values, as a
 * sealed 1e30 is; a trimmed call (fltee_set_dense_trim) deals with them.
 * Narrowing (the producer below), per row: a = the largest finite |v_j|; s = a / 448 (f32, RN)
 * when that quotient is a normal, nonzero f32, else s = 1; y = v_j / s (f32, RN); NaN ->
 * sign | 0x7F; |y| > 448, +-inf included -> sign | 0x7E; otherwise the nearest representable
 * e4m3 magnitude, ties to the even code; the sign is kept (-0.0 -> 0x80).  A maximum does not
 * depend on the order it is taken in: the producer is deterministic. */
/* bytes of one fp8 slice of d parameters: 8 * (ceil(d / 8) + 1) */
size_t fltee_fp8_slice_bytes(size_t d);
/* The fp8-call rule, the one place it is decided; the arguments are fltee_upload_is_packed's.
 * Returns 1 when ecall_secure_aggregation reads the payload as fp8 slices:
 *     on  &&  d >= 13  &&  k_req in {0, d} (the request declares a dense upload)
 *         &&  ct_bytes == 8 * (ceil(d / 8) + 1).
 * 13 is the smallest d from which that size differs from a bf16 slice at every d: for d = 9..12
 * both are 24 bytes, and from 13 on ceil(d / 4) > ceil(d / 8) + 1; packed slices and records are
 * larger at every d >= 13.  So with all three switches on one server answers four formats by
 * their size.  Host arithmetic. */
int fltee_upload_is_fp8(int on, size_t d, size_t k_req, size_t ct_bytes);
/* Process-wide, like fltee_set_upload_bf16; off by default: every call is then launch for launch
 * what it was.  On: an ecall_secure_aggregation call that the rule above accepts is loaded,
 * decrypted, verified and (under FLTEE_AEAD_DROP) gathered as P + 1 units per client, and
 * aggregated with FLTEE_OPT_FP8 and k = d: algs 3, 4, 5 by the fp8 accumulate, algs 1, 2, 7 and
 * the tree on the unpacked records — [out] bit for bit what the x values sent as (j, x_j) records
 * give.  The existing 0x2 refusals come first; advanced's "fold longer than the payload" refusal
 * counts a slice as its d records.  fltee_set_dense_trim / _select apply as for a bf16 call (the
 * trim runs on the unpacked records).  Under AEAD the last AAD word of an fp8 call is
 * BE32(aggregation_alg | 0x20000000): a slice sealed for one of the four formats verifies under
 * no other (0x3001).  On an eid over several GPUs the dense group path declines an fp8 call and
 * the root runs it, every alg: the one-GPU bits.
 * ecall_client_size_optimized_secure_aggregation (alg 6) ignores the switch. */
void fltee_set_upload_fp8(int on);
#define FLTEE_AAD_FP8_BIT 0x20000000u
/* [n][8 (P + 1)] bytes of fp8 slices -> n * d records (j, w(q_j) * s), client-major: what every
 * route other than the fp8 accumulate runs on.  Asynchronous on `stream`.  d >= 1, d < 2^32;
 * d_rows 4-byte aligned. */
fltee_status_t fltee_unpack_fp8_device(const void *d_rows, size_t n, size_t d, void *d_records,
                                       void *stream);
/* The client producer: n clients' values [n][d] f32 -> [n][8 (P + 1)] bytes of fp8 slices,
 * narrowed as above, in two launches (each client's scale, then the quantise, which writes the
 * padding and the trailer too).  Sealing is fltee_encrypt_device / fltee_encrypt_auth_device with
 * 8 (P + 1) bytes per client.  d_rows 4-byte aligned.  The scales lie in the library's one
 * producer scratch between the two launches (fltee_client_clip_device's coefficients use the same
 * buffer): calls of the producers are serialised on one stream, not run concurrently on two. */
fltee_status_t fltee_client_pack_fp8_device(const float *d_values, size_t n, size_t d, void *d_rows,
                                            void *stream);

/* ---- robust aggregation: the coordinate-wise trimmed mean / median behind the ECALL ----------
 * A client with a valid session key can seal an authentic slice of 1e30 or NaN; a plain mean
 * hands it the round, and the host cannot repair that afterwards (it never sees the updates).
 * The trim count, the one place it is decided (host arithmetic):
 *     t = min(n * per_mille / 1000, (n - 1) / 2)   in integers, per_mille <= 500 (above: 500),
 * 0 for n = 0.  per_mille = 500 asks for the median (odd n; even n: the two middle values). */
size_t fltee_trim_count(size_t n, uint32_t per_mille);
/* Process-wide, like fltee_set_upload_packed; 0 (default) is off: every call is then launch for
 * launch what it was.  A value above 500 is stored as 500.  On: ecall_secure_aggregation computes
 * t = fltee_trim_count(n', per_mille), n' = the clients actually aggregated (the survivors under
 * FLTEE_AEAD_DROP: the gather, the trim and the divisor n' - 2 t agree), and a call on the dense
 * or the packed route (algs 3, 4, 5 on a dense upload in position; the staged and the pipelined
 * path alike) is aggregated with FLTEE_OPT_TRIM: [out] = the kept clients' in-order sum times
 * 1f32 / (f32)(n' - 2 t), the DP noise divided by n' - 2 t.  t = 0 (n' <= 2, a tiny per_mille)
 * runs untrimmed.  A host that switched trimming on never gets a silently untrimmed mean back:
 * what cannot be trimmed ends with 0x2, with the existing 0x2 refusals ([out] zero-filled, the
 * timers written, the round kept) — algs 1, 2 and 7, a sparse upload to algs 3, 4, 5, alg 5 under
 * fltee_set_path_oram_tree(1), t > FLTEE_TRIM_MAX, and every
 * ecall_client_size_optimized_secure_aggregation call; a dense-sized records upload out of
 * position (FLTEE_DEV_ERR_DENSE_ORDER, rerun sparse otherwise) ends with 0x2 after the one status
 * readback there already is.  Under AEAD the verification and the verdict come first, unchanged.
 * On an eid over several GPUs a trimmed records call takes the dense group path: every GPU
 * loads, decrypts and (AEAD) hashes its columns as for a plain call, and after the one verdict
 * trims its own columns — they are independent — into its slice of the output: the one-GPU
 * bits.  (A packed, bf16 or fp8 call is loaded and run on the root, trimmed or not.)  Nothing
 * new is revealed: the launch shapes depend on (n', d, t), the eid's size and the buffers'
 * alignment, all public. */
void fltee_set_dense_trim(uint32_t per_mille);
/* Process-wide; off by default: every call is then what it is above — t > FLTEE_TRIM_MAX (the
 * median from 131 clients on) ends with 0x2.  On, under fltee_set_dense_trim: a call whose
 * t = fltee_trim_count(n', per_mille) exceeds FLTEE_TRIM_MAX is aggregated with FLTEE_OPT_TRIM |
 * FLTEE_OPT_TRIM_SELECT when the request's n <= FLTEE_TRIM_SELECT_MAX_N, and ends with 0x2 above
 * it; a call with t <= FLTEE_TRIM_MAX stays on the list kernel, launch for launch.  Everything
 * else about a trimmed call holds: n' under FLTEE_AEAD_DROP, the divisor n' - 2 t, the staged and
 * the pipelined path, the refusals, a multi-GPU eid's column shards (each runs the selection
 * kernel on its columns).  Nothing
 * new is revealed: the launch shapes depend on (n', d) and on whether t > FLTEE_TRIM_MAX. */
void fltee_set_dense_trim_select(int on);

/* ---- robust aggregation: Multi-Krum behind the ECALL ------------------------------------------
 * The trimmed mean looks at one coordinate at a time; a colluding minority whose updates stay
 * inside every coordinate's range, or are so large that each coordinate's survivors come from
 * other clients, passes it.  Multi-Krum (FLTEE_OPT_KRUM above) scores whole clients by their
 * squared distances to their nearest neighbours and averages the m best-scored clients whole. */
/* Steps 1 - 4 of FLTEE_OPT_KRUM alone, device-resident: d_records is n dense uploads of d
 * parameters (records, or the layout opts' row flag names; FLTEE_OPT_DENSE is implied), opts is
 * the base of a fltee_device_opts_krum with FLTEE_OPT_KRUM set (INVALID_PARAMETER without the
 * flag) and gives krum_f, krum_m and, with FLTEE_OPT_CLIP, the bound (the other options are
 * ignored).  Leaves the n scores (f64) in d_scores and the n keep words (0 / 0xFFFFFFFF) in
 * d_keep, device memory both; asynchronous on `stream`.  The refusals and the scratch are those
 * of the aggregate call on alg 3.  For tests, and for hosts that drive one process per GPU. */
fltee_status_t fltee_krum_select_device(const void *d_records, size_t n, size_t d,
                                        const fltee_device_opts *opts, double *d_scores,
                                        uint32_t *d_keep, void *stream);
/* Step 1 of FLTEE_OPT_KRUM / FLTEE_OPT_GMED alone, over column ranges: the Gram matrix G = X X^T
 * of n dense uploads of d parameters (d_in: records, or with packed != 0 f32 rows) as an eid over
 * `ranks` GPUs computes it.  The one-GPU pass adds the partial matrices of the `chunks` column
 * chunks of its geometry (a function of (n, d): chunks of chunk_cols columns, a multiple of 16) in
 * ascending chunk order from +0.0.  Range i of `ranks` is the whole chunks
 * [chunks i / ranks, chunks (i + 1) / ranks) — columns [min(c_i chunk_cols, d),
 * min(c_(i+1) chunk_cols, d)), possibly none; each range runs the one-GPU Gram kernels on its
 * columns, and a carry chain adds its chunks, ascending, onto the running NP x NP f64 sum of the
 * ranges before it (the first from +0.0; a range without chunks is skipped): the additions of the
 * one-GPU pass in their order, so G is that pass's bit for bit for any `ranks`.  Here every range
 * runs on the current device, on its null stream, asynchronously; ranks = 1 is the one-GPU pass
 * itself, launch for launch.  d_G_out: NP x NP doubles, NP = 16 ceil(n / 16), device memory; the
 * entries past n are zero.  The selection-only entries above and below cover the rest of a call.
 * Refused by host arithmetic, before any launch, with FLTEE_ERROR_INVALID_PARAMETER: ranks = 0 or
 * above 64, n = 0 or above FLTEE_KRUM_MAX_N, d >= 2^31, a null pointer.  The records' idx ==
 * position check reaches fltee_device_status only with ranks = 1 (a range's kernels compare with
 * range-local positions, which an eid's ranks hold and whole rows do not).  For tests of the
 * chain's order, and for hosts that drive one process per GPU. */
fltee_status_t fltee_krum_gram_ranges_device(const void *d_in, int packed, size_t n, size_t d,
                                             uint32_t ranks, double *d_G_out);
/* Process-wide, like fltee_set_dense_trim; (0, 0) is off and the default: every call is then
 * launch for launch what it was.  On: an ecall_secure_aggregation call on the dense path of algs
 * 3, 4, 5 (a dense upload in position, records or value rows; the staged and the pipelined path
 * alike) is aggregated with FLTEE_OPT_KRUM, krum_f = f, krum_m = m, on the n' clients actually
 * aggregated (the survivors under FLTEE_AEAD_DROP: the gather, the selection and the divisor m
 * agree on n'); the DP noise is divided by m.  A host that switched Multi-Krum on never gets a
 * plain mean back: what cannot be answered ends with 0x2, with the existing 0x2 refusals ([out]
 * zero-filled, the timers written, the round kept) — algs 1, 2, 6 and 7, a sparse upload, alg 5
 * under fltee_set_path_oram_tree(1), n' < 2 f + 3, m = 0, m > n' - f, n > FLTEE_KRUM_MAX_N,
 * fltee_set_dense_trim on at the same time, and a dense-sized records upload out of position.
 * On an eid over several GPUs a records call is sharded by column, cut on the Gram pass's chunk
 * boundaries: after the one verdict every GPU runs the Gram kernels on its columns, a carry chain
 * adds the chunks' partials rank after rank in the one-GPU order (fltee_krum_gram_ranges_device
 * above states it), the root scores and ranks on the resulting G, the n keep words go to every
 * GPU device to device, and each sums the kept clients over its columns: the one-GPU bits.  (A
 * packed, bf16 or fp8 call is loaded and run on the root.)  Nothing new is revealed: the launch
 * shapes depend on (n', d), the eid's size and the buffers' alignment; the keep set is never read
 * back. */
void fltee_set_dense_krum(uint32_t f, uint32_t m);

/* ---- robust aggregation: the geometric median behind the ECALL --------------------------------
 * Multi-Krum is a hard selection: it needs a guess of f and drops n - m honest updates a round.
 * The geometric median (FLTEE_OPT_GMED above) needs no f, tolerates any minority of corrupted
 * clients and keeps every honest client with a smooth weight. */
/* Steps 1 - 5 of FLTEE_OPT_GMED alone, device-resident: d_records is n dense uploads of d
 * parameters (records, or the layout opts' row flag names; FLTEE_OPT_DENSE is implied), opts is
 * the base of a fltee_device_opts_gmed with FLTEE_OPT_GMED set (INVALID_PARAMETER without the
 * flag) and gives gmed_iters, gmed_nu and, with FLTEE_OPT_CLIP, the bound (the other options are
 * ignored).  Leaves the n weights alpha (f32) in d_alpha and the last iteration's n distances rho
 * (f64; +inf for an invalid client) in d_rho, device memory both; asynchronous on `stream`.  The
 * refusals and the scratch are those of the aggregate call on alg 3.  For tests, and for hosts
 * that drive one process per GPU. */
fltee_status_t fltee_gmed_weights_device(const void *d_records, size_t n, size_t d,
                                         const fltee_device_opts *opts, float *d_alpha,
                                         double *d_rho, void *stream);
/* Process-wide, like fltee_set_dense_krum; (0, anything) is off and the default: every call is
 * then launch for launch what it was.  On: an ecall_secure_aggregation call on the dense path of
 * algs 3, 4, 5 (records or value rows; the staged and the pipelined path alike) is aggregated
 * with FLTEE_OPT_GMED, gmed_iters = iters, gmed_nu = nu, on the n' clients actually aggregated
 * (the survivors under FLTEE_AEAD_DROP); the DP noise is divided by n'.  A host that switched the
 * geometric median on never gets a plain mean back: what cannot be answered ends with 0x2, with
 * the existing 0x2 refusals — algs 1, 2, 6 and 7, a sparse upload, alg 5 under
 * fltee_set_path_oram_tree(1), n > FLTEE_KRUM_MAX_N, iters > FLTEE_GMED_MAX_ITERS, a nu that is
 * not a finite value above 0, fltee_set_dense_trim or fltee_set_dense_krum on at the same time,
 * and a dense-sized records upload out of position.  On an eid over several GPUs a records call
 * is sharded by column as a Multi-Krum call is: the Gram passes and their carry chain on the
 * GPUs, the iterations on the root's G, the n weights and n valid words to every GPU device to
 * device, the weighted sums per column slice: the one-GPU bits.  (A packed, bf16 or fp8 call is
 * loaded and run on the root.)  Nothing new is revealed: the launch shapes depend on (n', d,
 * iters), the eid's size and the buffers' alignment; the weights are never read back. */
void fltee_set_dense_gmed(uint32_t iters, double nu);

/* ---- authenticated uploads: AES-128-GCM (NIST SP 800-38D), 96-bit IV, 128-bit tag ------
 * Per client: K = the session key, H = E_K(0^128), J0 = IV || 0x00000001, keystream block
 * i = E_K(IV || BE32(2 + i)), T = GHASH_H(AAD || pad || C || pad || BE64(8 |AAD|) ||
 * BE64(8 |C|)) ^ E_K(J0).  GHASH runs on the GPU in constant time (k_ghash.hip), in
 * segments of FLTEE_GCM_SEGMENT_BLOCKS 16-byte blocks.  Refused by host arithmetic with
 * FLTEE_ERROR_INVALID_PARAMETER: aad_len > 64, ct_bytes > 2^36 - 32 (the 32-bit counter
 * would wrap), and for the producer a ct_bytes that is no multiple of 8 (whole records). */
#define FLTEE_GCM_SEGMENT_BLOCKS 512
#define FLTEE_GCM_TAG_BYTES 16
#define FLTEE_GCM_MAX_AAD 64
/* n slices of (ct_bytes || 16-byte tag) at stride ct_bytes+16; one 12-byte IV for the call;
 * aad: n x aad_len bytes (aad_len <= 64, may be 0).  Writes n * floor(ct_bytes/8) records and
 * d_fail[n] (u32 0/1); ORs FLTEE_DEV_ERR_AUTH into the status word on any mismatch.  The
 * computed tags never leave the device. */
fltee_status_t fltee_decrypt_auth_device(const uint32_t *client_ids, size_t n, const void *d_cipher,
                                         size_t ct_bytes, const uint8_t iv[12], const uint8_t *aad,
                                         size_t aad_len, void *d_records, uint32_t *d_fail,
                                         void *stream);
/* the inverse: the client producer (ciphertext || tag per client); n slices of ct_bytes of
 * plaintext in, n slices of ct_bytes + 16 out */
fltee_status_t fltee_encrypt_auth_device(const uint32_t *client_ids, size_t n, const void *d_plain,
                                         size_t ct_bytes, const uint8_t iv[12], const uint8_t *aad,
                                         size_t aad_len, void *d_cipher, void *stream);
/* the same tag computed on the host by the same multiply (no GPU): for CPU tests */
fltee_status_t fltee_debug_gcm_tag_host(uint32_t client_id, const uint8_t iv[12], const uint8_t *aad,
                                        size_t aad_len, const uint8_t *ct, size_t ct_len,
                                        uint8_t tag[16]);
/* ---- the pieces of a COLUMN-SHARDED authenticated decrypt (device-resident, in the style of
 * the fltee_*_range_device pieces): W workers each hold a window of every client's slice —
 * the ciphertext blocks [first_block, first_block + ceil(win_bytes / 16)), n rows at
 * row_stride bytes — and together verify and decrypt what fltee_decrypt_auth_device does on
 * whole slices.  GHASH right-aligns a slice's AAD and ciphertext blocks in
 * P = fltee_gcm_segments(ct_bytes, aad_len) segments of FLTEE_GCM_SEGMENT_BLOCKS blocks and
 * keeps one 16-byte partial per segment; a partial is XOR-linear in its blocks, so
 *   1. every worker: fltee_ghash_window_device -> its d_part (n x P x 16 bytes; segments its
 *      window does not touch are zero); exactly one window of the slices passes with_aad = 1;
 *   2. fltee_ghash_merge_device: d_acc ^= d_part, once per other worker;
 *   3. fltee_gcm_finish_device on the merged partials and the n received tags (n x 16 bytes,
 *      a buffer of their own: no worker's window has them behind it): d_fail[c] = 0 / 1 and
 *      FLTEE_DEV_ERR_AUTH into the status word; the computed tags never leave the device;
 *   4. every worker: fltee_decrypt_slice_auth_device, the CTR half alone on its window
 *      (keystream block i of a row = E_K(IV || BE32(2 + first_block + i))) ->
 *      n x floor(win_bytes / 8) records, compact.
 * A partial is the field element as the kernels hold it: the 16 bytes of the GCM block, each
 * byte with its bits reversed.  Refused with FLTEE_ERROR_INVALID_PARAMETER by host arithmetic,
 * before any device call: aad_len > 64, ct_bytes > 2^36 - 32, a window that starts past the
 * slice (16 first_block > ct_bytes), reaches past ct_bytes, or ends off a 16-byte boundary
 * anywhere but at ct_bytes, and row_stride < win_bytes. */
size_t fltee_gcm_segments(size_t ct_bytes, size_t aad_len);
/* aad: n x aad_len bytes, read with with_aad != 0 only (aad_len shapes the layout either way) */
fltee_status_t fltee_ghash_window_device(const uint32_t *client_ids, size_t n, const void *d_window,
                                         size_t row_stride, size_t ct_bytes, size_t first_block,
                                         size_t win_bytes, const uint8_t *aad, size_t aad_len,
                                         int with_aad, void *d_part, void *stream);
fltee_status_t fltee_ghash_merge_device(void *d_acc, const void *d_part, size_t n, size_t P,
                                        void *stream);
fltee_status_t fltee_gcm_finish_device(const uint32_t *client_ids, size_t n, const void *d_part,
                                       size_t ct_bytes, const uint8_t iv[12], size_t aad_len,
                                       const void *d_tags, uint32_t *d_fail, void *stream);
fltee_status_t fltee_decrypt_slice_auth_device(const uint32_t *client_ids, size_t n,
                                               const void *d_window, size_t row_stride,
                                               size_t first_block, size_t win_bytes,
                                               const uint8_t iv[12], void *d_records, void *stream);
/* one client's window partials (P x 16 bytes) on the host by the same multiply (no GPU): for
 * CPU tests; aad: this client's aad_len bytes; ct_window: the window's win_bytes bytes */
fltee_status_t fltee_debug_ghash_window_host(uint32_t client_id, const uint8_t *aad, size_t aad_len,
                                             int with_aad, const uint8_t *ct_window, size_t ct_bytes,
                                             size_t first_block, size_t win_bytes, uint8_t *part_out);
/* The ECALLs' upload format.  Off (default): plain AES-128-CTR with a zero counter block, as
 * lib.rs:312-343 and every earlier version of this library.  On: client c's slice is
 * ciphertext (B bytes) || tag (16 bytes) of the scheme above with
 *     IV  = BE32(fl_id) || BE32(round) || BE32(0)
 *     AAD = BE32(fl_id) || BE32(round) || BE32(client_id) || BE32(aggregation_alg)
 * (a packed call, fltee_set_upload_packed: BE32(aggregation_alg | 0x80000000); a bf16 call,
 * fltee_set_upload_bf16: BE32(aggregation_alg | 0x40000000); an fp8 call,
 * fltee_set_upload_fp8: BE32(aggregation_alg | 0x20000000)),
 * so encrypted_parameters_size = n (B + 16) (alg 6 reads client_size (k 8 + 16) bytes) and
 * the records per client are floor(B / 8).  The existing refusals come first and stay 0x2;
 * a slice whose tag does not verify ends the call with *retval = FLTEE_ERROR_MAC_MISMATCH
 * before any aggregation is launched, [out] zero-filled, the round not advanced.  An eid over
 * several GPUs shards the authenticated ECALL as it shards the plain one, under the same
 * contract and with the one-GPU bits: dense uploads by parameter range — every GPU copies,
 * decrypts and hashes its own columns (the pieces above), the root XORs the partials, checks
 * the tags and reads one verdict before any GPU sums; the position-range routes (algs 1, 2,
 * 7) and alg 6's batches by whole clients — every GPU verifies the clients it loads, and the
 * GPUs' verdicts are read before anything is sorted or folded.  A shape the group declines
 * runs authenticated on the root. */
void fltee_set_upload_aead(int on);

/* What an authenticated ECALL does after its verdict (process-wide, like fltee_set_upload_aead;
 * no effect while AEAD is off).  The device holds one fail word per client.
 *   ABORT  (default): as above, and as every earlier version: only the OR of the fail words is
 *          read; a failure ends the call with 0x3001 and the host learns nothing more.
 *   REPORT: the call ends as under ABORT, but the one readback of the verdict also takes the n
 *          fail words ((n + 1) * 4 bytes, a function of n alone, at the same place and the same
 *          synchronisation), and fltee_auth_report names the clients that failed.
 *   DROP:  the verdict is kept, and the call aggregates the verified clients.  With S = the
 *          verified clients in upload order and n' = |S| >= max(1, min_survivors): *retval = 0,
 *          the timers are written, the round advances, and [out] is bit for bit what the same
 *          ECALL on the same kind of eid returns for the clients of S alone (their ids, their
 *          slices in order, client_size = n'): the 1/n' average, the DP noise divisor, nips19's
 *          threshold and alg 6's batches (re-formed over S in order) all take n'; nips19 and DP
 *          draw their seeds once per call.  With fewer survivors the call ends as under REPORT.
 *          The 0x2 refusals come first and are evaluated on the request as sent.  A clean call
 *          runs the launches it runs under ABORT.  After a failing verdict the records of S are
 *          compacted into a second buffer (fltee_gather_clients_device's kernel; its scratch is
 *          reserved on this path only) and the launch shapes depend on the public sizes and on
 *          the failed set — which the host can cause, and reads from the report.  On an eid
 *          over several GPUs a group path that read a failing verdict stops before any
 *          aggregation launch, as under ABORT; under REPORT and DROP the root alone then loads
 *          and verifies the whole payload again (for the per-client words) and, under DROP,
 *          aggregates the survivors: the one-GPU bits, the second load paid only by a call with
 *          a failure.  A payload past one gather launch (n or k above 2^32 - 1, or more than
 *          2^31 - 1 blocks of 2048 records) is not dropped from: such a call ends as under
 *          REPORT. */
#define FLTEE_AEAD_ABORT 0
#define FLTEE_AEAD_REPORT 1
#define FLTEE_AEAD_DROP 2
void fltee_set_upload_aead_policy(int policy, size_t min_survivors /* 0 = 1 */);
/* The verdict of the last authenticated ECALL of fl_id under REPORT / DROP (either ECALL; it
 * is overwritten by every such call, a clean one stores an empty list, and ecall_fl_init of
 * that fl_id forgets it): the failed client ids in upload order into failed_ids[0 .. cap);
 * *n_failed is the full count even when cap is smaller; *round = the round that call was for.
 * Nothing stored (ABORT, AEAD off, no call yet): *n_failed = 0 and *round = the config's
 * current round.  FLTEE_ERROR_UNEXPECTED (0x1) for an unknown fl_id, answered before the eid
 * is looked at (the configs are process-wide); 0x2 for a null n_failed. */
fltee_status_t fltee_auth_report(fltee_eid_t eid, uint32_t fl_id, uint32_t *round,
                                 uint32_t *failed_ids, size_t cap, size_t *n_failed);
/* The survivors gather, device-resident: d_out[s][0 .. k) = d_records[d_keep[s]][0 .. k) for
 * s < n_keep, on n x k records of 8 bytes; d_keep (ascending client positions) is device
 * memory; d_out must not overlap d_records (never in place: with client 0 dropped slice s of
 * the output lies over slice s - 1 of the input).  16-byte loads and stores where a source
 * and a destination slice agree modulo 16, 8-byte records otherwise.  Asynchronous on
 * `stream`; n_keep = 0 writes nothing.  Refused with FLTEE_ERROR_INVALID_PARAMETER by host
 * arithmetic, before any device call: a null pointer, n_keep > n, k == 0, n * k >= 2^31.  A
 * d_keep[s] >= n is clamped (nothing is read out of bounds) and ORs FLTEE_DEV_ERR_LAUNCH into
 * the library's status word (fltee_device_status). */
fltee_status_t fltee_gather_clients_device(const void *d_records, size_t n, size_t k,
                                           const uint32_t *d_keep, size_t n_keep, void *d_out,
                                           void *stream);

/* out[j] = coef * sum_r rows[r*d + j], rows added in order (exact fp32): the
 * root-side combine of per-GPU partial sums, in the batch order of alg 6
 * (lib.rs:564-573: global[i] += batch_sum[i], then average). */
fltee_status_t fltee_sum_rows_device(const float *d_rows, size_t nrows, size_t d, float coef,
                                     float *d_out, void *stream);

/* common.rs:56-72 on a device vector: out[i] += (N(0, clipping*sigma) / n) as f32. */
fltee_status_t fltee_dp_noise_device(float *d_out, size_t d, float sigma, float clipping,
                                     size_t n, uint64_t seed, void *stream);

/* Synchronise `stream` and return (and clear) the library's status word. */
fltee_status_t fltee_device_status(void *stream, uint32_t *status);

/* ---- intermediate stages, exposed for the permutation-parity tests ------ */
/* In-place oblivious bitonic network on M = 2^m 8-byte records.
 * mode 0: sort by u32 idx with the reference comparator (advanced.rs:147-176)
 * mode 1: sort by the whole u64 (stable-by-construction composite keys)
 * mode 2: keyed shuffle network (nips19.rs:66-105 structure, seed)          */
fltee_status_t fltee_bitonic_device(void *d_records, size_t m, uint32_t mode, uint32_t seed,
                                    void *stream);
/* In-place stable oblivious network of alg 7 on m = 2^j (<= 2^29) 16-byte records
 * {u64 key; f32 val; u32 pad}: ascending by key alone (keys distinct, except identical
 * pads key = ~0, val = +0.0).  Any other m: FLTEE_ERROR_INVALID_PARAMETER. */
fltee_status_t fltee_stable_sort_device(void *d_records16, size_t m, void *stream);
/* advanced.rs:66-101 fold over [0, fold_len) of src (length m) into dst. */
fltee_status_t fltee_fold_device(const void *d_src, void *d_dst, size_t m, size_t fold_len,
                                 size_t halo, uint32_t *d_status, void *stream);
/* common.rs:77-98,151-161 — nips19 Laplace counts r[d] and threshold T. */
fltee_status_t fltee_laplace_r_device(size_t d, size_t k, size_t n, uint64_t seed, uint32_t *d_r,
                                      float *T_out, void *stream);

/* ---- position-range pieces of `advanced` (multi-GPU, SURVEY §8e Option B) --
 * The padded array of advanced.rs:116-142 (M = 2^m entries) is split into W
 * contiguous ranges of m = M/W records, one per GPU; range r holds global
 * positions [r*m, (r+1)*m).  Run on every range, in this order, these pieces are
 * the reference's network and fold step for step (fl-tee_amd/fltee/parallel.py
 * drives them over RCCL):
 *   init_range -> range_sort -> for each stage 2^s > m: (range_exchange with the
 *   partner range for every step 2^j >= m) then range_merge -> fold_range ->
 *   compact_range -> sum of the W outputs (RCCL reduce) on the root.          */
/* entries pos_base .. pos_base+m-1 of records ++ (i, 0.0) for i < d ++ (u32::MAX,
 * 0.0) pads (advanced.rs:116-142); d_records holds the records at positions
 * pos_base.. (read where position < nrec). */
fltee_status_t fltee_advanced_init_range_device(const void *d_records, size_t nrec, size_t d,
                                                size_t pos_base, size_t m, void *d_dst,
                                                void *stream);
/* stages 2 .. m of the bitonic network (advanced.rs:147-176) on one range; the
 * direction of every compare-exchange comes from its GLOBAL position. */
fltee_status_t fltee_bitonic_range_sort_device(void *d_records, size_t m, size_t pos_base,
                                               uint32_t mode, uint32_t seed, void *stream);
/* the same, knowing that entries valid .. m-1 of the range are identical (u32::MAX,
 * +0.0) pads (valid >= m: none): stage blocks made of pads alone are skipped, which
 * leaves them as they are — the same permutation.  valid = 0: nothing to do. */
fltee_status_t fltee_bitonic_range_sort_padded_device(void *d_records, size_t m, size_t pos_base,
                                                      size_t valid, uint32_t mode, uint32_t seed,
                                                      void *stream);
/* the steps j = m/2 .. 1 of stage 2^stage_log (> m) on one range. */
fltee_status_t fltee_bitonic_range_merge_device(void *d_records, size_t m, size_t pos_base,
                                                uint32_t mode, uint32_t seed, uint32_t stage_log,
                                                void *stream);
/* the step j = |pos_mine - pos_theirs| (>= m, a power of two) of stage 2^stage_log
 * between this range and a copy of its partner's: d_mine takes the partner's
 * record wherever that compare-exchange swaps. */
fltee_status_t fltee_bitonic_range_exchange_device(void *d_mine, const void *d_theirs, size_t m,
                                                   size_t pos_mine, size_t pos_theirs,
                                                   uint32_t mode, uint32_t seed,
                                                   uint32_t stage_log, void *stream);
/* the steps j = 2^step_top .. 2^step_bot (< m, step_top < stage_log) of stage
 * 2^stage_log on one range (register passes).  Mode 0 only needs directions, so a
 * range whose position bits were permuted by an all-to-all can run its cross-range
 * steps locally through this call (fltee/parallel.py, transposed exchange). */
fltee_status_t fltee_bitonic_range_steps_device(void *d_records, size_t m, size_t pos_base,
                                                uint32_t mode, uint32_t seed, uint32_t stage_log,
                                                uint32_t step_top, uint32_t step_bot,
                                                void *stream);
/* records of context the fold needs in front of a range: halo rounded up to 16 (the
 * range fold reads one more record in front, see below). */
size_t fltee_fold_context(size_t halo);
/* advanced.rs:66-101 on [origin, end) of d_src (length m, global position =
 * pos_base + local): [0, origin) holds >= fltee_fold_context(halo) + 1 records of the
 * previous range, d_src[end] the next range's first record (unless end + pos_base
 * >= fold_len).  Writes d_dst[origin, end) and the fold's side records into d_side
 * (fltee_fold_side_bytes(end - origin, halo) bytes).  Runs of any length (a client
 * repeating an index): a run begun before a walk boundary is finished by the patch
 * below — bit for bit for every run of <= halo + 1 entries, re-associated at the
 * walk boundaries beyond. */
size_t fltee_fold_side_bytes(size_t span, size_t halo);
fltee_status_t fltee_fold_range_device(const void *d_src, void *d_dst, size_t m, size_t origin,
                                       size_t end, int64_t pos_base, size_t fold_len, size_t halo,
                                       void *d_side, void *stream);
/* the range's segmented total (16 bytes into d_total) from its side records: the
 * carry the ranges after it need */
fltee_status_t fltee_fold_range_total_device(const void *d_side, size_t span, size_t halo,
                                             void *d_total, void *stream);
/* the long-run patch of one range's fold output d_dst (the same origin, end, pos_base,
 * fold_len and halo as fltee_fold_range_device): d_prev_totals = the totals of the
 * n_prev ranges before this one, in range order.  Writes every walk's first position
 * (fixed addresses). */
fltee_status_t fltee_fold_range_patch_device(void *d_dst, size_t origin, size_t end,
                                             int64_t pos_base, size_t fold_len, size_t halo,
                                             const void *d_side, const void *d_prev_totals,
                                             size_t n_prev, void *stream);
/* one folded range (c records) -> d_out[d]: val * coef at each run representative's
 * index i < d held by this range, +0.0 elsewhere (oblivious compaction; scratch
 * d_buf, d_tmp of d + c records each).  The sum of every range's d_out is the
 * aggregate, bit for bit. */
fltee_status_t fltee_compact_range_device(const void *d_chunk, size_t c, size_t d, void *d_buf,
                                          void *d_tmp, float coef, float *d_out, void *stream);

/* ---- position-range pieces of alg 7's stable network (multi-GPU) ----------
 * The padded array of alg 7 (M = 2^j entries of 16 bytes {u64 key = idx << 32 | global
 * position; f32 val; u32 pad}) split into W contiguous ranges of m = M/W records; range r
 * holds global positions [r*m, (r+1)*m).  Run on every range, in this order, these pieces
 * are fltee_stable_sort_device's network step for step:
 *   init_range -> range_sort -> for each stage 2^s > m: (range_exchange with the partner
 *   range for every step 2^j >= m, j = s-1 .. log2 m) then range_merge -> range_strip ->
 *   the fold / compaction pieces of `advanced` above.
 * Every piece refuses, by host arithmetic before any device call, with
 * FLTEE_ERROR_INVALID_PARAMETER: m not a power of two, m < 2^12 (one LDS tile) or m > 2^29,
 * a position that is not a multiple of m, or a range ending past 2^31. */
/* entries pos_base .. pos_base+m-1 of records ++ (i, 0.0) for i < d ++ pads (key ~0,
 * +0.0), each keyed with its global position; d_records holds the records at positions
 * pos_base.. (read where position < nrec).  nrec + d < 2^31. */
fltee_status_t fltee_stable_init_range_device(const void *d_records, size_t nrec, size_t d,
                                              size_t pos_base, size_t m, void *d_dst16, void *stream);
/* stages 1 .. log2 m of the network on one range; the direction of every compare-exchange
 * comes from its GLOBAL position.  Entries valid .. m-1 of the range are identical pads
 * (valid >= m: none): stage blocks made of pads alone are skipped, which leaves them as
 * they are.  valid = 0: nothing to do. */
fltee_status_t fltee_stable_range_sort_device(void *d_rec16, size_t m, size_t pos_base,
                                              size_t valid, void *stream);      /* stages 1..log2 m */
/* the step j = |pos_mine - pos_theirs| (>= m, a power of two: the two positions differ in
 * that one bit) of stage 2^stage_log (> j) between this range and a copy of its partner's:
 * d_mine[x] becomes the smaller or the larger of (d_mine[x], d_theirs[x]) by key — the
 * smaller exactly when (this range is the lower one) == (bit stage_log of pos_mine is 0).
 * Also refused: pos_mine == pos_theirs, a distance that is no power of two, stage_log not
 * above log2 of the distance. */
fltee_status_t fltee_stable_range_exchange_device(void *d_mine16, const void *d_theirs16, size_t m,
                                                  size_t pos_mine, size_t pos_theirs,
                                                  uint32_t stage_log, void *stream);
/* the steps j = m/2 .. 1 of stage 2^stage_log (> m, else refused) on one range. */
fltee_status_t fltee_stable_range_merge_device(void *d_rec16, size_t m, size_t pos_base,
                                               uint32_t stage_log, void *stream); /* steps m/2..1 of a stage > m */
/* m 16-byte records -> the fold's 8-byte (idx, val) records; a pad becomes (u32::MAX, +0.0). */
fltee_status_t fltee_stable_range_strip_device(const void *d_rec16, size_t m, void *d_dst8, void *stream);

/* nips19 by position range (the shuffle is the same kind of network): entries
 * pos_base .. pos_base+m-1 of records ++ d*tf Laplace dummies (common.rs:189-197;
 * d_r from fltee_laplace_r_device, tf = (usize)T) ++ (u32::MAX, 0.0) pads; and
 * safe_aggregate (common.rs:25-35) of m entries into d_out[d] (zeroed first,
 * un-averaged: the ranges' partial sums are added by the caller's reduce). */
fltee_status_t fltee_nips19_build_range_device(const void *d_records, size_t nrec,
                                               const uint32_t *d_r, size_t d, size_t tf,
                                               size_t pos_base, size_t m, void *d_dst,
                                               void *stream);
fltee_status_t fltee_safe_aggregate_device(const void *d_src, size_t m, size_t d, float *d_out,
                                           void *stream);
/* safe_aggregate split over ranges, bit-exact: the entries of one range with idx < d in
 * position order into d_list (at most cap; *count = how many there are, also when they
 * do not fit: INVALID_PARAMETER), synchronising `stream`; then, on the root, the ordered
 * fold of the ranges' lists concatenated in range order (the shuffled order):
 * d_out[i] = coef * (+0 + v1 + v2 ...) over the entries with idx i. */
fltee_status_t fltee_select_device(const void *d_src, size_t m, size_t d, void *d_list,
                                   size_t cap, size_t *count, void *stream);
fltee_status_t fltee_ordered_list_device(const void *d_list, size_t lc, size_t d, float coef,
                                         float *d_out, void *stream);
/* Test hook: the stable sort that fold runs, alone: the n 8-byte records of d_rec in
 * order of min(idx, d), upload order within an index (the records with idx >= d last,
 * and FLTEE_DEV_ERR_INDEX_RANGE in the library's status word), into d_sorted (another
 * buffer of n records).  n < 2^29, d >= 1. */
fltee_status_t fltee_debug_sort_records_device(const void *d_rec, size_t n, size_t d,
                                               void *d_sorted, void *stream);

/* Test hooks: deterministic RNG seed for sampling / nips19 / DP (0 = off). */
/* The ECALLs' path_oram (aggregation_alg 5): on = the tree Path ORAM of oram.rs:64-118
 * (Z = 4, stash 20, next_pow2(d) blocks, oram.rs's access sequence; k_oram.hip) where
 * next_pow2(d) <= 2^22, the sweep beyond; off (default) = the output-equivalent oblivious
 * sweep.  Both give the in-order sum bit for bit.  The device API selects it per call
 * with FLTEE_OPT_ORAM_TREE. */
void fltee_set_path_oram_tree(int on);
/* The ECALLs' advanced and alg 6 when some index has a run of more than n + 1 entries
 * (a client repeated an index inside its upload; fl_main.py's top-k never does):
 * off (default) = the fixed-cost fold with its long-run carry: such a run's sum is the
 * enclave's re-associated at the fold's walk boundaries (runs of <= n + 1 entries bit for
 * bit); on = the enclave's exact fold for ANY run length (advanced.rs:66-101), at the
 * public worst-case cost: one sequential walk of the whole sorted array whatever the data. */
void fltee_set_advanced_exact_runs(int on);
/* ecall_secure_aggregation with aggregation_alg 7 (lib.rs:389, FLTEE_ALG_BUBBLE): off
 * (default) = refused with 0x2, as every earlier version of this library did; on = answered
 * with the enclave's in-order result (the staged and the pipelined path, DP, the round
 * counter).  On an eid over several GPUs it is sharded by position range — the stable
 * network over W ranges of C = M / W records, each GPU loading and decrypting the clients
 * of its own range, then advanced's halo fold, compaction and reduce: the same bits —
 * except for the shapes the group declines, which the root runs alone as before: C < 2^12,
 * C < 16 W, a fold context (n rounded up to 16, plus 16) above C, M > 2^29, a request
 * k other than the payload's, and everything under fltee_set_advanced_exact_runs(1).
 * A host that sends alg 7 switches it on once at start-up.  The device API (fltee_aggregate_device) answers alg 7
 * whatever this says. */
void fltee_set_bubble_ecall(int on);
void fltee_debug_set_seed(uint64_t seed);
/* Library build/version string. */
const char *fltee_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLTEE_AGG_H */
