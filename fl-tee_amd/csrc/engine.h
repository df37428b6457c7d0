// engine.h — per-device state and the internal aggregation entry points.
#pragma once
#include <mutex>
#include <vector>

#include "common.h"

namespace fltee {

constexpr int kMaxDevices = 64;

struct Buffer {
    void *ptr = nullptr;
    size_t cap = 0;
    uint32_t grow_bit = 0;       // engine scratch: its bit of the growth mask (1 << Ws), set when it grows
    bool reserve(size_t bytes);  // grow-only hipMalloc
    void release();              // hipFree (the owning device must be current)
};

// grow-only pinned host memory (the ECALL's staging: one DMA each way per call)
struct HostBuffer {
    void *ptr = nullptr;   // host address
    void *dptr = nullptr;  // the same pinned bytes as kernels address them (zero-copy)
    size_t cap = 0;
    bool reserve(size_t bytes);
};

// The engine's scratch buffers (DeviceCtx::ws_*) in the one order everything that lists
// them uses: Plan::bytes, fltee_debug_plan's sizes, the bits of fltee_debug_scratch_grown.
enum Ws { kWsA, kWsB, kWsMat, kWsR, kWsCoef, kWsRec, kWsKeys, kWsRadix, kWsOram, kWsSide,
          kWsLb, kWsS16, kWsCnt, kWsSel, kWsCount };

// What aggregate() runs for a public shape (Plan::route), and for the `advanced` family how
// the array is folded and brought to out after its first sort (AdvShape::tail).
enum Route : uint32_t {
    kRouteNone,          // refused before a route was chosen (unknown alg)
    kRouteDense,         // flat algs, FLTEE_OPT_DENSE: the dense accumulate
    kRouteScatterRows,   // non_oblivious: scatter into per-client rows
    kRouteCountingFold,  // non_oblivious: ordered fold in the counting sort's order
    kRouteFlatOrdered,   // baseline / path_oram, k == d: ordered fold by the composite-key network
    kRouteSweep,         // baseline / path_oram: the ordered sweep
    kRouteTree,          // path_oram as the tree Path ORAM
    kRouteTreeLazy,      // ... one access per record, readout through advanced's network
    kRouteAdvanced,
    kRouteBubble,        // alg 7: the stable network, then advanced's tail
    kRouteOptimized,     // alg 6: advanced per batch
    kRouteNips19,
    kRoutePacked,        // flat algs, FLTEE_OPT_PACKED: the packed accumulate (k_rows.hip)
    kRouteTrimDense,     // flat algs, FLTEE_OPT_TRIM with t > 0 on records: the trimmed mean (k_trim.hip)
    kRouteTrimPacked,    // ... on packed rows
    kRouteBf16,          // flat algs, FLTEE_OPT_BF16: the bf16 accumulate (k_rows.hip)
    kRouteTrimSelectDense,   // FLTEE_OPT_TRIM | _TRIM_SELECT with t > 0 on records: trim by selection (k_trim_select.hip)
    kRouteTrimSelectPacked,  // ... on packed rows
    kRouteFp8,           // flat algs, FLTEE_OPT_FP8: the fp8 accumulate (k_rows.hip)
    kRouteKrumDense,     // flat algs, FLTEE_OPT_KRUM on records: Multi-Krum (k_krum.hip; its scratch in ws_mat)
    kRouteKrumPacked,    // ... on packed rows
    kRouteGmedDense,     // flat algs, FLTEE_OPT_GMED on records: the geometric median (k_gmed.hip; its scratch in ws_mat)
    kRouteGmedPacked,    // ... on packed rows
};
enum Tail : uint32_t {
    kTailNone,
    kTailFused,     // the fold inside the compaction's first pass (k_compact.hip fc_shape)
    kTailStream,    // the streaming fold over the compaction's prefix, then the compaction
    kTailOneEntry,  // d = 1 and no records: the one entry copied, then the compaction
    kTailSort,      // k_req != k (or the compaction switched off): fold, then the full second sort
};

// One `advanced` network: n clients' k records over d parameters, folded over fold_len.
struct AdvShape {
    size_t nrec = 0, d = 0, L = 0, M = 0, fold_len = 0;
    size_t halo = 0;    // the effective one: opts.fold_halo, or n
    size_t span = 0;    // positions the separate fold covers (kTailStream: the compaction's prefix)
    Tail tail = kTailNone;
    bool stable = false;  // alg 7: the first sort is the stable network's (k_stable.hip)
    size_t side_bytes = 0, lb_bytes = 0;
};

// A call's options as the engine holds them: the public struct, and behind it the fields of
// fltee_device_opts_krum (read_opts fills them under FLTEE_OPT_KRUM; zero otherwise) and of
// fltee_device_opts_gmed (under FLTEE_OPT_GMED).
struct EngineOpts : fltee_device_opts {
    size_t krum_f, krum_m;
    size_t gmed_iters;
    double gmed_nu;
};

// The one decision about a call's public shape (alg, n, k, d, opts): whether it is refused,
// what runs, and the bytes of every scratch buffer that touches.  Host arithmetic only.
// Outside the plan, because they depend on data: nips19's selected list (ws_sel) and the
// ws_keys / ws_radix its ordered fold sizes from the count read back from the device
// (ordered_from_list).
struct Plan {
    fltee_status_t status = FLTEE_SUCCESS;  // else the refusal; the sizes are still filled in
    Route route = kRouteNone;
    bool clip_records = false;  // FLTEE_OPT_CLIP works on a clipped copy of the records
    bool unpack = false;        // FLTEE_OPT_PACKED / _BF16 / _FP8 off their own routes: the records are unpacked into ws_rec
    AdvShape adv;               // advanced, alg 7, an alg-6 batch, the lazy tree's readout (1 x slots)
    AdvShape adv_last;          // alg 6: the short last batch (when n % batch)
    size_t batch = 0;           // alg 6
    size_t tree_slots = 0;      // the tree ORAM's slots (k_oram.hip oram_slots)
    size_t kq = 0, tf = 0, L = 0, M = 0;  // nips19 (nips19.rs:38: T from the REQUEST's k)
    float T = 0.0f;
    size_t sel_tiles = 0;       // nips19: tiles of the shuffle's selecting last pass (0: select apart)
    size_t bytes[kWsCount] = {};
};

struct DeviceCtx {
    bool ready = false;
    int device = -1;
    uint32_t *status = nullptr;  // library-owned device status word
    Buffer ws_a, ws_b, ws_mat, ws_r, ws_coef, ws_rec;  // aggregation scratch
    // bytes of ws_mat (from its start) known to hold the scatter path's empty sentinel:
    // the scatter sum restores every slot it used, so the fill runs once per buffer
    size_t mat_clean = 0, mat_clean_cap = 0;
    void *mat_clean_ptr = nullptr;
    Buffer cipher, records, round_keys, outbuf;         // ECALL staging
    Buffer stage;                                        // small ECALLs: out, status, keys, ciphertext
    HostBuffer pin_in, pin_out;                          // small ECALLs: pinned staging both ways
    hipEvent_t call_ev[3] = {};                          // small ECALLs: the phase timers
    // authenticated uploads (k_ghash.hip): subkeys + AAD, powers of H, partials, fail words
    Buffer gcm_sub, gcm_pow, gcm_part, gcm_fail;
    // FLTEE_AEAD_DROP: the verified clients' records, compacted (k_survivors.hip), their
    // keep list behind them; reserved only by a call that drops a client.  keep_host: the
    // list's host side, alive until the next call (its upload is asynchronous)
    Buffer survivors;
    std::vector<uint32_t> keep_host;
    Buffer ws_client, ws_client_coef;                   // client-side producers
    Buffer ws_cnt, ws_sel;                               // nips19's selected list
    Buffer ws_keys, ws_radix;  // ordered folds: records sorted by idx, the counting sort's scratch
    Buffer ws_oram;            // path_oram tree mode: the tree + stash slots, then their records
    Buffer ws_side;            // advanced's streaming fold: its side records (k_fold.hip)
    Buffer ws_lb;              // the fused fold's look-back slots (k_compact.hip), zeroed
    Buffer ws_s16;             // alg 7: the stable network's 16-byte records (k_stable.hip)
    uint32_t fc_epoch = 0;     // their launch counter
    uint32_t *host_word = nullptr;                       // pinned readback word
    hipStream_t stream = nullptr;                        // ECALL stream
    hipStream_t copy_stream = nullptr;                   // ECALL H2D (pipelined load)
    static constexpr int kCopyEvents = 64;
    hipEvent_t copy_ev[kCopyEvents] = {};
};

// One process-wide lock: the enclave had a single TCS (Enclave.config.xml:6).
std::recursive_mutex &api_mutex();

DeviceCtx *device_ctx(int dev);
DeviceCtx *current_ctx();
uint64_t next_seed();
void set_debug_seed(uint64_t seed);
float nips19_threshold(size_t d, size_t k, size_t n);

// path_oram as the tree Path ORAM for the ECALLs (fltee_set_path_oram_tree); the device
// API selects it per call with FLTEE_OPT_ORAM_TREE
void set_oram_tree(int on);
bool oram_tree_default();
// advanced / alg 6 in the ECALLs: the one-lane sequential fold at the public worst-case
// cost (fltee_set_advanced_exact_runs: the enclave's sums bit for bit for any run length),
// else the halo fold (bit for bit up to n + 1 entries a run, re-associated beyond)
void set_exact_runs(int on);
bool exact_runs_default();
// alg 7 (lib.rs:389) through ecall_secure_aggregation: answered only after
// fltee_set_bubble_ecall(1); off (default) it stays the 0x2 it has always been
void set_bubble_ecall(int on);
bool bubble_ecall_default();

fltee_status_t aggregate(uint32_t alg, const void *rec, size_t n, size_t k, size_t d, float *out,
                         const EngineOpts &o, hipStream_t s, uint32_t *status);
// a FLTEE_OPT_KRUM call up to its selection: the n scores and keep words copied to sel_scores /
// sel_keep (device memory), nothing written to an output
fltee_status_t krum_select(const void *rec, size_t n, size_t d, const EngineOpts &o, double *sel_scores,
                           uint32_t *sel_keep, hipStream_t s, uint32_t *status);
// a FLTEE_OPT_GMED call up to its weights: the n alpha and the last iteration's n rho copied to
// sel_alpha / sel_rho (device memory), nothing written to an output
fltee_status_t gmed_weights(const void *rec, size_t n, size_t d, const EngineOpts &o, float *sel_alpha,
                            double *sel_rho, hipStream_t s, uint32_t *status);
// common.rs:25-35 on m entries of src (the shuffled array), bit-exact: out[i] = coef *
// (+0 + v1 + v2 ...) over the entries with idx == i in position order (accumulate:
// out[i] += the un-scaled sum).  Synchronises `s` once to read the selected count.
hipError_t safe_aggregate_ordered(DeviceCtx *c, const uint64_t *src, size_t m, size_t d,
                                  float coef, float *out, bool accumulate, uint32_t *status,
                                  hipStream_t s);
// the selected list sel[0, lc) (nips19 entries with idx < d, in shuffled order) -> out
hipError_t ordered_from_list(DeviceCtx *c, const uint64_t *sel, size_t lc, size_t d, float coef,
                             float *out, bool acc, uint32_t *status, hipStream_t s);
// one alg-6 batch: `advanced` of n clients into out[d], un-averaged (current device)
hipError_t advanced_batch(const void *rec, size_t n, size_t k, size_t d, size_t halo, float *out,
                          uint32_t *status, hipStream_t s);
hipError_t read_device_word(DeviceCtx *c, const uint32_t *dev_word, size_t *out, hipStream_t s);
size_t workspace_bytes(uint32_t alg, size_t n, size_t k, size_t d, const EngineOpts &o);
bool reserve(uint32_t alg, size_t n, size_t k, size_t d, const EngineOpts &o);
// the plan's refusal alone (host arithmetic)
fltee_status_t plan_status(uint32_t alg, size_t n, size_t k, size_t d, const EngineOpts &o);

}  // namespace fltee
