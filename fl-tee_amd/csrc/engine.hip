// engine.hip — device-side orchestration of the aggregation algorithms.
//
// fltee_aggregate_device() is the aggregation of ecall_secure_aggregation
// (lib.rs:355-408) on records already decrypted into HBM: the dispatcher on
// aggregation_alg (lib.rs:359-397), optional DP noise (lib.rs:399-408), with
// the enclave's 1f32/n averaging (common.rs:14-19).  Scratch HBM is held per
// device, grow-only, so steady-state calls do no hipMalloc (graph-capturable
// once reserved).
#include <sys/random.h>
#include <time.h>

#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "engine.h"

namespace fltee {

hipError_t launch_rows_accumulate(const float *mat, size_t n, size_t d, float coef, float *out,
                                  bool accumulate, hipStream_t s);
hipError_t launch_scatter_sum(const void *rec, size_t n, size_t k, size_t d, uint32_t *mat,
                              size_t *mat_clean,
                              uint32_t *dup, float coef, float *out, bool accumulate,
                              uint32_t *status, hipStream_t s);

// Sparse non_oblivious: scatter into per-client rows (k_accumulate.hip) when the
// [n][d] row matrix costs less HBM traffic than the stable sort it replaces
// (rows: ~8*n*d bytes; sort: >= 16*M bytes per pass), or when the rows are small enough
// (<= 2^24 cells, 128 MB of traffic: ~25 us) that the counting sort's nine launches and
// its count readback cost more than they move (round 5: MLP-MNIST n = 3, k = 508 took
// ~100 us through the sort, `profiles/r05/small_ecall/`).
static bool use_scatter_rows(size_t n, size_t k, size_t d) {
    const size_t cells = n * d;
    return cells <= ((size_t)1 << 30) &&
           (cells <= ((size_t)1 << 24) || cells <= 64 * next_pow2_sz(n * k));
}

// Sparse baseline / path_oram (the sweep otherwise): uploads of dense size (k = d, e.g.
// fl_main.py --alpha 1.0, whose top-k orders each client's records by |val|, utils.py:
// 346-352), where the sweep's n*k*d compare-selects (n*d^2) would dominate, go through the
// ordered fold in the composite-key network's order (idx, upload position): the
// enclave's o_update result for any upload, bit for bit (baseline.rs:28-60 adds each
// index's records in upload order).  A public-size decision.
static bool flat_ordered(size_t n, size_t k, size_t d) { return k == d && n * k > 0; }

// the engine's scratch buffers in Ws order
static Buffer DeviceCtx::*const kScratch[kWsCount] = {
    &DeviceCtx::ws_a,    &DeviceCtx::ws_b,    &DeviceCtx::ws_mat,   &DeviceCtx::ws_r,    &DeviceCtx::ws_coef,
    &DeviceCtx::ws_rec,  &DeviceCtx::ws_keys, &DeviceCtx::ws_radix, &DeviceCtx::ws_oram, &DeviceCtx::ws_side,
    &DeviceCtx::ws_lb,   &DeviceCtx::ws_s16,  &DeviceCtx::ws_cnt,   &DeviceCtx::ws_sel};
static std::atomic<uint32_t> g_scratch_grown{0};  // fltee_debug_scratch_grown

static DeviceCtx g_ctx[kMaxDevices];
static std::mutex g_ctx_mu;
static std::atomic<uint64_t> g_debug_seed{0};
static std::atomic<uint64_t> g_seed_calls{0};

static std::atomic<uint64_t> g_net_launches{0}, g_net_bytes{0};
struct NetLaunch {
    const char *kernel;  // nullptr: the final event
    uint64_t bytes;
    hipEvent_t ev;
};
static std::mutex g_net_mu;
static std::vector<NetLaunch> g_net_log;
static std::atomic<bool> g_net_timing{false};
constexpr size_t kNetLogCap = 16384;

// the launch trace (common.h): one text line per launch / copy / memset / sync / RCCL op
static std::atomic<bool> g_trace{false};
static std::mutex g_trace_mu;
static std::string g_trace_text;
static size_t g_trace_lines = 0;
constexpr size_t kTraceCap = (size_t)64 << 20;

bool trace_on() { return g_trace.load(std::memory_order_relaxed); }

void trace_event(const char *what, const char *site, uint64_t a, uint64_t b, uint64_t c) {
    char line[512];
    const int len = std::snprintf(line, sizeof line, "%s|%s|%llu|%llu|%llu\n", what, site,
                                  (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
    std::lock_guard<std::mutex> lk(g_trace_mu);
    if (len > 0 && g_trace_text.size() + (size_t)len < kTraceCap) {
        g_trace_text.append(line, (size_t)len < sizeof line ? (size_t)len : sizeof line - 1);
        ++g_trace_lines;
    }
}

void net_account(uint64_t bytes, const char *kernel, hipStream_t s) {
    if (trace_on()) trace_event("bytes", kernel, bytes, 0, 0);
    g_net_launches.fetch_add(1, std::memory_order_relaxed);
    g_net_bytes.fetch_add(bytes, std::memory_order_relaxed);
    if (!g_net_timing.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lk(g_net_mu);
    if (g_net_log.size() >= kNetLogCap) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return;
    if (hipEventRecord(e, s) != hipSuccess) { (void)hipEventDestroy(e); return; }
    g_net_log.push_back({kernel, bytes, e});
}

static void net_log_clear() {
    for (auto &r : g_net_log) (void)hipEventDestroy(r.ev);
    g_net_log.clear();
}

uint64_t next_seed() {
    const uint64_t s = g_debug_seed.load();
    if (s) return s + 0x9E3779B97F4A7C15ull * (++g_seed_calls);
    uint64_t r = 0;
    if (getrandom(&r, sizeof r, 0) != (ssize_t)sizeof r) r = (uint64_t)time(nullptr) * 0x2545F4914F6CDD1Dull;
    return r ? r : 1;
}

void set_debug_seed(uint64_t seed) {
    g_debug_seed.store(seed);
    g_seed_calls.store(0);
}

DeviceCtx *device_ctx(int dev) {
    if (dev < 0 || dev >= kMaxDevices) return nullptr;
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    DeviceCtx &c = g_ctx[dev];
    if (!c.ready) {
        if (hipSetDevice(dev) != hipSuccess) return nullptr;
        if (hipMalloc(&c.status, 256) != hipSuccess) return nullptr;
        if (fl_memset(c.status, 0, 256) != hipSuccess) return nullptr;
        c.device = dev;
        for (int w = 0; w < kWsCount; ++w) (c.*kScratch[w]).grow_bit = 1u << w;
        c.ready = true;
    }
    return &c;
}

DeviceCtx *current_ctx() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    return device_ctx(dev);
}

bool Buffer::reserve(size_t bytes) {
    if (bytes <= cap) return true;
    g_scratch_grown.fetch_or(grow_bit, std::memory_order_relaxed);
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    const size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&ptr, want) != hipSuccess) { ptr = nullptr; return false; }
    cap = want;
    return true;
}

bool HostBuffer::reserve(size_t bytes) {
    if (bytes <= cap) return true;
    if (ptr) (void)hipHostFree(ptr);
    ptr = dptr = nullptr;
    cap = 0;
    const size_t want = bytes + bytes / 8 + 4096;
    if (hipHostMalloc(&ptr, want, hipHostMallocDefault) != hipSuccess) { ptr = nullptr; return false; }
    if (hipHostGetDevicePointer(&dptr, ptr, 0) != hipSuccess) dptr = ptr;  // one address space
    cap = want;
    return true;
}

void Buffer::release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
}

float nips19_threshold(size_t d, size_t k, size_t n) {
    const float epsilon = 100.0f, delta = 1.0f / (float)n;
    const float l1 = 2.0f * (float)k;
    return l1 / epsilon * logf((float)d / delta);
}

static size_t f32_to_usize_sat(float x) {
    if (!(x > 0.0f)) return 0;
    if (x >= 18446744073709551616.0f) return SIZE_MAX;
    return (size_t)x;
}

// runtime A/B toggles the plan reads (the fused fold's own, fltee_debug_set_fold_compact,
// is read through fc_lookback_bytes)
static bool g_radix_order = true;          // fltee_debug_set_radix_order
static bool g_advanced_compaction = true;  // fltee_debug_set_advanced_compaction
static bool g_nips19_fused_select = true;  // fltee_debug_set_nips19_fused_select
void set_radix_order(int on) { g_radix_order = on != 0; }

// the positions advanced's separate fold covers in front of the compaction, which
// reads [0, L) only: up to the first pad (position L is read as the run-end test of
// L - 1), not the pads after it
static size_t advanced_fold_span(size_t L, size_t M) {
    const size_t mf = (L + 1 + 15) / 16 * 16;
    return mf > M ? M : mf;
}

// the ordered fold's sort scratch for n records: the counting sort's, or the composite-key
// network's keys (network_order, or fltee_debug_set_radix_order(0))
static size_t ordered_radix_bytes(size_t n, size_t d, bool network_order) {
    return g_radix_order && !network_order ? radix_scratch_bytes(n, d) : next_pow2_sz(n) * 8;
}

static AdvShape adv_shape(size_t n, size_t k, size_t d, size_t k_req, size_t halo) {
    AdvShape a;
    a.nrec = n * k, a.d = d, a.L = n * k + d, a.M = next_pow2_sz(a.L);
    a.fold_len = n * k_req + d, a.halo = halo ? halo : n, a.span = a.M;
    // Second sort (advanced.rs:106-111): with fold_len == L its [0, d) prefix is the
    // order-preserving compaction of the idx < d representatives (k_compact.hip), and
    // the fold runs inside the compaction's first pass where fc_shape takes it; the
    // k_req != k quirk leaves unfolded records competing for that prefix and keeps the
    // full network.
    if (a.fold_len != a.L || !g_advanced_compaction) {
        a.tail = kTailSort;
    } else if ((a.lb_bytes = fc_lookback_bytes(a.M, a.L, d, a.halo)) != 0) {
        a.tail = kTailFused;
    } else {
        a.span = advanced_fold_span(a.L, a.M);
        a.tail = a.span >= 2 ? kTailStream : kTailOneEntry;
    }
    if (a.tail != kTailFused) a.side_bytes = fold_side_bytes(a.span, a.fold_len, a.halo, 0, 0);
    return a;
}

static void plan_adv_bytes(Plan &p, const AdvShape &a) {
    auto up = [&p](Ws w, size_t b) { if (b > p.bytes[w]) p.bytes[w] = b; };
    up(kWsA, a.M * 8), up(kWsB, a.M * 8), up(kWsSide, a.side_bytes), up(kWsLb, a.lb_bytes);
    if (a.stable) up(kWsS16, a.M * 16);
}

// the value-row format a call's flags name (rows.h); two of the flags together: the plan refuses
static RowFmt row_format(uint32_t flags) {
    return (flags & FLTEE_OPT_PACKED) ? kRowsF32
           : (flags & FLTEE_OPT_BF16) ? kRowsBf16
           : (flags & FLTEE_OPT_FP8)  ? kRowsFp8
                                      : kRowsNone;
}
static bool one_row_flag(uint32_t flags) {
    const uint32_t f = flags & (FLTEE_OPT_PACKED | FLTEE_OPT_BF16 | FLTEE_OPT_FP8);
    return (f & (f - 1)) == 0;
}

static Plan plan_for(uint32_t alg, size_t n, size_t k, size_t d, const EngineOpts &o) {
    Plan p;
    // a value-row upload is a dense one: n rows of values, k == d >= rows_min_d (f32: 2, bf16: 3,
    // fp8: 13)
    const RowFmt fmt = row_format(o.flags);
    const bool packed = fmt == kRowsF32, bf16 = fmt == kRowsBf16, fp8 = fmt == kRowsFp8;
    const bool dense = fmt != kRowsNone || (o.flags & FLTEE_OPT_DENSE) != 0;
    const bool tree = alg == FLTEE_ALG_PATH_ORAM && (o.flags & FLTEE_OPT_ORAM_TREE);
    // the trimmed mean (FLTEE_OPT_TRIM, k_trim.hip): a dense or packed call on the flat algs
    // without the tree, 2 t < n, t <= FLTEE_TRIM_MAX; t = 0 is the untrimmed route itself.
    // With FLTEE_OPT_TRIM_SELECT (k_trim_select.hip) any t with 2 t < n, n <= FLTEE_TRIM_SELECT_MAX_N:
    // the same refusals, the same scratch (none of its own)
    const bool trim = (o.flags & FLTEE_OPT_TRIM) != 0, select = (o.flags & FLTEE_OPT_TRIM_SELECT) != 0;
    const size_t nrec = n * k, k_req = (o.flags & FLTEE_OPT_K_REQ) ? o.k_req : k;
    auto refuse_if = [&p](bool bad) { if (bad) p.status = FLTEE_ERROR_INVALID_PARAMETER; };
    // 32-bit positions; a dense upload has one record per parameter
    refuse_if(n == 0 || nrec + d >= ((size_t)1 << 31) || (dense && k != d) ||
              (fmt != kRowsNone && d < rows_min_d(fmt)) ||
              !one_row_flag(o.flags));
    if (trim) {
        const bool flat = alg == FLTEE_ALG_BASELINE || alg == FLTEE_ALG_NON_OBLIVIOUS || alg == FLTEE_ALG_PATH_ORAM;
        refuse_if(!flat || !dense || (o.flags & (FLTEE_OPT_ORAM_TREE | FLTEE_OPT_ORAM_LAZY)) ||
                  (select ? n > FLTEE_TRIM_SELECT_MAX_N || o.trim >= n : o.trim > FLTEE_TRIM_MAX) ||
                  2 * o.trim >= n);  // (o.trim >= n: 2 t may wrap)
    }
    refuse_if(select && !trim);
    // Multi-Krum (FLTEE_OPT_KRUM, k_krum.hip): a dense call on the flat algs without the tree,
    // n >= 2 f + 3, 1 <= m <= n - f, n <= FLTEE_KRUM_MAX_N; never together with the trim
    const bool krum = (o.flags & FLTEE_OPT_KRUM) != 0;
    if (krum) {
        const bool flat = alg == FLTEE_ALG_BASELINE || alg == FLTEE_ALG_NON_OBLIVIOUS || alg == FLTEE_ALG_PATH_ORAM;
        refuse_if(!flat || !dense || trim || (o.flags & (FLTEE_OPT_ORAM_TREE | FLTEE_OPT_ORAM_LAZY)) ||
                  n > FLTEE_KRUM_MAX_N || o.krum_f > n || n < 2 * o.krum_f + 3 ||  // (f > n: 2 f may wrap)
                  o.krum_m == 0 || o.krum_m > n - o.krum_f);
    }
    // the geometric median (FLTEE_OPT_GMED, k_gmed.hip): a dense call on the flat algs without the
    // tree, n <= FLTEE_KRUM_MAX_N, 1 <= R <= FLTEE_GMED_MAX_ITERS, nu finite and above 0; never
    // together with the trim, Multi-Krum or NO_AVERAGE (a weighted mean has no partial-sum form)
    const bool gmed = (o.flags & FLTEE_OPT_GMED) != 0;
    if (gmed) {
        const bool flat = alg == FLTEE_ALG_BASELINE || alg == FLTEE_ALG_NON_OBLIVIOUS || alg == FLTEE_ALG_PATH_ORAM;
        refuse_if(!flat || !dense || trim || krum || (o.flags & FLTEE_OPT_NO_AVERAGE) ||
                  (o.flags & (FLTEE_OPT_ORAM_TREE | FLTEE_OPT_ORAM_LAZY)) || n > FLTEE_KRUM_MAX_N ||
                  o.gmed_iters == 0 || o.gmed_iters > FLTEE_GMED_MAX_ITERS ||
                  !(o.gmed_nu > 0.0) || !(o.gmed_nu < __builtin_inf()));  // (a NaN fails both compares)
    }
    switch (alg) {
    case FLTEE_ALG_PATH_ORAM:
    case FLTEE_ALG_BASELINE:
    case FLTEE_ALG_NON_OBLIVIOUS:
        if (tree) {
            // a shape outside oram_fits is refused (the ECALL gates the tree on the same
            // predicate and takes the sweep instead)
            const bool lazy = (o.flags & FLTEE_OPT_ORAM_LAZY) != 0;
            p.route = lazy ? kRouteTreeLazy : kRouteTree;
            refuse_if(!oram_fits(nrec, d, lazy));
            p.tree_slots = oram_slots(d);
            p.bytes[kWsOram] = p.tree_slots * (lazy ? 24 : 16);  // slots, lazy: their records too
            // the leaf precompute's two key arrays
            p.bytes[kWsA] = p.bytes[kWsB] = next_pow2_sz(oram_accesses(nrec, d, lazy)) * 8;
            // lazy readout: every slot's (idx, value) through advanced's network (one
            // "client" of `slots` records: each index at most once, runs of <= 2 entries)
            if (lazy) plan_adv_bytes(p, p.adv = adv_shape(1, p.tree_slots, d, p.tree_slots, 1));
        } else if (dense) {
            p.route = packed ? kRoutePacked : bf16 ? kRouteBf16 : fp8 ? kRouteFp8 : kRouteDense;
            // (a trimmed bf16 or fp8 call: the records trim on the unpacked copy)
            if (trim && o.trim)
                p.route = select ? (packed ? kRouteTrimSelectPacked : kRouteTrimSelectDense)
                                 : (packed ? kRouteTrimPacked : kRouteTrimDense);
            // (a bf16 or fp8 Krum call: the records route on the unpacked copy, as for the trim)
            if (krum) {
                p.route = packed ? kRouteKrumPacked : kRouteKrumDense;
                // the Gram partials, G, the scores and the keep words: a slot no dense route touches
                p.bytes[kWsMat] = n <= FLTEE_KRUM_MAX_N ? krum_scratch_bytes(n, d) : 0;
            }
            if (gmed) {
                p.route = packed ? kRouteGmedPacked : kRouteGmedDense;
                // Krum's partials and G, then w, u, rho, alpha and valid: from (n, d) alone
                p.bytes[kWsMat] = n && n <= FLTEE_KRUM_MAX_N ? gmed_scratch_bytes(n, d) : 0;  // (refused otherwise)
            }
        } else if (alg == FLTEE_ALG_NON_OBLIVIOUS && use_scatter_rows(n, k, d)) {
            p.route = kRouteScatterRows;
            p.bytes[kWsMat] = n * d * 4;
        } else if (alg == FLTEE_ALG_NON_OBLIVIOUS || flat_ordered(n, k, d)) {
            const bool net = alg != FLTEE_ALG_NON_OBLIVIOUS;
            p.route = net ? kRouteFlatOrdered : kRouteCountingFold;
            refuse_if(next_pow2_sz(nrec) > kMaxNetRecords);
            p.bytes[kWsKeys] = nrec * 8, p.bytes[kWsRadix] = ordered_radix_bytes(nrec, d, net);
        } else {
            p.route = kRouteSweep;
        }
        break;
    case FLTEE_ALG_BUBBLE:
        // bubble_sort_based.rs:42 folds n * k_req + d entries; only k_req == k is answered
        p.route = kRouteBubble;
        p.adv = adv_shape(n, k, d, k, o.fold_halo);
        p.adv.stable = true;
        refuse_if(k_req != k || p.adv.M > kMaxNetRecords || p.adv.M > stable_sort_max_records());
        plan_adv_bytes(p, p.adv);
        break;
    case FLTEE_ALG_ADVANCED:
        p.route = kRouteAdvanced;
        p.adv = adv_shape(n, k, d, k_req, o.fold_halo);
        refuse_if(p.adv.M > kMaxNetRecords || p.adv.fold_len > p.adv.L);  // advanced.rs:72 panic
        plan_adv_bytes(p, p.adv);
        break;
    case FLTEE_ALG_OPTIMIZED:
        p.route = kRouteOptimized;
        p.batch = o.batch && o.batch < n ? o.batch : n;
        p.adv = adv_shape(p.batch, k, d, k, o.fold_halo);
        refuse_if(p.adv.M > kMaxNetRecords);
        plan_adv_bytes(p, p.adv);
        if (p.batch && n % p.batch)
            plan_adv_bytes(p, p.adv_last = adv_shape(n % p.batch, k, d, k, o.fold_halo));
        break;
    case FLTEE_ALG_NIPS19:
        p.route = kRouteNips19;
        p.kq = k_req;
        p.T = nips19_threshold(d, p.kq, n);
        p.tf = f32_to_usize_sat(p.T);
        p.bytes[kWsR] = d * 4;
        refuse_if(p.tf > ((size_t)1 << 31) / (d ? d : 1));
        if (p.status != FLTEE_SUCCESS) break;  // (d * tf would overflow)
        p.L = nrec + d * p.tf, p.M = next_pow2_sz(p.L);
        refuse_if(p.M > kMaxNetRecords);
        p.bytes[kWsA] = p.M * 8;
        // the tile counts: the shuffle's selecting last pass, or (where that launcher
        // declines) safe_aggregate's own tiles
        p.sel_tiles = g_nips19_fused_select && d ? bitonic_select_tiles(p.M) : 0;
        p.bytes[kWsCnt] = (2 * (p.sel_tiles > select_tiles(p.M) ? p.sel_tiles : select_tiles(p.M)) + 2) * 4;
        break;
    default:
        refuse_if(true);  // lib.rs:396 panics on unknown algs
        break;
    }
    if (o.flags & FLTEE_OPT_CLIP) {
        // every route but the dense accumulate (which takes the coefficients) reads records:
        // FLTEE_OPT_DENSE on algs 1, 2, 6, 7 and on the tree only asserts k == d
        p.bytes[kWsCoef] = n * 4;
        p.clip_records = p.route != kRouteDense && p.route != kRoutePacked && p.route != kRouteTrimDense &&
                         p.route != kRouteTrimPacked && p.route != kRouteBf16 && p.route != kRouteFp8 &&
                         p.route != kRouteTrimSelectDense && p.route != kRouteTrimSelectPacked &&
                         p.route != kRouteKrumDense && p.route != kRouteKrumPacked &&
                         p.route != kRouteGmedDense && p.route != kRouteGmedPacked;
        if (p.clip_records) p.bytes[kWsRec] = nrec * 8;
    }
    // every route but the packed / bf16 / fp8 accumulate reads records: the plan (n, d, d) has, on the
    // rows unpacked into the record scratch (where FLTEE_OPT_CLIP then clips them in place)
    p.unpack = fmt != kRowsNone && p.route != kRoutePacked && p.route != kRouteTrimPacked && p.route != kRouteBf16 &&
               p.route != kRouteTrimSelectPacked && p.route != kRouteFp8 && p.route != kRouteKrumPacked &&
               p.route != kRouteGmedPacked;
    if (p.unpack) p.bytes[kWsRec] = nrec * 8;
    return p;
}

// The fused fold's look-back slots, ready for one more launch.  A slot must never carry a
// live epoch it was not given: new slots hold whatever was there, and at epoch 2^30 - 1 the
// counter would wrap into epochs old slots still hold — either way the slots are zeroed and
// the epochs start over.  s: the stream the launch follows on (in front of every fused
// launch: the slots of launches before it on that stream may still be read); none
// (fltee_reserve): grow only, zeroed on the host's time.
static bool reserve_lb(DeviceCtx *c, size_t bytes, const hipStream_t *s) {
    const bool grow = bytes > c->ws_lb.cap;
    if (!bytes || (!grow && (!s || c->fc_epoch < (1u << 30) - 1))) return true;
    if (!c->ws_lb.reserve(bytes)) return false;
    if ((s ? fl_memset_async(c->ws_lb.ptr, 0, c->ws_lb.cap, *s) : fl_memset(c->ws_lb.ptr, 0, c->ws_lb.cap)) !=
        hipSuccess)
        return false;
    c->fc_epoch = 0;
    return true;
}

static bool reserve_plan(DeviceCtx *c, const Plan &p, const hipStream_t *s) {
    for (int w = 0; w < kWsCount; ++w)
        if (!(w == kWsLb ? reserve_lb(c, p.bytes[w], s) : (c->*kScratch[w]).reserve(p.bytes[w]))) return false;
    return true;
}

static bool g_exact_runs = false;  // the ECALLs' advanced / alg 6: reject runs > n + 1 unless set
void set_exact_runs(int on) { g_exact_runs = on != 0; }
bool exact_runs_default() { return g_exact_runs; }
static bool g_bubble_ecall = false;  // ecall_secure_aggregation answers alg 7 only when set
void set_bubble_ecall(int on) { g_bubble_ecall = on != 0; }
bool bubble_ecall_default() { return g_bubble_ecall; }
static bool g_oram_tree = false;  // the ECALLs' path_oram: the sweep unless set
void set_oram_tree(int on) { g_oram_tree = on != 0; }
bool oram_tree_default() { return g_oram_tree; }

// The ordered fold of n records (common.rs:25-35, non_oblivious.rs:11-13): the records in
// stable order by idx, then out[i] = the in-order sum of index i's.  The order comes from
// the hand-written counting sort (k_radix.hip: the sequence of indices in list order is
// what the enclave's own g[idx] += val loop touches) — or, fltee_debug_set_radix_order(0),
// from the composite-key bitonic sort, the records gathered by its keys (the same order,
// bit for bit: test_gpu_parity.py).
// ws_keys (n * 8) and ws_radix (ordered_radix_bytes) are the caller's: the plan's, or
// ordered_from_list's.
static hipError_t ordered_fold_records(DeviceCtx *c, const void *rec, size_t n, size_t d,
                                       float coef, float *out, bool acc, uint32_t *status,
                                       hipStream_t s, bool network_order = false) {
    if (n == 0) return acc ? hipSuccess : fl_memset_async(out, 0, d * 4, s);
    uint64_t *sorted = (uint64_t *)c->ws_keys.ptr;
    hipError_t e;
    if (g_radix_order && !network_order) {
        e = launch_sort_records_by_idx(rec, n, d, c->ws_radix.ptr, c->ws_radix.cap, sorted, status,
                                       acc ? nullptr : out, d, s);
    } else {
        const size_t mc = next_pow2_sz(n);
        uint64_t *keys = (uint64_t *)c->ws_radix.ptr;
        e = launch_composite_init(rec, n, d, mc, keys, status, s);
        if (e == hipSuccess) e = bitonic_sort(keys, mc, 1, 0, s, n);  // ~0 keys past n
        if (e == hipSuccess) e = launch_gather_by_keys(keys, n, rec, sorted, s);
        if (e == hipSuccess && !acc) e = fl_memset_async(out, 0, d * 4, s);
    }
    if (e == hipSuccess) e = launch_fold_sorted(sorted, n, d, coef, out, acc, s);
    return e;
}

// the selected list sel[0, lc) (entries with idx < d in position order) -> out: stable
// order by idx (list position within an index), then the ordered fold.  lc was read back
// from the device: the one scratch sized here, outside the plan.
hipError_t ordered_from_list(DeviceCtx *c, const uint64_t *sel, size_t lc, size_t d, float coef,
                             float *out, bool acc, uint32_t *status, hipStream_t s) {
    if (lc && (!c->ws_keys.reserve(lc * 8) || !c->ws_radix.reserve(ordered_radix_bytes(lc, d, false))))
        return hipErrorOutOfMemory;
    return ordered_fold_records(c, sel, lc, d, coef, out, acc, status, s);
}

// fltee_debug_sort_records_device: the ordered fold's sort alone, on scratch reserved as
// ordered_from_list reserves it — the counting sort, no output to zero-fill; or,
// fltee_debug_set_radix_order(0), the composite-key network's order — then the n sorted
// records copied out of ws_keys.
static hipError_t debug_sort_records(DeviceCtx *c, const void *rec, size_t n, size_t d, void *dst,
                                     uint32_t *status, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!c->ws_keys.reserve(n * 8) || !c->ws_radix.reserve(ordered_radix_bytes(n, d, false)))
        return hipErrorOutOfMemory;
    uint64_t *sorted = (uint64_t *)c->ws_keys.ptr;
    hipError_t e;
    if (g_radix_order) {
        e = launch_sort_records_by_idx(rec, n, d, c->ws_radix.ptr, c->ws_radix.cap, sorted, status,
                                       nullptr, 0, s);
    } else {
        const size_t mc = next_pow2_sz(n);
        uint64_t *keys = (uint64_t *)c->ws_radix.ptr;
        e = launch_composite_init(rec, n, d, mc, keys, status, s);
        if (e == hipSuccess) e = bitonic_sort(keys, mc, 1, 0, s, n);
        if (e == hipSuccess) e = launch_gather_by_keys(keys, n, rec, sorted, s);
    }
    if (e == hipSuccess) e = fl_memcpy_async(dst, sorted, n * 8, hipMemcpyDeviceToDevice, s);
    return e;
}

hipError_t read_device_word(DeviceCtx *c, const uint32_t *dev_word, size_t *out, hipStream_t s) {
    if (!c->host_word && hipHostMalloc((void **)&c->host_word, 64, hipHostMallocDefault) != hipSuccess) {
        c->host_word = nullptr;
        return hipErrorOutOfMemory;
    }
    hipError_t e = fl_memcpy_async(c->host_word, dev_word, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = fl_stream_sync(s);
    if (e == hipSuccess) *out = *c->host_word;
    return e;
}

hipError_t safe_aggregate_ordered(DeviceCtx *c, const uint64_t *src, size_t m, size_t d,
                                  float coef, float *out, bool acc, uint32_t *status,
                                  hipStream_t s) {
    if (d == 0) return hipSuccess;
    if (m == 0) return acc ? hipSuccess : fl_memset_async(out, 0, d * 4, s);
    const size_t nb = select_tiles(m);
    if (!c->ws_cnt.reserve((2 * nb + 2) * 4)) return hipErrorOutOfMemory;
    uint32_t *cnt = (uint32_t *)c->ws_cnt.ptr, *base = cnt + nb + 1;
    hipError_t e = launch_select_count(src, m, d, cnt, base, s);
    size_t lc = 0;  // entries with idx < d (the DP-noised histogram total)
    if (e == hipSuccess) e = read_device_word(c, base + nb, &lc, s);
    if (e != hipSuccess) return e;
    if (!c->ws_sel.reserve(lc * 8 + 8)) return hipErrorOutOfMemory;
    uint64_t *sel = (uint64_t *)c->ws_sel.ptr;
    if (lc) e = launch_select_write(src, m, d, base, sel, s);
    if (e != hipSuccess) return e;
    return ordered_from_list(c, sel, lc, d, coef, out, acc, status, s);
}

// nips19's shuffle + safe_aggregate with the selection fused into the shuffle's last
// pass (bitonic_sort_nips19_select, over the plan's sel_tiles tiles): the 2^27-entry array
// is never written out or read back.  hipErrorNotSupported: the launcher declined (the
// caller shuffles, then selects).
static hipError_t nips19_shuffle_aggregate(DeviceCtx *c, const Plan &p, uint32_t key, const void *rec,
                                           size_t nrec, size_t d, float coef, float *out, bool acc,
                                           uint32_t *status, hipStream_t s) {
    const size_t ntl = p.sel_tiles;
    uint64_t *A = (uint64_t *)c->ws_a.ptr;
    uint32_t *cnt = (uint32_t *)c->ws_cnt.ptr, *base = cnt + ntl + 1;
    // tiles of pads alone are skipped by the last pass and keep a zero count
    hipError_t e = fl_memset_async(cnt, 0, ntl * 4, s);
    if (e == hipSuccess)
        e = bitonic_sort_nips19_select(A, p.M, key, rec, nrec, (const uint32_t *)c->ws_r.ptr, d, p.tf, cnt, s);
    if (e != hipSuccess) return e;
    e = launch_select_scan(cnt, ntl, base, s);
    size_t lc = 0;
    if (e == hipSuccess) e = read_device_word(c, base + ntl, &lc, s);
    if (e != hipSuccess) return e;
    if (!c->ws_sel.reserve(lc * 8 + 8)) return hipErrorOutOfMemory;
    uint64_t *sel = (uint64_t *)c->ws_sel.ptr;
    if (lc) e = launch_select_gather(A, log2_pow2(p.M / ntl), ntl, cnt, base, sel, s);
    if (e != hipSuccess) return e;
    return ordered_from_list(c, sel, lc, d, coef, out, acc, status, s);
}

// `advanced` over the planned shape's records into out (coef or accumulate), on scratch the
// plan reserved.  a.stable (alg 7): the array is sorted by (idx, upload position) through
// the stable network (k_stable.hip) instead of advanced's first sort; the tail is shared.
static hipError_t run_advanced(DeviceCtx *c, const void *rec, const AdvShape &a, float coef, float *out,
                               bool acc, uint32_t *status, hipStream_t s) {
    uint64_t *A = (uint64_t *)c->ws_a.ptr, *B = (uint64_t *)c->ws_b.ptr;
    hipError_t e;
    if (a.stable) {  // init fused into the first pass, strip into the last
        e = stable_sort(c->ws_s16.ptr, a.M, s, a.L, true, rec, a.nrec, a.d, A);
    } else {
        e = bitonic_sort_advanced(A, a.M, rec, a.nrec, a.d, s);  // init fused into the sort
        if (e == hipErrorNotSupported) {
            e = launch_advanced_init(rec, a.nrec, a.d, a.M, A, s);
            if (e == hipSuccess) e = bitonic_sort(A, a.M, 0, 0, s, a.L);
        }
    }
    if (e != hipSuccess) return e;
    switch (a.tail) {
    case kTailFused:
        if (!reserve_lb(c, a.lb_bytes, &s)) return hipErrorOutOfMemory;  // (the epoch wrap: no growth here)
        return launch_fold_compact_extract(A, B, a.M, a.L, a.d, a.halo, coef, out, acc, status, s,
                                           c->ws_lb.ptr, c->ws_lb.cap, &c->fc_epoch);
    case kTailStream:  // the fold emits the compaction's first-pass form (no conversion there, 16-B pairs)
        e = launch_fold(A, B, a.span, a.fold_len, a.halo, c->ws_side.ptr, c->ws_side.cap, s, a.d,
                        compact_dummy());
        if (e != hipSuccess) return e;
        return launch_compact_extract_converted(B, A, a.L, a.d, coef, out, acc, s);
    case kTailOneEntry:  // nothing to fold: copied as the enclave's folded array, converted by that pass
        e = launch_fold(A, B, a.span, a.fold_len, a.halo, c->ws_side.ptr, c->ws_side.cap, s);
        if (e != hipSuccess) return e;
        return launch_compact_extract(B, A, a.L, a.d, coef, out, acc, s);
    default:
        e = launch_fold(A, B, a.M, a.fold_len, a.halo, c->ws_side.ptr, c->ws_side.cap, s);
        if (e == hipSuccess) e = bitonic_sort(B, a.M, 0, 0, s, a.L);  // the fold copies the pads past fold_len
        if (e == hipSuccess) e = launch_extract(B, a.d, coef, out, acc, s);
        return e;
    }
}

// `advanced` of n clients' records into out[d] un-averaged (coef 1, overwrite): one
// batch sum of alg 6 (advanced.rs:10-21), on the current device's scratch
hipError_t advanced_batch(const void *rec, size_t n, size_t k, size_t d, size_t halo, float *out,
                          uint32_t *status, hipStream_t s) {
    DeviceCtx *c = current_ctx();
    if (!c) return hipErrorInvalidDevice;
    EngineOpts o;
    std::memset(&o, 0, sizeof o);
    o.fold_halo = halo;
    const Plan p = plan_for(FLTEE_ALG_ADVANCED, n, k, d, o);
    if (p.status != FLTEE_SUCCESS) return hipErrorInvalidValue;
    if (!reserve_plan(c, p, &s)) return hipErrorOutOfMemory;
    return run_advanced(c, rec, p.adv, 1.0f, out, false, status, s);
}

// plan -> the refusal -> the plan's scratch -> clip -> the route -> DP
// sel_scores / sel_keep (krum_select): a Multi-Krum call ends after its selection, the scores and
// keep words copied there; sel_alpha / sel_rho (gmed_weights): a geometric-median call after its
// weights likewise
static fltee_status_t aggregate_impl(uint32_t alg, const void *rec, size_t n, size_t k, size_t d, float *out,
                                     const EngineOpts &o, hipStream_t s, uint32_t *status,
                                     double *sel_scores, uint32_t *sel_keep, float *sel_alpha = nullptr,
                                     double *sel_rho = nullptr) {
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_UNEXPECTED;
    const Plan p = plan_for(alg, n, k, d, o);
    if (p.status != FLTEE_SUCCESS) return p.status;
    if (!reserve_plan(c, p, &s)) return FLTEE_ERROR_OUT_OF_MEMORY;
    const bool acc = (o.flags & FLTEE_OPT_ACCUMULATE) != 0;
    // (the trimmed mean averages the n - 2 t clients it keeps; the DP noise takes the same divisor)
    // (Multi-Krum averages the m clients it keeps)
    const size_t n_avg = o.n_avg                        ? o.n_avg
                         : (o.flags & FLTEE_OPT_TRIM) ? n - 2 * o.trim
                         : (o.flags & FLTEE_OPT_KRUM) ? o.krum_m
                                                      : n;
    const float coef = (o.flags & FLTEE_OPT_NO_AVERAGE) ? 1.0f : 1.0f / (float)n_avg;

    // packed / bf16 / fp8 rows off their own route: every alg below runs on the records (j, v[j])
    // (fmt: what rec holds from here on)
    const RowFmt sent = row_format(o.flags), fmt = p.unpack ? kRowsNone : sent;
    if (p.unpack) {
        if (launch_unpack_rows(sent, rec, n, d, (uint64_t *)c->ws_rec.ptr, s) != hipSuccess)
            return FLTEE_ERROR_UNEXPECTED;
        rec = c->ws_rec.ptr;
    }

    // per-client L2 clip (update.py:187-204), off by default
    const float *ccoef = nullptr;
    if (o.flags & FLTEE_OPT_CLIP) {
        float *cf = (float *)c->ws_coef.ptr;
        if ((fmt != kRowsNone ? launch_rows_clip_coef(fmt, rec, n, d, o.clipping, cf, s)
                              : launch_client_clip_coef(rec, n, k, o.clipping, cf, s)) != hipSuccess)
            return FLTEE_ERROR_UNEXPECTED;
        ccoef = cf;
        if (p.clip_records) {
            // (an unpacked copy is already the scratch: clipped where it is)
            if ((!p.unpack &&
                 fl_memcpy_async(c->ws_rec.ptr, rec, n * k * 8, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
                launch_apply_clip(c->ws_rec.ptr, n, k, cf, s) != hipSuccess)
                return FLTEE_ERROR_UNEXPECTED;
            rec = c->ws_rec.ptr;
        }
    }

    hipError_t e = hipSuccess;
    switch (p.route) {
    case kRouteTree:
    case kRouteTreeLazy: {  // the tree Path ORAM (k_oram.hip)
        const bool lazy = p.route == kRouteTreeLazy;
        uint8_t *tree = (uint8_t *)c->ws_oram.ptr;
        uint64_t *recs = lazy ? (uint64_t *)(tree + p.tree_slots * 16) : nullptr;
        const uint64_t seed = o.seed ? o.seed : next_seed();
        e = launch_check_range(rec, n * k, (uint32_t)next_pow2_sz(d), status, s);  // oram.rs panics
        if (e == hipSuccess)
            e = launch_oram_tree(rec, n * k, d, lazy, tree, seed, (uint64_t *)c->ws_a.ptr,
                                 (uint64_t *)c->ws_b.ptr, recs, coef, acc, out, status, s);
        // lazy readout: every slot's (idx, value) through advanced's oblivious network
        if (e == hipSuccess && lazy) e = run_advanced(c, recs, p.adv, coef, out, acc, status, s);
        break;
    }
    case kRouteDense:
        e = launch_dense_accumulate(rec, n, d, coef, out, ccoef, acc, status, s);
        break;
    case kRoutePacked:
    case kRouteBf16:
    case kRouteFp8:
        e = launch_dense_accumulate_rows(fmt, rec, n, d, coef, out, ccoef, acc, s);
        break;
    case kRouteTrimDense:
    case kRouteTrimPacked:
        e = launch_trimmed_mean(rec, p.route == kRouteTrimPacked, n, d, o.trim, coef, out, ccoef, acc, status, s);
        break;
    case kRouteTrimSelectDense:
    case kRouteTrimSelectPacked:
        e = launch_trim_select(rec, p.route == kRouteTrimSelectPacked, n, d, o.trim, coef, out, ccoef, acc, status,
                               s);
        break;
    case kRouteKrumDense:
    case kRouteKrumPacked: {
        const bool rows = p.route == kRouteKrumPacked;
        c->mat_clean = 0;  // (the scatter rows' sentinel, if it was there, is overwritten)
        e = launch_krum_select(rec, rows, n, d, o.krum_f, o.krum_m, ccoef, c->ws_mat.ptr, status, s);
        if (e == hipSuccess && sel_scores) {
            e = fl_memcpy_async(sel_scores, krum_scores(c->ws_mat.ptr, n, d), n * 8, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess)
                e = fl_memcpy_async(sel_keep, krum_keep(c->ws_mat.ptr, n, d), n * 4, hipMemcpyDeviceToDevice, s);
            return e == hipSuccess ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
        }
        if (e == hipSuccess)
            e = launch_krum_accumulate(rec, rows, n, d, krum_keep(c->ws_mat.ptr, n, d), coef, out, ccoef, acc, s);
        break;
    }
    case kRouteGmedDense:
    case kRouteGmedPacked: {
        const bool rows = p.route == kRouteGmedPacked;
        void *ws = c->ws_mat.ptr;
        c->mat_clean = 0;  // (the scatter rows' sentinel, if it was there, is overwritten)
        e = launch_gmed_weights(rec, rows, n, d, o.gmed_iters, o.gmed_nu, ccoef, ws, status, s);
        if (e == hipSuccess && sel_alpha) {
            e = fl_memcpy_async(sel_alpha, gmed_alpha(ws, n, d), n * 4, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = fl_memcpy_async(sel_rho, gmed_rho(ws, n, d), n * 8, hipMemcpyDeviceToDevice, s);
            return e == hipSuccess ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
        }
        // (the weights sum to one: no averaging factor; n_avg is the DP noise's divisor alone)
        if (e == hipSuccess)
            e = launch_gmed_accumulate(rec, rows, n, d, gmed_alpha(ws, n, d), gmed_valid(ws, n, d), out, ccoef, acc, s);
        break;
    }
    case kRouteScatterRows:
        if (c->mat_clean_ptr != c->ws_mat.ptr || c->mat_clean_cap != c->ws_mat.cap) {
            c->mat_clean = 0;  // a new allocation: contents unknown
            c->mat_clean_ptr = c->ws_mat.ptr;
            c->mat_clean_cap = c->ws_mat.cap;
        }
        e = launch_scatter_sum(rec, n, k, d, (uint32_t *)c->ws_mat.ptr, &c->mat_clean,
                               c->status + 16, coef, out, acc, status, s);
        if (e != hipSuccess) c->mat_clean = 0;  // the emptying pass may not have run
        break;
    case kRouteCountingFold:
        e = ordered_fold_records(c, rec, n * k, d, coef, out, acc, status, s);
        break;
    case kRouteFlatOrdered:
    case kRouteSweep:
        // baseline / path_oram on sparse uploads: the ordered sweep (exact for any
        // upload, a client may repeat an index; fixed cost n*k*d compare-selects) —
        // or, for dense-sized uploads (flat_ordered), the composite-key network's
        // ordered fold (exact for any upload too).  Records with idx >= d are ignored
        // (o_update's compare never matches): the network's range flag goes to a
        // scratch word.
        if (alg == FLTEE_ALG_PATH_ORAM)  // oram.rs: blocks beyond next_pow2(d) do not exist
            e = launch_check_range(rec, n * k, (uint32_t)next_pow2_sz(d), status, s);
        if (e == hipSuccess && p.route == kRouteFlatOrdered)
            e = ordered_fold_records(c, rec, n * k, d, coef, out, acc, c->status + 32, s, true);
        else if (e == hipSuccess)
            e = launch_sweep_accumulate(rec, n * k, d, coef, out, acc, s);
        break;
    case kRouteAdvanced:
    case kRouteBubble:  // alg 7: the stable sort, then advanced's fold / compaction / extract
        e = run_advanced(c, rec, p.adv, coef, out, acc, status, s);
        break;
    case kRouteOptimized:
        if (!acc) e = fl_memset_async(out, 0, d * 4, s);
        for (size_t c0 = 0; e == hipSuccess && c0 < n; c0 += p.batch)
            e = run_advanced(c, (const uint8_t *)rec + c0 * k * 8, c0 + p.batch <= n ? p.adv : p.adv_last,
                             1.0f, out, true, status, s);
        // accumulate: out += sum, un-averaged as on every other route (what was in out stays)
        if (e == hipSuccess && !acc && coef != 1.0f) e = launch_scale(out, d, coef, s);
        break;
    case kRouteNips19: {
        const uint64_t seed = o.seed ? o.seed : next_seed();
        uint64_t *A = (uint64_t *)c->ws_a.ptr;
        const uint32_t *r = (const uint32_t *)c->ws_r.ptr;
        e = launch_laplace_r(d, p.kq, p.T, seed, (uint32_t *)c->ws_r.ptr, s);
        const uint32_t key = (uint32_t)(seed ^ (seed >> 32));
        bool done = false;
        if (e == hipSuccess && p.sel_tiles) {  // build + shuffle + select fused
            e = nips19_shuffle_aggregate(c, p, key, rec, n * k, d, coef, out, acc, status, s);
            done = e != hipErrorNotSupported;
            if (!done) e = hipSuccess;
        }
        if (e == hipSuccess && !done) {  // build fused into the shuffle's first pass where it can be
            e = bitonic_sort_nips19(A, p.M, key, rec, n * k, r, d, p.tf, s);
            if (e == hipErrorNotSupported) {
                e = launch_nips19_build(rec, n * k, r, d, p.tf, p.M, A, s);
                if (e == hipSuccess) e = bitonic_sort(A, p.M, 2, key, s, p.L);
            }
            if (e == hipSuccess) e = safe_aggregate_ordered(c, A, p.M, d, coef, out, acc, status, s);
        }
        break;
    }
    default:
        return FLTEE_ERROR_INVALID_PARAMETER;  // (the plan refuses every shape without a route)
    }
    if (e == hipSuccess && (o.flags & FLTEE_OPT_DP)) {
        const uint64_t seed = o.seed ? o.seed : next_seed();
        e = launch_dp_noise(out, d, o.sigma, o.clipping, n_avg, seed, s);
    }
    if (e != hipSuccess)
        std::fprintf(stderr, "[fltee] aggregate(alg %u, n %zu, k %zu, d %zu): %s\n", alg, n, k, d,
                     hipGetErrorString(e));
    return e == hipSuccess ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
}

fltee_status_t aggregate(uint32_t alg, const void *rec, size_t n, size_t k, size_t d, float *out,
                         const EngineOpts &o, hipStream_t s, uint32_t *status) {
    return aggregate_impl(alg, rec, n, k, d, out, o, s, status, nullptr, nullptr);
}

fltee_status_t krum_select(const void *rec, size_t n, size_t d, const EngineOpts &o, double *sel_scores,
                           uint32_t *sel_keep, hipStream_t s, uint32_t *status) {
    if (!(o.flags & FLTEE_OPT_KRUM) || !sel_scores || !sel_keep) return FLTEE_ERROR_INVALID_PARAMETER;
    return aggregate_impl(FLTEE_ALG_BASELINE, rec, n, d, d, nullptr, o, s, status, sel_scores, sel_keep);
}

fltee_status_t gmed_weights(const void *rec, size_t n, size_t d, const EngineOpts &o, float *sel_alpha,
                            double *sel_rho, hipStream_t s, uint32_t *status) {
    if (!(o.flags & FLTEE_OPT_GMED) || !sel_alpha || !sel_rho) return FLTEE_ERROR_INVALID_PARAMETER;
    return aggregate_impl(FLTEE_ALG_BASELINE, rec, n, d, d, nullptr, o, s, status, nullptr, nullptr, sel_alpha,
                          sel_rho);
}

size_t workspace_bytes(uint32_t alg, size_t n, size_t k, size_t d, const EngineOpts &o) {
    const Plan p = plan_for(alg, n, k, d, o);
    size_t sum = 0;
    for (size_t b : p.bytes) sum += b;
    return sum;
}

fltee_status_t plan_status(uint32_t alg, size_t n, size_t k, size_t d, const EngineOpts &o) {
    return plan_for(alg, n, k, d, o).status;
}

bool reserve(uint32_t alg, size_t n, size_t k, size_t d, const EngineOpts &o) {
    DeviceCtx *c = current_ctx();
    return c && reserve_plan(c, plan_for(alg, n, k, d, o), nullptr);
}

// fltee_debug_plan: the plan as words (host only, no device needed)
fltee_status_t debug_plan_words(uint32_t alg, size_t n, size_t k, size_t d, const EngineOpts &o,
                                uint64_t *out) {
    const Plan p = plan_for(alg, n, k, d, o);
    out[0] = p.route, out[1] = p.adv.tail;
    out[2] = p.route == kRouteNips19 ? p.M : p.adv.M, out[3] = p.adv.halo;
    for (int w = 0; w < kWsCount; ++w) out[4 + w] = p.bytes[w];
    return p.status;
}

// fltee_debug_scratch_release: the current device's engine scratch freed, what described
// its contents forgotten (the caller holds the API mutex)
void release_scratch() {
    DeviceCtx *c = current_ctx();
    if (!c) return;
    for (auto w : kScratch) (c->*w).release();
    c->mat_clean = c->mat_clean_cap = 0;
    c->mat_clean_ptr = nullptr;
    c->fc_epoch = 0;
}


}  // namespace fltee

// ============================================================ C ABI =========
using namespace fltee;

static EngineOpts default_opts() {
    EngineOpts o;
    std::memset(&o, 0, sizeof o);
    return o;
}

// The caller's options.  The struct is copied up to `trim`; each field from there on is read
// only under its own flag (trim: FLTEE_OPT_TRIM; krum_f, krum_m, which lie behind the struct in a
// fltee_device_opts_krum: FLTEE_OPT_KRUM; gmed_iters, gmed_nu, behind it in a
// fltee_device_opts_gmed: FLTEE_OPT_GMED): a caller built against a struct that ended earlier
// never sets the flag, and nothing past its struct is touched.
static EngineOpts read_opts(const fltee_device_opts *opts) {
    EngineOpts o = default_opts();
    if (!opts) return o;
    std::memcpy(static_cast<fltee_device_opts *>(&o), opts, offsetof(fltee_device_opts, trim));
    if (o.flags & FLTEE_OPT_TRIM) o.trim = opts->trim;
    if (o.flags & FLTEE_OPT_KRUM) {
        const fltee_device_opts_krum *k = reinterpret_cast<const fltee_device_opts_krum *>(opts);
        o.krum_f = k->krum_f, o.krum_m = k->krum_m;
    }
    if (o.flags & FLTEE_OPT_GMED) {
        const fltee_device_opts_gmed *g = reinterpret_cast<const fltee_device_opts_gmed *>(opts);
        o.gmed_iters = g->gmed_iters, o.gmed_nu = g->gmed_nu;
    }
    return o;
}

extern "C" fltee_status_t fltee_aggregate_device(uint32_t alg, const void *d_records, size_t n,
                                                 size_t k, size_t d, float *d_out,
                                                 const fltee_device_opts *opts, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    const EngineOpts o = read_opts(opts);
    // (bf16 rows are read as 2-byte halves: an odd base is refused by host arithmetic)
    if ((o.flags & FLTEE_OPT_BF16) && ((uintptr_t)d_records & 1)) return FLTEE_ERROR_INVALID_PARAMETER;
    // (fp8 rows carry an f32 scale, read as one: a base that is not 4-byte aligned likewise)
    if ((o.flags & FLTEE_OPT_FP8) && ((uintptr_t)d_records & 3)) return FLTEE_ERROR_INVALID_PARAMETER;
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_UNEXPECTED;
    uint32_t *status = o.d_status ? o.d_status : c->status;
    hipStream_t s = (hipStream_t)stream;
    if (!o.d_status && fl_memset_async(c->status, 0, 4, s) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    return aggregate(alg, d_records, n, k, d, d_out, o, s, status);
}

extern "C" fltee_status_t fltee_krum_select_device(const void *d_records, size_t n, size_t d,
                                                   const fltee_device_opts *opts, double *d_scores,
                                                   uint32_t *d_keep, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    // (the flag is the caller's word that opts is the base of a fltee_device_opts_krum)
    if (!opts || !(opts->flags & FLTEE_OPT_KRUM) || !d_scores || !d_keep) return FLTEE_ERROR_INVALID_PARAMETER;
    // steps 1 - 4 take the layout, the clip and (f, m) from the options and nothing else
    const EngineOpts in = read_opts(opts);
    EngineOpts o = default_opts();
    o.flags = (in.flags & (FLTEE_OPT_PACKED | FLTEE_OPT_BF16 | FLTEE_OPT_FP8 | FLTEE_OPT_CLIP)) | FLTEE_OPT_DENSE |
              FLTEE_OPT_KRUM;
    o.clipping = in.clipping, o.d_status = in.d_status;
    o.krum_f = in.krum_f, o.krum_m = in.krum_m;
    if ((o.flags & FLTEE_OPT_BF16) && ((uintptr_t)d_records & 1)) return FLTEE_ERROR_INVALID_PARAMETER;
    if ((o.flags & FLTEE_OPT_FP8) && ((uintptr_t)d_records & 3)) return FLTEE_ERROR_INVALID_PARAMETER;
    if (plan_status(FLTEE_ALG_BASELINE, n, d, d, o) != FLTEE_SUCCESS) return FLTEE_ERROR_INVALID_PARAMETER;
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_UNEXPECTED;
    uint32_t *status = o.d_status ? o.d_status : c->status;
    hipStream_t s = (hipStream_t)stream;
    if (!o.d_status && fl_memset_async(c->status, 0, 4, s) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    return krum_select(d_records, n, d, o, d_scores, d_keep, s, status);
}

extern "C" fltee_status_t fltee_krum_gram_ranges_device(const void *d_in, int packed, size_t n, size_t d,
                                                        uint32_t ranks, double *d_G_out) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    // host arithmetic, before any launch
    if (!d_in || !d_G_out || ranks == 0 || ranks > (uint32_t)kMaxDevices || n == 0 || n > FLTEE_KRUM_MAX_N ||
        d >= ((size_t)1 << 31))
        return FLTEE_ERROR_INVALID_PARAMETER;
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_UNEXPECTED;
    const KrumGeom g = krum_geometry(n, d);
    // the largest range's partials and the running sum fit the one-GPU call's scratch
    if (!c->ws_mat.reserve(krum_scratch_bytes(n, d))) return FLTEE_ERROR_OUT_OF_MEMORY;
    c->mat_clean = 0;
    void *ws = c->ws_mat.ptr;
    double *sum = krum_gram(ws, g);
    hipStream_t s = nullptr;
    if (fl_memset_async(c->status, 0, 4, s) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    hipError_t e = hipSuccess;
    if (ranks == 1 || d == 0) {
        e = launch_krum_gram(d_in, packed != 0, n, d, nullptr, ws, c->status, s);
    } else {
        const size_t unit = packed ? 4 : 8;
        const size_t stride = packed ? RowF32::row_stride(d) * 4 : d * 8;
        bool first = true;
        for (uint32_t i = 0; i < ranks && e == hipSuccess; ++i) {
            const size_t lo = krum_cut(g, d, ranks, i), hi = krum_cut(g, d, ranks, i + 1);
            if (hi == lo) continue;  // a range without chunks: skipped in the chain
            // (a range's kernels compare idx with range-local positions, as a rank's slice holds
            // them; these rows hold the whole call's: the order flag goes to a scratch word)
            const size_t lc = (hi - lo + g.chunk_cols - 1) / g.chunk_cols;
            e = launch_krum_gram_range((const uint8_t *)d_in + lo * unit, packed != 0, stride, n, hi - lo, g, lc,
                                       nullptr, (double *)ws, lo ? c->status + 32 : c->status, s);
            if (e == hipSuccess)
                e = launch_krum_reduce_carry((const double *)ws, g.np, lc, first ? nullptr : sum, sum, s);
            first = false;
        }
    }
    if (e == hipSuccess) e = fl_memcpy_async(d_G_out, sum, g.np * g.np * 8, hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_gmed_weights_device(const void *d_records, size_t n, size_t d,
                                                    const fltee_device_opts *opts, float *d_alpha,
                                                    double *d_rho, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    // (the flag is the caller's word that opts is the base of a fltee_device_opts_gmed)
    if (!opts || !(opts->flags & FLTEE_OPT_GMED) || !d_alpha || !d_rho) return FLTEE_ERROR_INVALID_PARAMETER;
    // steps 1 - 5 take the layout, the clip and (R, nu) from the options and nothing else
    const EngineOpts in = read_opts(opts);
    EngineOpts o = default_opts();
    o.flags = (in.flags & (FLTEE_OPT_PACKED | FLTEE_OPT_BF16 | FLTEE_OPT_FP8 | FLTEE_OPT_CLIP)) | FLTEE_OPT_DENSE |
              FLTEE_OPT_GMED;
    o.clipping = in.clipping, o.d_status = in.d_status;
    o.gmed_iters = in.gmed_iters, o.gmed_nu = in.gmed_nu;
    if ((o.flags & FLTEE_OPT_BF16) && ((uintptr_t)d_records & 1)) return FLTEE_ERROR_INVALID_PARAMETER;
    if ((o.flags & FLTEE_OPT_FP8) && ((uintptr_t)d_records & 3)) return FLTEE_ERROR_INVALID_PARAMETER;
    if (plan_status(FLTEE_ALG_BASELINE, n, d, d, o) != FLTEE_SUCCESS) return FLTEE_ERROR_INVALID_PARAMETER;
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_UNEXPECTED;
    uint32_t *status = o.d_status ? o.d_status : c->status;
    hipStream_t s = (hipStream_t)stream;
    if (!o.d_status && fl_memset_async(c->status, 0, 4, s) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    return gmed_weights(d_records, n, d, o, d_alpha, d_rho, s, status);
}

extern "C" size_t fltee_workspace_bytes(uint32_t alg, size_t n, size_t k, size_t d,
                                        const fltee_device_opts *opts) {
    const EngineOpts o = read_opts(opts);
    return workspace_bytes(alg, n, k, d, o);
}

extern "C" fltee_status_t fltee_reserve(uint32_t alg, size_t n, size_t k, size_t d,
                                        const fltee_device_opts *opts) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    const EngineOpts o = read_opts(opts);
    // a refused trimmed call is refused here too, by the plan, before anything is reserved
    if ((o.flags & (FLTEE_OPT_TRIM | FLTEE_OPT_TRIM_SELECT | FLTEE_OPT_KRUM | FLTEE_OPT_GMED)) &&
        plan_status(alg, n, k, d, o) != FLTEE_SUCCESS)
        return FLTEE_ERROR_INVALID_PARAMETER;
    return reserve(alg, n, k, d, o) ? FLTEE_SUCCESS : FLTEE_ERROR_OUT_OF_MEMORY;
}

extern "C" fltee_status_t fltee_device_status(void *stream, uint32_t *status) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c || !status) return FLTEE_ERROR_UNEXPECTED;
    hipStream_t s = (hipStream_t)stream;
    if (fl_stream_sync(s) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    if (fl_memcpy(status, c->status, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    if (fl_memset(c->status, 0, 4) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    return FLTEE_SUCCESS;
}

extern "C" fltee_status_t fltee_bitonic_device(void *d_records, size_t m, uint32_t mode,
                                               uint32_t seed, void *stream) {
    if (m & (m - 1)) return FLTEE_ERROR_INVALID_PARAMETER;
    if (m >= ((size_t)1 << 31)) return FLTEE_ERROR_INVALID_PARAMETER;
    return bitonic_sort((uint64_t *)d_records, m, mode, seed, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_stable_sort_device(void *d_records16, size_t m, void *stream) {
    if (m == 0 || (m & (m - 1)) || m > stable_sort_max_records()) return FLTEE_ERROR_INVALID_PARAMETER;
    return stable_sort(d_records16, m, (hipStream_t)stream) == hipSuccess ? FLTEE_SUCCESS
                                                                          : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_fold_device(const void *d_src, void *d_dst, size_t m,
                                            size_t fold_len, size_t halo, uint32_t *d_status,
                                            void *stream) {
    if (fold_len == 0 || fold_len > m || !d_status) return FLTEE_ERROR_INVALID_PARAMETER;
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c || !c->ws_side.reserve(fold_side_bytes(m, fold_len, halo, 0, 0)))
        return FLTEE_ERROR_OUT_OF_MEMORY;
    return launch_fold((const uint64_t *)d_src, (uint64_t *)d_dst, m, fold_len, halo,
                       c->ws_side.ptr, c->ws_side.cap, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_INVALID_PARAMETER;
}

extern "C" fltee_status_t fltee_laplace_r_device(size_t d, size_t k, size_t n, uint64_t seed,
                                                 uint32_t *d_r, float *T_out, void *stream) {
    if (n == 0) return FLTEE_ERROR_INVALID_PARAMETER;
    const float T = nips19_threshold(d, k, n);
    if (T_out) *T_out = T;
    return launch_laplace_r(d, k, T, seed, d_r, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

// ---- position-range pieces of `advanced` (SURVEY §8e Option B) ----------
static bool range_ok(size_t m, size_t pos_base) {
    return m >= 2 && !(m & (m - 1)) && pos_base % m == 0 && pos_base + m <= ((size_t)1 << 31);
}

extern "C" fltee_status_t fltee_advanced_init_range_device(const void *d_records, size_t nrec,
                                                           size_t d, size_t pos_base, size_t m,
                                                           void *d_dst, void *stream) {
    return launch_advanced_init_range(d_records, nrec, d, pos_base, m, (uint64_t *)d_dst,
                                      (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_bitonic_range_sort_device(void *d_records, size_t m,
                                                          size_t pos_base, uint32_t mode,
                                                          uint32_t seed, void *stream) {
    if (!range_ok(m, pos_base)) return FLTEE_ERROR_INVALID_PARAMETER;
    return bitonic_sort_range((uint64_t *)d_records, m, mode, seed, (uint32_t)pos_base,
                              (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_bitonic_range_sort_padded_device(void *d_records, size_t m,
                                                                 size_t pos_base, size_t valid,
                                                                 uint32_t mode, uint32_t seed,
                                                                 void *stream) {
    if (!range_ok(m, pos_base)) return FLTEE_ERROR_INVALID_PARAMETER;
    if (valid == 0) return FLTEE_SUCCESS;  // pads alone: sorted as they are
    return bitonic_sort_range((uint64_t *)d_records, m, mode, seed, (uint32_t)pos_base,
                              (hipStream_t)stream, valid >= m ? 0u : (uint32_t)valid) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_bitonic_range_merge_device(void *d_records, size_t m,
                                                           size_t pos_base, uint32_t mode,
                                                           uint32_t seed, uint32_t stage_log,
                                                           void *stream) {
    if (!range_ok(m, pos_base) || ((size_t)1 << stage_log) <= m || stage_log > 31)
        return FLTEE_ERROR_INVALID_PARAMETER;
    return bitonic_merge_range((uint64_t *)d_records, m, mode, seed, stage_log,
                               (uint32_t)pos_base, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_bitonic_range_exchange_device(void *d_mine, const void *d_theirs,
                                                              size_t m, size_t pos_mine,
                                                              size_t pos_theirs, uint32_t mode,
                                                              uint32_t seed, uint32_t stage_log,
                                                              void *stream) {
    if (!range_ok(m, pos_mine) || !range_ok(m, pos_theirs) || stage_log > 31)
        return FLTEE_ERROR_INVALID_PARAMETER;
    const size_t j = pos_mine > pos_theirs ? pos_mine - pos_theirs : pos_theirs - pos_mine;
    if ((j & (j - 1)) || j < m || j >= ((size_t)1 << stage_log) || (pos_mine ^ pos_theirs) != j)
        return FLTEE_ERROR_INVALID_PARAMETER;
    return bitonic_exchange((uint64_t *)d_mine, (const uint64_t *)d_theirs, m, (uint32_t)pos_mine,
                            (uint32_t)pos_theirs, mode, seed, stage_log, log2_pow2(j),
                            (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_bitonic_range_steps_device(void *d_records, size_t m,
                                                           size_t pos_base, uint32_t mode,
                                                           uint32_t seed, uint32_t stage_log,
                                                           uint32_t step_top, uint32_t step_bot,
                                                           void *stream) {
    if (!range_ok(m, pos_base) || stage_log > 31 || step_bot > step_top ||
        step_top >= stage_log || ((size_t)1 << step_top) >= m)
        return FLTEE_ERROR_INVALID_PARAMETER;
    return bitonic_steps_range((uint64_t *)d_records, m, mode, seed, stage_log, step_top,
                               step_bot, (uint32_t)pos_base, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

// ---- position-range pieces of alg 7's stable network (k_stable.hip) -------
// host arithmetic only: every refusal comes before any HIP call
static bool stable_range_ok(size_t m, size_t pos_base) {
    return m >= ((size_t)1 << 12) && m <= ((size_t)1 << 29) && !(m & (m - 1)) && pos_base % m == 0 &&
           pos_base <= ((size_t)1 << 31) && pos_base + m <= ((size_t)1 << 31);
}

extern "C" fltee_status_t fltee_stable_init_range_device(const void *d_records, size_t nrec, size_t d,
                                                         size_t pos_base, size_t m, void *d_dst16,
                                                         void *stream) {
    if (!stable_range_ok(m, pos_base) || nrec >= ((size_t)1 << 31) || d >= ((size_t)1 << 31) ||
        nrec + d >= ((size_t)1 << 31))
        return FLTEE_ERROR_INVALID_PARAMETER;
    return stable_init_range(d_records, nrec, d, pos_base, m, d_dst16, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_stable_range_sort_device(void *d_rec16, size_t m, size_t pos_base,
                                                         size_t valid, void *stream) {
    if (!stable_range_ok(m, pos_base)) return FLTEE_ERROR_INVALID_PARAMETER;
    if (valid == 0) return FLTEE_SUCCESS;  // pads alone: sorted as they are
    return stable_sort_range(d_rec16, m, pos_base, (hipStream_t)stream, valid >= m ? 0 : valid) ==
                   hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_stable_range_exchange_device(void *d_mine16, const void *d_theirs16,
                                                             size_t m, size_t pos_mine,
                                                             size_t pos_theirs, uint32_t stage_log,
                                                             void *stream) {
    if (!stable_range_ok(m, pos_mine) || !stable_range_ok(m, pos_theirs) || pos_mine == pos_theirs ||
        stage_log > 31)
        return FLTEE_ERROR_INVALID_PARAMETER;
    const size_t j = pos_mine > pos_theirs ? pos_mine - pos_theirs : pos_theirs - pos_mine;
    // a power of two below the stage; the partner differs in that one position bit
    if ((j & (j - 1)) || j >= ((size_t)1 << stage_log) || (pos_mine ^ pos_theirs) != j)
        return FLTEE_ERROR_INVALID_PARAMETER;
    return stable_exchange(d_mine16, d_theirs16, m, pos_mine, pos_theirs, stage_log,
                           (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_stable_range_merge_device(void *d_rec16, size_t m, size_t pos_base,
                                                          uint32_t stage_log, void *stream) {
    if (!stable_range_ok(m, pos_base) || stage_log > 31 || ((size_t)1 << stage_log) <= m)
        return FLTEE_ERROR_INVALID_PARAMETER;
    return stable_merge_range(d_rec16, m, pos_base, stage_log, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_stable_range_strip_device(const void *d_rec16, size_t m, void *d_dst8,
                                                          void *stream) {
    if (!stable_range_ok(m, 0)) return FLTEE_ERROR_INVALID_PARAMETER;
    return stable_strip_range(d_rec16, m, (uint64_t *)d_dst8, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" size_t fltee_fold_context(size_t halo) { return fold_context(halo); }

extern "C" size_t fltee_fold_side_bytes(size_t span, size_t halo) {
    return fold_side_bytes(span, (size_t)1 << 62, halo, 1, 1);
}

extern "C" fltee_status_t fltee_fold_range_device(const void *d_src, void *d_dst, size_t m,
                                                  size_t origin, size_t end, int64_t pos_base,
                                                  size_t fold_len, size_t halo, void *d_side,
                                                  void *stream) {
    // range mode: [0, origin) holds >= fold_context(halo) + 1 records of context
    if (!d_side || origin < fold_context(halo) + 1 || end > m || origin >= end || (origin & 1) ||
        (end & 1) || (m & 1))
        return FLTEE_ERROR_INVALID_PARAMETER;
    if (end < m ? false : (int64_t)end + pos_base < (int64_t)fold_len)
        return FLTEE_ERROR_INVALID_PARAMETER;  // needs the next range's first record
    return launch_fold_range((const uint64_t *)d_src, (uint64_t *)d_dst, m, origin, end,
                             (long long)pos_base, fold_len, halo, (FoldSide *)d_side,
                             (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_fold_range_total_device(const void *d_side, size_t span,
                                                        size_t halo, void *d_total, void *stream) {
    if (!d_side || !d_total) return FLTEE_ERROR_INVALID_PARAMETER;
    const size_t lanes = fold_lanes(span, (size_t)1 << 62, halo, 1, 1);
    return launch_fold_range_total((const FoldSide *)d_side, lanes, (FoldAgg *)d_total,
                                   (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_fold_range_patch_device(void *d_dst, size_t origin, size_t end,
                                                        int64_t pos_base, size_t fold_len,
                                                        size_t halo, const void *d_side,
                                                        const void *d_prev_totals, size_t n_prev,
                                                        void *stream) {
    if (!d_dst || !d_side || origin >= end || (n_prev && !d_prev_totals))
        return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_fold_range_patch((uint64_t *)d_dst, end - origin, origin, (long long)pos_base,
                                   fold_len, halo, (const FoldSide *)d_side,
                                   (const FoldAgg *)d_prev_totals, n_prev, (hipStream_t)stream) ==
                   hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_compact_range_device(const void *d_chunk, size_t c, size_t d,
                                                     void *d_buf, void *d_tmp, float coef,
                                                     float *d_out, void *stream) {
    if (d + c >= ((size_t)1 << 29)) return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_compact_offset((const uint64_t *)d_chunk, c, d, (uint64_t *)d_buf,
                                 (uint64_t *)d_tmp, coef, d_out, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_nips19_build_range_device(const void *d_records, size_t nrec,
                                                          const uint32_t *d_r, size_t d,
                                                          size_t tf, size_t pos_base, size_t m,
                                                          void *d_dst, void *stream) {
    if (nrec + d * tf >= ((size_t)1 << 31)) return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_nips19_build_range(d_records, nrec, d_r, d, tf, pos_base, m, (uint64_t *)d_dst,
                                     (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_safe_aggregate_device(const void *d_src, size_t m, size_t d,
                                                      float *d_out, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_UNEXPECTED;
    if (m >= ((size_t)1 << 31)) return FLTEE_ERROR_INVALID_PARAMETER;
    return safe_aggregate_ordered(c, (const uint64_t *)d_src, m, d, 1.0f, d_out, false, c->status,
                                  (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

// safe_aggregate split for position ranges (nips19 over several GPUs): each range's
// entries with idx < d in position order, then the ordered fold of their concatenation
// in range order on the root — the one-GPU result bit for bit.
extern "C" fltee_status_t fltee_select_device(const void *d_src, size_t m, size_t d, void *d_list,
                                              size_t cap, size_t *count, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c || !count || m >= ((size_t)1 << 31)) return FLTEE_ERROR_INVALID_PARAMETER;
    hipStream_t s = (hipStream_t)stream;
    *count = 0;
    if (m == 0 || d == 0) return FLTEE_SUCCESS;
    const size_t nb = select_tiles(m);
    if (!c->ws_cnt.reserve((2 * nb + 2) * 4)) return FLTEE_ERROR_OUT_OF_MEMORY;
    uint32_t *cnt = (uint32_t *)c->ws_cnt.ptr, *base = cnt + nb + 1;
    size_t lc = 0;
    if (launch_select_count((const uint64_t *)d_src, m, d, cnt, base, s) != hipSuccess ||
        read_device_word(c, base + nb, &lc, s) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    *count = lc;
    if (lc > cap || (lc && !d_list)) return FLTEE_ERROR_INVALID_PARAMETER;  // caller grows the list
    if (lc && launch_select_write((const uint64_t *)d_src, m, d, base, (uint64_t *)d_list, s) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    return FLTEE_SUCCESS;
}

extern "C" fltee_status_t fltee_ordered_list_device(const void *d_list, size_t lc, size_t d,
                                                    float coef, float *d_out, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c || lc >= ((size_t)1 << 29)) return FLTEE_ERROR_INVALID_PARAMETER;
    if (d == 0) return FLTEE_SUCCESS;
    return ordered_from_list(c, (const uint64_t *)d_list, lc, d, coef, d_out, false, c->status,
                             (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

// test hook: the ordered fold's stable sort by min(idx, d) alone (fltee_agg.h)
extern "C" fltee_status_t fltee_debug_sort_records_device(const void *d_rec, size_t n, size_t d,
                                                          void *d_sorted, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c || d == 0 || n >= ((size_t)1 << 29) || (n && (!d_rec || !d_sorted)))
        return FLTEE_ERROR_INVALID_PARAMETER;
    return debug_sort_records(c, d_rec, n, d, d_sorted, c->status, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" void fltee_debug_set_seed(uint64_t seed) { set_debug_seed(seed); }

// test hook: the launch trace (common.h).  on = 1 clears it and starts recording, 0 stops.
extern "C" void fltee_debug_trace(int on) {
    std::lock_guard<std::mutex> lk(fltee::g_trace_mu);
    if (on) {
        fltee::g_trace_text.clear();
        fltee::g_trace_lines = 0;
    }
    fltee::g_trace.store(on != 0);
}

// the trace so far as text (one line per event: what|site|a|b|c); returns its length
// (copies at most cap - 1 bytes and a NUL into buf when buf is given)
extern "C" size_t fltee_debug_trace_text(char *buf, size_t cap) {
    std::lock_guard<std::mutex> lk(fltee::g_trace_mu);
    const std::string &t = fltee::g_trace_text;
    if (buf && cap) {
        const size_t n = t.size() < cap - 1 ? t.size() : cap - 1;
        std::memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return t.size();
}

// the planned network schedule (k_bitonic.hip plan_network), 8 words per launch
extern "C" size_t fltee_debug_network_plan(uint32_t mlog, uint32_t tlog, uint32_t nt, int rmax,
                                           uint32_t *out, size_t cap) {
    return fltee::debug_plan(mlog, tlog, nt, rmax, out, cap);
}

// the pad-only units a network launch skips (k_bitonic.hip pad_units): {live, hole_at, hole_len}
extern "C" void fltee_debug_pad_units(uint32_t mode, uint32_t valid, uint32_t mlog, uint32_t pbase,
                                      uint32_t ilog, uint32_t jstep, uint32_t sblog, uint32_t uplog,
                                      uint32_t *out) {
    fltee::debug_pad_units(mode, valid, mlog, pbase, ilog, jstep, sblog, uplog, out);
}

// measurement hook: streaming passes launched and the bytes they sweep since the last reset
extern "C" void fltee_debug_net_stats(uint64_t *launches, uint64_t *bytes, int reset) {
    if (launches) *launches = fltee::g_net_launches.load();
    if (bytes) *bytes = fltee::g_net_bytes.load();
    if (reset) {
        fltee::g_net_launches.store(0);
        fltee::g_net_bytes.store(0);
    }
}

// measurement hook: per-launch log of the accounted launches.  on = 1 clears the log and
// starts recording (an event on the launch's stream before each accounted launch); on = 0
// records the final event on `stream` (after the last launch of the timed call) and stops.
extern "C" void fltee_debug_net_timing(int on, void *stream) {
    std::lock_guard<std::mutex> lk(fltee::g_net_mu);
    if (on) {
        fltee::net_log_clear();
        fltee::g_net_timing.store(true);
        return;
    }
    fltee::g_net_timing.store(false);
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) == hipSuccess) {
        if (hipEventRecord(e, (hipStream_t)stream) == hipSuccess)
            fltee::g_net_log.push_back({nullptr, 0, e});
        else
            (void)hipEventDestroy(e);
    }
}

// entry i of the log (the caller has synchronised the stream): kernel name, launch-side
// bytes and the time to the next entry's event (ms).  Returns the number of launches
// logged (the final event not counted); i past it fills nothing.
extern "C" size_t fltee_debug_net_log(size_t i, char *name, size_t name_cap, uint64_t *bytes,
                                      float *ms) {
    std::lock_guard<std::mutex> lk(fltee::g_net_mu);
    const auto &L = fltee::g_net_log;
    const size_t nl = L.empty() ? 0 : (L.back().kernel ? L.size() : L.size() - 1);
    if (i < nl) {
        if (name && name_cap) {
            std::snprintf(name, name_cap, "%s", L[i].kernel ? L[i].kernel : "");
        }
        if (bytes) *bytes = L[i].bytes;
        if (ms) {
            *ms = -1.0f;
            if (i + 1 < L.size()) (void)hipEventElapsedTime(ms, L[i].ev, L[i + 1].ev);
        }
    }
    return nl;
}

// ---- value-only dense slices (k_rows.hip): f32 rows ... ------------------------
extern "C" size_t fltee_packed_slice_bytes(size_t d) { return row_units(kRowsF32, d) * 8; }

extern "C" fltee_status_t fltee_unpack_dense_device(const void *d_packed, size_t n, size_t d,
                                                    void *d_records, void *stream) {
    if (n == 0 || d == 0 || d > 0xFFFFFFFFull || !d_packed || !d_records)
        return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_unpack_rows(kRowsF32, d_packed, n, d, (uint64_t *)d_records, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_client_pack_dense_device(const float *d_values, size_t n, size_t d,
                                                         void *d_packed, void *stream) {
    if (n == 0 || d == 0 || d > 0xFFFFFFFFull || !d_values || !d_packed)
        return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_pack_rows(kRowsF32, d_values, n, d, d_packed, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

// ---- ... and bf16 rows ---------------------------------------------------------
extern "C" size_t fltee_bf16_slice_bytes(size_t d) { return row_units(kRowsBf16, d) * 8; }

extern "C" fltee_status_t fltee_unpack_bf16_device(const void *d_rows, size_t n, size_t d, void *d_records,
                                                   void *stream) {
    if (n == 0 || d == 0 || d > 0xFFFFFFFFull || !d_rows || !d_records || ((uintptr_t)d_rows & 1))
        return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_unpack_rows(kRowsBf16, d_rows, n, d, (uint64_t *)d_records, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_client_pack_bf16_device(const float *d_values, size_t n, size_t d,
                                                        void *d_rows, void *stream) {
    if (n == 0 || d == 0 || d > 0xFFFFFFFFull || !d_values || !d_rows || ((uintptr_t)d_rows & 1))
        return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_pack_rows(kRowsBf16, d_values, n, d, d_rows, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

// ---- ... and fp8 rows (e4m3fn codes, a per-client f32 scale in the last unit) ------------
extern "C" size_t fltee_fp8_slice_bytes(size_t d) { return row_units(kRowsFp8, d) * 8; }

extern "C" fltee_status_t fltee_unpack_fp8_device(const void *d_rows, size_t n, size_t d, void *d_records,
                                                  void *stream) {
    if (n == 0 || d == 0 || d > 0xFFFFFFFFull || !d_rows || !d_records || ((uintptr_t)d_rows & 3))
        return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_unpack_rows(kRowsFp8, d_rows, n, d, (uint64_t *)d_records, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_client_pack_fp8_device(const float *d_values, size_t n, size_t d, void *d_rows,
                                                       void *stream) {
    if (n == 0 || d == 0 || d > 0xFFFFFFFFull || !d_values || !d_rows || ((uintptr_t)d_rows & 3))
        return FLTEE_ERROR_INVALID_PARAMETER;
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_INVALID_PARAMETER;
    // (the clients' scales between the two launches: the producers' coefficient scratch)
    if (!c->ws_client_coef.reserve(n * 4)) return FLTEE_ERROR_OUT_OF_MEMORY;
    return launch_pack_fp8(d_values, n, d, (float *)c->ws_client_coef.ptr, d_rows, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_sum_rows_device(const float *d_rows, size_t nrows, size_t d,
                                                float coef, float *d_out, void *stream) {
    if (nrows == 0) return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_rows_accumulate(d_rows, nrows, d, coef, d_out, false, (hipStream_t)stream) ==
                   hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_dp_noise_device(float *d_out, size_t d, float sigma,
                                                float clipping, size_t n, uint64_t seed,
                                                void *stream) {
    if (n == 0) return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_dp_noise(d_out, d, sigma, clipping, n, seed ? seed : next_seed(),
                           (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

namespace fltee {
void set_dense_variant(int v); void set_compact_variant(int v); void set_fold_compact(int on);
bool fold_compact_geometry(size_t M, size_t L, size_t d, size_t halo, uint64_t out[7]);
bool fold_stream_geometry(size_t span, size_t fold_len, size_t halo, uint64_t out[5]);
hipError_t launch_read_floor(const void *src, size_t bytes, uint32_t *sink, unsigned blocks, hipStream_t s);
}
// measurement hook (bench.py): a plain streaming read of `bytes` (16-B multiple) of d_src;
// d_sink: `blocks` words
extern "C" int fltee_debug_read_floor(const void *d_src, size_t bytes, void *d_sink, unsigned blocks,
                                      void *stream) {
    return fltee::launch_read_floor(d_src, bytes, (uint32_t *)d_sink, blocks, (hipStream_t)stream) ==
                   hipSuccess ? 0 : 1;
}
// tuning hook (not part of the public header)
extern "C" void fltee_debug_set_dense_variant(int v) { fltee::set_dense_variant(v); }
// A/B hook: 0 runs advanced's second bitonic sort instead of the compaction network
extern "C" void fltee_debug_set_advanced_compaction(int on) { fltee::g_advanced_compaction = on != 0; }
extern "C" void fltee_debug_set_compact_variant(int v) { fltee::set_compact_variant(v); }
// A/B hook: 0 runs advanced's fold as its own pass before the compaction
extern "C" void fltee_debug_set_fold_compact(int on) { fltee::set_fold_compact(on); }
// A/B hook: 0 runs the networks over the pad-only stage blocks too
extern "C" void fltee_debug_set_pad_skip(int on) { fltee::set_pad_skip(on); }
extern "C" void fltee_debug_set_radix_order(int on) { fltee::set_radix_order(on); }
extern "C" void fltee_set_path_oram_tree(int on) {
    std::lock_guard<std::recursive_mutex> lk(fltee::api_mutex());
    fltee::set_oram_tree(on);
}
extern "C" void fltee_set_advanced_exact_runs(int on) {
    std::lock_guard<std::recursive_mutex> lk(fltee::api_mutex());
    fltee::set_exact_runs(on);
}
extern "C" void fltee_set_bubble_ecall(int on) {
    std::lock_guard<std::recursive_mutex> lk(fltee::api_mutex());
    fltee::set_bubble_ecall(on);
}
// test hook: blocks a bucket of the tree ORAM takes on eviction (4; 0 forces the stash)
extern "C" void fltee_debug_set_oram_bucket(int z) {
    std::lock_guard<std::recursive_mutex> lk(fltee::api_mutex());
    fltee::set_oram_bucket(z);
}
extern "C" void fltee_debug_set_aes_variant(int v) {
    std::lock_guard<std::recursive_mutex> lk(fltee::api_mutex());
    fltee::set_aes_variant(v);
}
extern "C" void fltee_debug_set_swizzle(int on) { fltee::set_swizzle(on); }
extern "C" void fltee_debug_set_fused_init(int on) { fltee::set_fused_init(on); }
// test hook: the one decision aggregate() takes about a public shape (engine.h Plan), host
// only: no device is touched.  Returns what fltee_aggregate_device returns for the shape
// before it launches anything (FLTEE_SUCCESS or the 0x2 refusal) and writes 4 + kWsCount
// words: out[0] the route (engine.h Route), out[1] the `advanced` family's tail (Tail; alg 6:
// a full batch's), out[2] M (the sorted array: advanced / alg 7 / an alg-6 batch / the lazy
// tree's readout / nips19; 0 otherwise), out[3] the effective fold halo, then the bytes of
// each scratch buffer in Ws order (a, b, mat, r, coef, rec, keys, radix, oram, side, lb, s16,
// cnt, sel) — their sum is fltee_workspace_bytes.  sel is always 0: nips19's selected list,
// and the keys / radix its ordered fold takes, are sized from a count read back from the
// device.  The sizes are filled in for a refused shape too.
extern "C" fltee_status_t fltee_debug_plan(uint32_t alg, size_t n, size_t k, size_t d,
                                           const fltee_device_opts *opts, uint64_t *out) {
    return fltee::debug_plan_words(alg, n, k, d, read_opts(opts), out);
}
// test hook: the Gram pass's geometry for (n, d) (k_krum.hip krum_geometry), host only:
// {padded rows, 16-row tiles, 128-row macro-tiles, columns a chunk, chunks, scratch bytes}
extern "C" void fltee_debug_krum_geometry(size_t n, size_t d, uint64_t *out) {
    const fltee::KrumGeom g = fltee::krum_geometry(n, d);
    out[0] = g.np, out[1] = g.tiles, out[2] = g.macros, out[3] = g.chunk_cols, out[4] = g.chunks;
    out[5] = fltee::krum_scratch_bytes(n, d);
}
// test hooks: which engine scratch buffers grew (allocated) since the last call — bit w for
// buffer w in Ws order — read and cleared; and the current device's engine scratch released
// (with the scatter rows' clean mark and the look-back epoch), so a test can start from empty.
extern "C" uint32_t fltee_debug_scratch_grown(void) { return fltee::g_scratch_grown.exchange(0); }
extern "C" void fltee_debug_scratch_release(void) {
    std::lock_guard<std::recursive_mutex> lk(fltee::api_mutex());
    fltee::release_scratch();
}
// test hook: how run_advanced folds a whole array of L = n * k + d entries (M = next_pow2(L),
// fold_len == L, halo = the effective one: opts.fold_halo, or n) under the current A/B
// settings.  Read-only, host only.  out[0]: 1 the fold fused into the compaction's first
// pass, then {per, S, ntiles, lim, G, last pass (FINAL != 0), Hr}; 2 the streaming fold +
// patch, 3 the one-lane walk, then {Hr, C, lanes, prefetch depth, patch blocks, span, 0}.
extern "C" void fltee_debug_fold_geometry(size_t M, size_t L, size_t d, size_t halo, uint64_t *out) {
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (fltee::g_advanced_compaction && fltee::fold_compact_geometry(M, L, d, halo, out + 1)) {
        out[0] = 1;
        return;
    }
    const size_t span = fltee::g_advanced_compaction ? fltee::advanced_fold_span(L, M) : M;
    out[0] = fltee::fold_stream_geometry(span, L, halo, out + 1) ? 2 : 3;
    out[6] = span;
}
// A/B hook: 0 writes nips19's shuffled array out and selects in separate passes
extern "C" void fltee_debug_set_nips19_fused_select(int on) { fltee::g_nips19_fused_select = on != 0; }
// test hook: the fused-producer sort alone (gen 1: advanced, 2: nips19 with key seed),
// into d_data[0, m); INVALID_PARAMETER when m is too small to fuse
extern "C" fltee_status_t fltee_debug_sort_fused(uint32_t gen, void *d_data, size_t m,
                                                 const void *d_rec, size_t nrec, const uint32_t *d_r,
                                                 size_t d, size_t tf, uint32_t seed, void *stream) {
    if (!d_data || (nrec && !d_rec) || (gen == 2 && d && tf && !d_r)) return FLTEE_ERROR_INVALID_PARAMETER;
    hipError_t e;
    if (gen == 1) e = fltee::bitonic_sort_advanced((uint64_t *)d_data, m, d_rec, nrec, d, (hipStream_t)stream);
    else if (gen == 2)
        e = fltee::bitonic_sort_nips19((uint64_t *)d_data, m, seed, d_rec, nrec, d_r, d, tf, (hipStream_t)stream);
    else return FLTEE_ERROR_INVALID_PARAMETER;
    if (e == hipErrorNotSupported || e == hipErrorInvalidValue) return FLTEE_ERROR_INVALID_PARAMETER;
    return e == hipSuccess ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
}
