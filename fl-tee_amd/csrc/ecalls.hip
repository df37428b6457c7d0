// ecalls.hip — the four ECALLs of Enclave.edl on an MI355X (host side).
//
// State machine restated from secure_aggregation/enclave/src/lib.rs:
//   FL_CONFIG_MAP (lib.rs:83-91, fl_config.rs)      -> g_cfg
//   SESSION_KEYS (lib.rs:93-101, session_key_store) -> g_keys (id set; the key is
//                                                      a pure function of the id)
//   single TCS (Enclave.config.xml:6)               -> api_mutex()
// The data path runs on the eid's GPU: "Loading" = H2D of the ciphertext,
// "Decryption" = AES-128-CTR kernel, "Aggregation" = engine.hip + DP noise.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "common.h"
#include "engine.h"
#include "group.h"

namespace fltee {

std::recursive_mutex &api_mutex() {
    static std::recursive_mutex mu;
    return mu;
}

struct FLConfig {  // fl_config.rs:29-44
    std::vector<uint32_t> client_ids;
    size_t d = 0, k = 0;
    float sigma = 0, clipping = 0, alpha = 0, ratio = 0;
    uint32_t alg = 0, round = 0;
    uint8_t verbose = 0, dp = 0;
    std::set<uint32_t> sampled;  // current_sampled_clients (HashSet)
};

static std::map<uint32_t, FLConfig> g_cfg;
static std::set<uint32_t> g_keys;
static bool g_have_keys = false;
static std::vector<int> g_eid_dev;  // eid - 1 -> hip device (a group's root device)
static std::map<fltee_eid_t, Group *> g_groups;  // eids from fltee_device_init_multi

static Group *group_of(fltee_eid_t eid) {
    auto it = g_groups.find(eid);
    return it == g_groups.end() ? nullptr : it->second;
}

void aes128_expand_key(const uint8_t key[16], uint32_t rk[44]);

static inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static size_t f32_to_usize_sat(float x) {
    if (!(x > 0.0f)) return 0;
    if (x >= 18446744073709551616.0f) return SIZE_MAX;
    return (size_t)x;
}

// sgx_rand::sample reservoir (common.rs:101-105) driven by Philox4x32-10.
static void sample_client_ids(const std::vector<uint32_t> &ids, size_t amount, uint64_t seed,
                              std::vector<uint32_t> &out) {
    const size_t take = std::min(amount, ids.size());
    out.assign(ids.begin(), ids.begin() + take);
    if (take != amount) return;
    uint64_t counter = 0;
    auto draw = [&]() {
        uint32_t c[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), 0u, FLTEE_STREAM_SAMPLE};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        ++counter;
        return ((uint64_t)c[1] << 32) | c[0];
    };
    for (size_t i = 0; i + amount < ids.size(); ++i) {
        const uint64_t range = (uint64_t)(i + 1 + amount);
        const uint64_t zone = UINT64_MAX - UINT64_MAX % range;
        uint64_t v;
        do { v = draw(); } while (v >= zone);
        const uint64_t kk = v % range;
        if (kk < amount) out[kk] = ids[amount + i];
    }
}

static DeviceCtx *eid_ctx(fltee_eid_t eid) {
    if (eid == 0 || eid > g_eid_dev.size() || g_eid_dev[eid - 1] < 0) return nullptr;
    const int dev = g_eid_dev[eid - 1];
    if (hipSetDevice(dev) != hipSuccess) return nullptr;
    DeviceCtx *c = device_ctx(dev);
    if (c && !c->stream) {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
        if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
        for (int i = 0; i < DeviceCtx::kCopyEvents; ++i)
            if (hipEventCreateWithFlags(&c->copy_ev[i], hipEventDisableTiming) != hipSuccess) return nullptr;
    }
    return c;
}

static uint32_t check_uploaded(const FLConfig &cfg, const uint32_t *ids, size_t n) {
    if (n != cfg.sampled.size()) {  // lib.rs:269-272
        std::printf("[VERIFICATION ERROR] Uploaded client id is not matched for secure sampled one.\n");
        return FLTEE_ERROR_INVALID_PARAMETER;
    }
    for (size_t i = 0; i < n; ++i)
        if (!cfg.sampled.count(ids[i])) {
            std::printf("[VERIFICATION ERROR] Uploaded client id is not matched for secure sampled one.\n");
            return FLTEE_ERROR_INVALID_PARAMETER;
        }
    return FLTEE_SUCCESS;
}

// AES-128 round keys of the n clients' session keys (session_key_store.rs:21-22)
static void client_round_keys(const uint32_t *ids, size_t n, std::vector<uint32_t> &rk) {
    rk.resize(n * 44);
    aes128_session_round_keys(ids, n, rk.data());
}

// H2D + GPU AES-CTR decrypt of n slices of bpc bytes -> c->records (n * (bpc/8) records)
// Loading + decryption (lib.rs:285-343), pipelined: the ciphertext crosses PCIe in
// client chunks of ~64 MB on the copy stream, and each chunk's AES-CTR kernel runs on
// the ECALL stream as soon as its copy lands, under the next chunk's copy.  Timers
// (execution_time_results[0..1]): t_load = until the last chunk has landed; t_dec =
// the decryption left after it (the part not hidden under the copies).
constexpr size_t kLoadChunkBytes = (size_t)64 << 20;

// ---- authenticated uploads (fltee_set_upload_aead; k_ghash.hip) ----------------------
static bool g_upload_aead = false;
// What follows a failed tag (fltee_set_upload_aead_policy): ABORT, REPORT or DROP, and DROP's
// quorum (>= 1)
static int g_aead_policy = FLTEE_AEAD_ABORT;
static size_t g_aead_min_survivors = 1;

// The verdict of fl_id's last authenticated ECALL under REPORT / DROP (fltee_auth_report):
// the failed client ids in upload order; empty after a clean call
struct AuthReport {
    uint32_t round = 0;
    std::vector<uint32_t> failed;
};
static std::map<uint32_t, AuthReport> g_auth_reports;

// ---- value-only dense uploads (fltee_set_upload_packed, _bf16, _fp8; k_rows.hip) ----
static bool g_upload_packed = false, g_upload_bf16 = false, g_upload_fp8 = false;
// robust aggregation (fltee_set_dense_trim): the per-mille of clients trimmed on each side of
// every coordinate of a dense call, 0 = off
static uint32_t g_dense_trim = 0;
// fltee_set_dense_trim_select: a trimmed call with t > FLTEE_TRIM_MAX is answered by selection
// (k_trim_select.hip) instead of refused; t <= FLTEE_TRIM_MAX stays on the list kernel
static bool g_dense_trim_select = false;
// Multi-Krum (fltee_set_dense_krum): the assumed Byzantine clients f and the clients kept m of
// every ECALL on the dense path; (0, 0) (default): off
static uint32_t g_dense_krum_f = 0, g_dense_krum_m = 0;
static bool dense_krum_on() { return (g_dense_krum_f | g_dense_krum_m) != 0; }
// the geometric median (fltee_set_dense_gmed): the Weiszfeld iterations R and the smoothing floor nu
// of every ECALL on the dense path; R = 0 (default): off
static uint32_t g_dense_gmed_iters = 0;
static double g_dense_gmed_nu = 0.0;
static bool dense_gmed_on() { return g_dense_gmed_iters != 0; }

// The trim count (include/fltee_agg.h fltee_trim_count): the one place it is decided.
static size_t trim_count(size_t n, uint32_t per_mille) {
    if (n == 0) return 0;
    if (per_mille > 500) per_mille = 500;
    const size_t t = (size_t)((unsigned __int128)n * per_mille / 1000), cap = (n - 1) / 2;
    return t < cap ? t : cap;
}

// The value-row rule (include/fltee_agg.h fltee_upload_is_packed, fltee_upload_is_bf16): the
// format's switch is on, the request declares a dense upload of d >= rows_min_d parameters,
// and every client's ciphertext is exactly one slice of the format (ct_bytes: 0 when the
// payload is not n equal slices).  Below rows_min_d a slice has the size of a record (d = 1)
// or, bf16 at d = 2, of an f32 slice, or, fp8 at d <= 12, of a bf16 slice or more (rows.h
// rows_min_d); from there the sizes differ, so one server answers all four formats.
static bool upload_is_rows(RowFmt f, bool on, size_t d, size_t k_req, size_t ct_bytes) {
    return on && d >= rows_min_d(f) && (k_req == 0 || k_req == d) && ct_bytes / 8 == row_units(f, d) &&
           ct_bytes % 8 == 0;
}

// A call's upload format: the FLTEE_OPT_ flag its aggregate takes (0: records) and the bit its
// AAD's alg word carries.  Packed is tried first.
struct UploadFmt {
    uint32_t opt, aad_bit;
};
static UploadFmt upload_format(bool packed_on, bool bf16_on, bool fp8_on, size_t d, size_t k_req,
                               size_t ct_bytes) {
    if (upload_is_rows(kRowsF32, packed_on, d, k_req, ct_bytes)) return {FLTEE_OPT_PACKED, FLTEE_AAD_PACKED_BIT};
    if (upload_is_rows(kRowsBf16, bf16_on, d, k_req, ct_bytes)) return {FLTEE_OPT_BF16, FLTEE_AAD_BF16_BIT};
    if (upload_is_rows(kRowsFp8, fp8_on, d, k_req, ct_bytes)) return {FLTEE_OPT_FP8, FLTEE_AAD_FP8_BIT};
    return {0u, 0u};
}

static bool keeps_verdict(bool aead) { return aead && g_aead_policy != FLTEE_AEAD_ABORT; }

// fail: the n fail words as load_and_decrypt read them back (the word gathering them behind)
static void store_auth_report(uint32_t fl_id, uint32_t round, const uint32_t *ids, size_t n,
                              const std::vector<uint32_t> &fail) {
    AuthReport &r = g_auth_reports[fl_id];
    r.round = round;
    r.failed.clear();
    for (size_t i = 0; i < n; ++i)
        if (fail[i]) r.failed.push_back(ids[i]);
}

// One call's GCM parameters: the IV, and aad_len bytes of AAD per client.
struct GcmArgs {
    uint8_t iv[12] = {};
    std::vector<uint8_t> aad;
    size_t aad_len = 0;
};

static inline void put_be32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

// What the ECALLs bind: IV = BE32(fl_id) || BE32(round) || BE32(0), AAD = BE32(fl_id) ||
// BE32(round) || BE32(client_id) || BE32(aggregation_alg) — alg: a packed call passes
// aggregation_alg | FLTEE_AAD_PACKED_BIT, a bf16 call aggregation_alg | FLTEE_AAD_BF16_BIT, an fp8
// call aggregation_alg | FLTEE_AAD_FP8_BIT, so a slice sealed for one format fails under the others
static void ecall_gcm_args(uint32_t fl_id, uint32_t round, const uint32_t *ids, size_t n,
                           uint32_t alg, GcmArgs &g) {
    put_be32(g.iv, fl_id);
    put_be32(g.iv + 4, round);
    put_be32(g.iv + 8, 0);
    g.aad_len = 16;
    g.aad.resize(n * 16);
    for (size_t c = 0; c < n; ++c) {
        put_be32(&g.aad[16 * c], fl_id);
        put_be32(&g.aad[16 * c + 4], round);
        put_be32(&g.aad[16 * c + 8], ids[c]);
        put_be32(&g.aad[16 * c + 12], alg);
    }
}

static bool gcm_sizes_ok(size_t ct_bytes, size_t aad_len) {
    return aad_len <= FLTEE_GCM_MAX_AAD && (uint64_t)ct_bytes <= ((uint64_t)1 << 36) - 32;
}

// The device side of a call's keys: the round keys into c->round_keys, per client H and
// E_K(J0) then the AAD padded to 64 bytes into c->gcm_sub (host: the caller's vector, alive
// until the stream is synchronised), the powers of H into c->gcm_pow; the partial and fail
// scratch reserved.  The word after the n fail words gathers FLTEE_DEV_ERR_AUTH for the
// ECALLs.
struct GcmDev {
    const uint32_t *rk;
    const uint8_t *sub, *aad;
    const uint8_t *pow;
    uint8_t *part;
    uint32_t *fail, *auth_word;
    size_t P;
};

// the host side of it: [round keys: n x 176][H, E_K(J0): n x 32][AAD padded: n x 64]
static void gcm_host_keys(const uint32_t *ids, size_t n, const uint8_t iv[12], const uint8_t *aad,
                          size_t aad_len, std::vector<uint8_t> &host) {
    const size_t rkb = n * 44 * 4, subb = n * 32, aadb = n * 64;
    host.assign(rkb + subb + aadb, 0);
    uint32_t *rk = (uint32_t *)host.data();
    aes128_session_round_keys(ids, n, rk);
    aes128_gcm_subkeys(rk, n, iv, host.data() + rkb);
    for (size_t i = 0; i < n && aad_len; ++i)
        std::memcpy(host.data() + rkb + subb + 64 * i, aad + aad_len * i, aad_len);
}

static uint32_t gcm_prepare(DeviceCtx *c, const uint32_t *ids, size_t n, size_t ct_bytes,
                            const uint8_t iv[12], const uint8_t *aad, size_t aad_len,
                            std::vector<uint8_t> &host, hipStream_t s, GcmDev &d) {
    const size_t rkb = n * 44 * 4, subb = n * 32, aadb = n * 64;
    if (!c->round_keys.reserve(rkb) || !c->gcm_sub.reserve(subb + aadb) ||
        !c->gcm_pow.reserve(ghash_pow_bytes(n)) ||
        !c->gcm_part.reserve(ghash_part_bytes(n, ct_bytes, aad_len) + 16) ||
        !c->gcm_fail.reserve(n * 4 + 16))
        return FLTEE_ERROR_OUT_OF_MEMORY;
    gcm_host_keys(ids, n, iv, aad, aad_len, host);
    if (fl_memcpy_async(c->round_keys.ptr, host.data(), rkb, hipMemcpyHostToDevice, s) != hipSuccess ||
        fl_memcpy_async(c->gcm_sub.ptr, host.data() + rkb, subb + aadb, hipMemcpyHostToDevice, s) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    d.rk = (const uint32_t *)c->round_keys.ptr;
    d.sub = (const uint8_t *)c->gcm_sub.ptr;
    d.aad = d.sub + subb;
    d.pow = (const uint8_t *)c->gcm_pow.ptr;
    d.part = (uint8_t *)c->gcm_part.ptr;
    d.fail = (uint32_t *)c->gcm_fail.ptr;
    d.auth_word = d.fail + n;
    d.P = ghash_segments(ct_bytes, aad_len);
    if (launch_ghash_powers(d.sub, n, c->gcm_pow.ptr, s) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    return FLTEE_SUCCESS;
}

// GHASH + tag check of the clients [c0, c0 + nc) of a prepared call: cipher points at client
// c0's slice; fail[c0 ..] and *status are written
static uint32_t gcm_verify(const GcmDev &d, size_t c0, size_t nc, const uint8_t *cipher, size_t ct_bytes,
                           size_t aad_len, uint32_t *fail, uint32_t *status, hipStream_t s) {
    const size_t stride = ct_bytes + FLTEE_GCM_TAG_BYTES;
    const uint8_t *pow = d.pow + ghash_pow_bytes(c0);
    uint8_t *part = d.part + c0 * d.P * 16;
    if (launch_ghash_bulk(cipher, nc, stride, ct_bytes, d.aad + 64 * c0, aad_len, pow, part, s) != hipSuccess ||
        launch_ghash_finish(const_cast<uint8_t *>(cipher), nc, stride, ct_bytes, aad_len, d.sub + 32 * c0,
                            pow, part, false, fail + c0, status, s) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    return FLTEE_SUCCESS;
}

// g (fltee_set_upload_aead): bpc is the slice stride B + 16; every chunk is authenticated
// next to its decryption, and the word gathering FLTEE_DEV_ERR_AUTH is read at the
// synchronisation that ends the decryption: FLTEE_ERROR_MAC_MISMATCH.  verdict (with g; the
// REPORT / DROP policies): that one readback also takes the n fail words in front of the
// word — (n + 1) * 4 bytes, a function of n alone — into verdict[0 .. n].
static uint32_t load_and_decrypt(DeviceCtx *c, const uint32_t *ids, size_t n, const uint8_t *enc,
                                 size_t bpc, float *t_load, float *t_dec, const GcmArgs *g = nullptr,
                                 std::vector<uint32_t> *verdict = nullptr) {
    const size_t ctb = g ? bpc - FLTEE_GCM_TAG_BYTES : bpc;
    const size_t rpc = ctb / 8;
    const double t0 = now_s();
    if (!c->cipher.reserve(n * bpc) || !c->records.reserve(n * rpc * 8) ||
        !c->round_keys.reserve(n * 44 * 4))
        return FLTEE_ERROR_OUT_OF_MEMORY;
    std::vector<uint32_t> rk;
    std::vector<uint8_t> ghost;
    GcmDev gd = {};
    uint32_t auth = 0;
    if (g) {
        if (uint32_t st = gcm_prepare(c, ids, n, ctb, g->iv, g->aad.data(), g->aad_len, ghost, c->stream, gd))
            return st;
        if (fl_memset_async(gd.auth_word, 0, 4, c->stream) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    } else {
        client_round_keys(ids, n, rk);
        if (fl_memcpy_async(c->round_keys.ptr, rk.data(), rk.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return FLTEE_ERROR_UNEXPECTED;
    }
    size_t per = bpc ? kLoadChunkBytes / bpc : n;
    if (per == 0) per = 1;
    if ((n + per - 1) / per > (size_t)DeviceCtx::kCopyEvents) per = (n + DeviceCtx::kCopyEvents - 1) / DeviceCtx::kCopyEvents;
    const uint8_t *cipher = (const uint8_t *)c->cipher.ptr;
    int ev = 0;
    for (size_t c0 = 0; c0 < n && bpc; c0 += per, ++ev) {
        const size_t nc = c0 + per < n ? per : n - c0;
        if (fl_memcpy_async((uint8_t *)c->cipher.ptr + c0 * bpc, enc + c0 * bpc, nc * bpc,
                           hipMemcpyHostToDevice, c->copy_stream) != hipSuccess ||
            hipEventRecord(c->copy_ev[ev], c->copy_stream) != hipSuccess ||
            hipStreamWaitEvent(c->stream, c->copy_ev[ev], 0) != hipSuccess)
            return FLTEE_ERROR_UNEXPECTED;
        if (g) {
            if (launch_aes_ctr_gcm(cipher + c0 * bpc, nc, bpc, rpc, gd.rk + c0 * 44,
                                   (uint8_t *)c->records.ptr + c0 * rpc * 8, rpc * 8, g->iv,
                                   c->stream) != hipSuccess ||
                gcm_verify(gd, c0, nc, cipher + c0 * bpc, ctb, g->aad_len, gd.fail, gd.auth_word, c->stream))
                return FLTEE_ERROR_UNEXPECTED;
            continue;
        }
        if (launch_aes_ctr(cipher + c0 * bpc, nc, bpc, rpc, (const uint32_t *)c->round_keys.ptr + c0 * 44,
                           (uint8_t *)c->records.ptr + c0 * rpc * 8, c->stream) != hipSuccess)
            return FLTEE_ERROR_UNEXPECTED;
    }
    if (fl_stream_sync(c->copy_stream) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    const double t1 = now_s();
    if (t_load) *t_load = (float)(t1 - t0);
    if (g && verdict) {
        verdict->assign(n + 1, 0);
        if (fl_memcpy_async(verdict->data(), gd.fail, (n + 1) * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            return FLTEE_ERROR_UNEXPECTED;
    } else if (g && fl_memcpy_async(&auth, gd.auth_word, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        return FLTEE_ERROR_UNEXPECTED;
    }
    // rk lives on this stack frame: the decrypt (and the key upload) must finish here
    if (fl_stream_sync(c->stream) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    if (t_dec) *t_dec = (float)(now_s() - t1);
    if (g && verdict) auth = (*verdict)[n];
    return auth ? FLTEE_ERROR_MAC_MISMATCH : FLTEE_SUCCESS;
}

static uint32_t read_status(DeviceCtx *c, uint32_t *st) {
    if (fl_memcpy_async(st, c->status, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        fl_stream_sync(c->stream) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    return FLTEE_SUCCESS;
}

// This ECALL's path_oram takes the tree Path ORAM (fltee_set_path_oram_tree; a shape past
// the tree's bounds, which aggregate() would refuse, takes the sweep)
static bool ecall_takes_tree(uint32_t alg, size_t n, size_t rpc, size_t d) {
    return alg == FLTEE_ALG_PATH_ORAM && oram_tree_default() && oram_fits(n * rpc, d, false);
}

// The options aggregate_records gives aggregate() for an ECALL's alg (shared with the
// staged path below).
// rpc: the records per client the aggregate sees (a packed, bf16 or fp8 call: d); fmt: c->records
// holds value-only slices — FLTEE_OPT_PACKED, FLTEE_OPT_BF16 or FLTEE_OPT_FP8, 0 for records
// trim: the call's trim count under fltee_set_dense_trim (0: an untrimmed call)
static EngineOpts ecall_opts(uint32_t alg, size_t n, size_t rpc, size_t d, size_t k_req,
                                    size_t batch, uint64_t seed, uint32_t fmt = 0, size_t trim = 0) {
    EngineOpts o;
    std::memset(&o, 0, sizeof o);
    o.k_req = k_req;
    o.flags |= FLTEE_OPT_K_REQ;
    o.batch = batch;
    const bool flat = alg == FLTEE_ALG_BASELINE || alg == FLTEE_ALG_PATH_ORAM ||
                      alg == FLTEE_ALG_NON_OBLIVIOUS;
    if (flat && rpc == d) o.flags |= FLTEE_OPT_DENSE;
    o.flags |= fmt;
    if (trim) o.flags |= FLTEE_OPT_TRIM, o.trim = trim;
    // (t past the lists reaches here only under fltee_set_dense_trim_select: refused before otherwise)
    if (trim > FLTEE_TRIM_MAX) o.flags |= FLTEE_OPT_TRIM_SELECT;
    // (fltee_set_dense_krum: every call carries the flag, and the plan refuses what is not a dense
    // call of a flat alg with n >= 2 f + 3, m <= n - f — never a plain mean)
    if (dense_krum_on()) o.flags |= FLTEE_OPT_KRUM, o.krum_f = g_dense_krum_f, o.krum_m = g_dense_krum_m;
    // (fltee_set_dense_gmed likewise: the plan refuses what is not a dense call of a flat alg)
    if (dense_gmed_on()) o.flags |= FLTEE_OPT_GMED, o.gmed_iters = g_dense_gmed_iters, o.gmed_nu = g_dense_gmed_nu;
    if (ecall_takes_tree(alg, n, rpc, d)) o.flags |= FLTEE_OPT_ORAM_TREE;
    if (alg == FLTEE_ALG_NIPS19) o.seed = seed ? seed : next_seed();
    // advanced's fold (advanced.rs:66-101) runs once with halo = n: bit for bit for every
    // run of up to n + 1 entries — every upload whose clients each send distinct indices
    // (n records + the initial entry) — and a run of more (some client repeated an index)
    // is finished by the fold's long-run carry in the same fixed-cost sequence (round 6,
    // k_fold.hip / k_compact.hip), its sum re-associated at the walk boundaries.  With the
    // exact-runs policy the halo is the public worst case (every record one index): one
    // sequential walk, bit for bit for any run.  Either way the cost is fixed by the
    // public sizes; no data-dependent relaunch.
    o.fold_halo = exact_runs_default() ? n * rpc + d : n;
    return o;
}

// What an ECALL returns for the device status word of one aggregate (aggregate_records'
// rules); *retry: a dense-sized upload out of position, to rerun sparse.
static uint32_t status_to_retval(uint32_t dev_st, uint32_t alg, bool *retry) {
    *retry = false;
    if (dev_st == 0) return FLTEE_SUCCESS;
    if (dev_st & FLTEE_DEV_ERR_INDEX_RANGE) return FLTEE_ERROR_INVALID_PARAMETER;
    if (dev_st & FLTEE_DEV_ERR_ORAM_STASH) return FLTEE_ERROR_UNEXPECTED;
    if (dev_st & FLTEE_DEV_ERR_DENSE_ORDER) {
        // a dense-sized upload (k = d) with a record out of position — not serialize_dense's
        // layout, e.g. fl_main.py --alpha 1.0, whose top-k orders the records by |val|.
        // Every flat alg reruns it sparse, with the reference's result for any upload:
        // non_oblivious by its scatter / ordered fold, baseline and path_oram by the
        // ordered fold in the composite-key network's order (engine.hip flat_ordered,
        // baseline.rs:28-60's upload order).  The rerun follows the upload's layout (one
        // bit: in position or not, the same for every round of a given client code), not
        // its values.
        (void)alg;
        *retry = true;
        return FLTEE_SUCCESS;
    }
    return FLTEE_ERROR_UNEXPECTED;
}

// Aggregate c->records (n clients x rpc records) with alg into the device out buffer,
// reading the status word back (one sync) and rerunning only where status_to_retval says.
// rec: the records when they are not c->records (the survivors of a DROP call).
static uint32_t aggregate_records(DeviceCtx *c, uint32_t alg, size_t n, size_t rpc, size_t d,
                                  size_t k_req, size_t batch, float *d_out, uint64_t seed = 0,
                                  const void *rec = nullptr, uint32_t fmt = 0, size_t trim = 0) {
    EngineOpts o = ecall_opts(alg, n, rpc, d, k_req, batch, seed, fmt, trim);
    if (alg == FLTEE_ALG_OPTIMIZED) o.flags &= ~FLTEE_OPT_K_REQ;
    if (!rec) rec = c->records.ptr;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (fl_memset_async(c->status, 0, 4, c->stream) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
        uint32_t st = aggregate(alg, rec, n, rpc, d, d_out, o, c->stream, c->status);
        if (st != FLTEE_SUCCESS) return st;
        uint32_t dev_st = 0;
        if (read_status(c, &dev_st)) return FLTEE_ERROR_UNEXPECTED;
        bool retry = false;
        st = status_to_retval(dev_st, alg, &retry);
        if (!retry) return st;
        // (under fltee_set_dense_trim / _krum / _gmed a sparse rerun would be a plain mean: refused)
        if (g_dense_trim || dense_krum_on() || dense_gmed_on()) return FLTEE_ERROR_INVALID_PARAMETER;
        o.flags &= ~FLTEE_OPT_DENSE;  // the sparse path: exact for any upload
    }
    return FLTEE_ERROR_INVALID_PARAMETER;
}

// FLTEE_AEAD_DROP after a failing verdict (fail[0 .. n) from load_and_decrypt): S = the
// verified clients in upload order, n' = |S|.  Below the quorum the call ends as under ABORT
// (FLTEE_ERROR_MAC_MISMATCH).  Otherwise c->records (n x rpc) is compacted into c->survivors
// (k_survivors.hip; reserved here, on the failure path only) and *rec / *n_keep say what to
// aggregate.  The keep list goes up asynchronously on the call's stream, from c->keep_host;
// nothing here synchronises.  Launch shapes: the public sizes and the failed set.  (The
// indices are the host's own, all < n: the kernel's range flag cannot be raised here.)
static uint32_t gather_survivors(DeviceCtx *c, const std::vector<uint32_t> &fail, size_t n, size_t rpc,
                                 size_t *n_keep, const void **rec) {
    std::vector<uint32_t> &keep = c->keep_host;
    keep.clear();
    for (size_t i = 0; i < n; ++i)
        if (!fail[i]) keep.push_back((uint32_t)i);
    const size_t ns = keep.size();
    if (ns < g_aead_min_survivors || ns == 0) return FLTEE_ERROR_MAC_MISMATCH;
    *n_keep = ns;
    if (ns == n) return FLTEE_SUCCESS;
    if (!gather_clients_fits(n, rpc, ns)) return FLTEE_ERROR_MAC_MISMATCH;  // past the gather's grid
    const size_t recb = (ns * rpc * 8 + 15) / 16 * 16;
    if (!c->survivors.reserve(recb + ns * 4)) return FLTEE_ERROR_OUT_OF_MEMORY;
    uint32_t *d_keep = (uint32_t *)((uint8_t *)c->survivors.ptr + recb);
    if (fl_memcpy_async(d_keep, keep.data(), ns * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        launch_gather_clients(c->records.ptr, n, rpc, d_keep, ns, c->survivors.ptr, c->status,
                              c->stream) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    *rec = c->survivors.ptr;
    return FLTEE_SUCCESS;
}

// Small calls (payload <= kStagedBytes) on one GPU with ONE host synchronisation. The
// round keys are computed straight into pinned memory and read from there by the AES-CTR
// kernel (which also zeroes the status word); the ciphertext is read the same way up to
// kZeroCopyBytes (one host memcpy into the pinned buffer; the kernel issues its loads
// before its rounds), and above that crosses in one DMA straight from the caller's
// buffer (the runtime's pageable path pipelines its own staging: 1.2 MB in 47 us against
// 67 us through a memcpy into our pinned buffer + a DMA, `profiles/r05/small_ecall/
// h2d_probe_r05l.jsonl`).  The aggregation follows on the stream, and the f32[d] output
// leaves with the device status word (it sits right after the output in HBM) through a
// copy kernel storing into pinned memory — then one stream sync.  The runtime's copy
// commands started ~10 us after the command before them in the kernel traces of small
// calls (`profiles/r05/small_ecall/`), so the small path avoids them.  The large-payload
// path (pageable 64 MB chunks with the decryption pipelined under the copies) pays a
// stream sync per phase.  Timers (execution_time_results, lib.rs:280-353): [0] = the
// host staging + the H2D (when there is one), [1] = the AES kernel (hipEvents), [2] =
// the rest of the call (alg 6: [1] = decrypt + aggregate, [2] = 0, lib.rs:425-592).
// alg: an ECALL alg, or FLTEE_ALG_OPTIMIZED with batch.
constexpr size_t kStagedBytes = (size_t)16 << 20;
constexpr size_t kZeroCopyBytes = (size_t)256 << 10;

__global__ __launch_bounds__(256) void copy_out_kernel(const uint4 *__restrict__ src,
                                                       uint4 *__restrict__ dst, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256)
        dst[i] = src[i];
}

static hipError_t launch_copy_out(const void *src, void *dst, size_t bytes, hipStream_t s) {
    const size_t n16 = (bytes + 15) / 16;  // both ends 16-B aligned, padded
    size_t blocks = (n16 + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    FLTEE_LAUNCH(copy_out_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const uint4 *)src,
                       (uint4 *)dst, n16);
    return hipGetLastError();
}

static uint32_t staged_ecall(DeviceCtx *c, uint32_t alg, const uint32_t *ids, size_t n,
                             const uint8_t *enc, size_t bpc, size_t d, size_t k_req, size_t batch,
                             uint64_t seed, const FLConfig &cfg, float *host_out, float *times,
                             uint32_t fmt = 0, size_t trim = 0) {
    const double t0 = now_s();
    const size_t rpc = bpc / 8;                // 8-byte units per client as decrypted
    const size_t rpa = fmt ? d : rpc;          // records per client as aggregated
    const size_t rkb = (n * 44 * 4 + 15) / 16 * 16, cb = n * bpc;
    const size_t d4 = (d * 4 + 15) / 16 * 16;
    const bool zero_copy = 16 + rkb + cb <= kZeroCopyBytes;
    // device [out: d4][status: 16][ciphertext: cb, DMA only]; pinned in [16][round keys:
    // rkb][ciphertext: cb, zero-copy only], pinned out [out: d4][status: 16]
    if (!c->stage.reserve(d4 + 16 + (zero_copy ? 0 : cb) + 16) ||
        !c->records.reserve(n * rpc * 8 + 16) ||
        !c->pin_in.reserve(16 + rkb + (zero_copy ? cb : 0) + 16) || !c->pin_out.reserve(d4 + 16))
        return FLTEE_ERROR_OUT_OF_MEMORY;
    for (int i = 0; i < 3; ++i)
        if (!c->call_ev[i] && hipEventCreate(&c->call_ev[i]) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
    uint8_t *pin = (uint8_t *)c->pin_in.ptr;
    aes128_session_round_keys(ids, n, (uint32_t *)(pin + 16));  // session_key_store.rs:21-22
    if (cb && zero_copy) std::memcpy(pin + 16 + rkb, enc, cb);
    const double t1 = now_s();  // host staging done; the DMA (if any) is timed by events
    hipStream_t s = c->stream;
    uint8_t *stage = (uint8_t *)c->stage.ptr;
    float *d_out = (float *)stage;
    uint32_t *d_st = (uint32_t *)(stage + d4);
    const uint32_t *d_rk = (const uint32_t *)((const uint8_t *)c->pin_in.dptr + 16);
    const uint8_t *d_cipher = zero_copy ? (const uint8_t *)d_rk + rkb : stage + d4 + 16;
    // (no H2D to time on the zero-copy path: no marker in front of the first kernel)
    if ((!zero_copy && hipEventRecord(c->call_ev[0], s) != hipSuccess) ||
        (!zero_copy && fl_memcpy_async(stage + d4 + 16, enc, cb, hipMemcpyHostToDevice, s) != hipSuccess) ||
        (!cb && fl_memset_async(d_st, 0, 4, s) != hipSuccess))
        return FLTEE_ERROR_UNEXPECTED;
    EngineOpts o = ecall_opts(alg == FLTEE_ALG_OPTIMIZED ? FLTEE_ALG_ADVANCED : alg, n, rpa, d,
                                     k_req, batch, seed, fmt, trim);
    if (alg == FLTEE_ALG_OPTIMIZED) o.flags &= ~FLTEE_OPT_K_REQ;
    // the call's device work: AES (timed by events) -> aggregation (-> DP) -> copy-out
    auto enqueue = [&](bool retry_pass) -> uint32_t {
        if (retry_pass && fl_memset_async(d_st, 0, 4, s) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
        if (!retry_pass &&
            (hipEventRecord(c->call_ev[1], s) != hipSuccess ||
             (cb && launch_aes_ctr(d_cipher, n, bpc, rpc, d_rk, (uint8_t *)c->records.ptr, s, d_st) !=
                        hipSuccess) ||
             hipEventRecord(c->call_ev[2], s) != hipSuccess))
            return FLTEE_ERROR_UNEXPECTED;
        const uint32_t a = aggregate(alg, c->records.ptr, n, rpa, d, d_out, o, s, d_st);
        if (a != FLTEE_SUCCESS) return a;
        if (cfg.dp && launch_dp_noise(d_out, d, cfg.sigma, cfg.clipping, dense_krum_on() ? g_dense_krum_m : n - 2 * trim,
                                      next_seed(), s) != hipSuccess)
            return FLTEE_ERROR_UNEXPECTED;
        return launch_copy_out(d_out, c->pin_out.dptr, d4 + 16, s) == hipSuccess
                   ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
    };
    // (Round 5, measured and not kept: this device work captured once per call shape as a
    // graph and replayed with one launch — MLP-MNIST n = 3 `advanced` 99-119 vs 101-110 us
    // per call: the replay still dispatches kernel by kernel, `profiles/r05/small_ecall/
    // graph_replay_r05g2.jsonl`.)
    uint32_t st = FLTEE_SUCCESS;
    for (int attempt = 0; attempt < 2; ++attempt) {
        st = enqueue(attempt > 0);
        if (st != FLTEE_SUCCESS) return st;
        if (fl_stream_sync(s) != hipSuccess) return FLTEE_ERROR_UNEXPECTED;
        bool retry = false;
        st = status_to_retval(*(const volatile uint32_t *)((const uint8_t *)c->pin_out.ptr + d4), alg,
                              &retry);
        if (!retry) break;
        // (under fltee_set_dense_trim / _krum / _gmed a sparse rerun would be a plain mean: refused)
        if (g_dense_trim || dense_krum_on() || dense_gmed_on()) return FLTEE_ERROR_INVALID_PARAMETER;
        o.flags &= ~FLTEE_OPT_DENSE;  // the sparse path: exact for any upload
    }
    if (st) return st;
    std::memcpy(host_out, c->pin_out.ptr, d * 4);
    float h2d = 0, aes = 0;
    if (!zero_copy) (void)hipEventElapsedTime(&h2d, c->call_ev[0], c->call_ev[1]);
    (void)hipEventElapsedTime(&aes, c->call_ev[1], c->call_ev[2]);
    const float wall = (float)(now_s() - t0);
    times[0] = (float)(t1 - t0) + h2d * 1e-3f;
    times[1] = aes * 1e-3f;
    times[2] = wall - times[0] - times[1];
    if (alg == FLTEE_ALG_OPTIMIZED) {
        times[1] += times[2];
        times[2] = 0;
    }
    return FLTEE_SUCCESS;
}

}  // namespace fltee

using namespace fltee;

// fltee_version(): build/version.cpp, generated by the Makefile (source hash + tune flags)

extern "C" fltee_status_t fltee_device_init(int hip_device, fltee_eid_t *eid) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    if (!eid) return FLTEE_ERROR_INVALID_PARAMETER;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || hip_device < 0 || hip_device >= count)
        return FLTEE_ERROR_UNEXPECTED;
    if (hipSetDevice(hip_device) != hipSuccess || !device_ctx(hip_device)) return FLTEE_ERROR_UNEXPECTED;
    g_eid_dev.push_back(hip_device);
    *eid = (fltee_eid_t)g_eid_dev.size();
    return FLTEE_SUCCESS;
}

extern "C" fltee_status_t fltee_device_init_multi(const int *hip_devices, int n, fltee_eid_t *eid) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    if (!eid || !hip_devices) return FLTEE_ERROR_INVALID_PARAMETER;
    uint32_t st = 0;
    Group *G = group_create(hip_devices, n, &st);
    if (!G) return st;
    if (hipSetDevice(hip_devices[0]) != hipSuccess || !device_ctx(hip_devices[0])) {
        group_destroy(G);
        return FLTEE_ERROR_UNEXPECTED;
    }
    g_eid_dev.push_back(hip_devices[0]);
    *eid = (fltee_eid_t)g_eid_dev.size();
    g_groups[*eid] = G;
    return FLTEE_SUCCESS;
}

extern "C" int fltee_device_count(fltee_eid_t eid) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    if (eid == 0 || eid > g_eid_dev.size() || g_eid_dev[eid - 1] < 0) return 0;
    Group *G = group_of(eid);
    return G ? group_size(G) : 1;
}

extern "C" fltee_status_t fltee_device_fini(fltee_eid_t eid) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    if (eid == 0 || eid > g_eid_dev.size() || g_eid_dev[eid - 1] < 0) return FLTEE_ERROR_INVALID_ENCLAVE_ID;
    const int dev = g_eid_dev[eid - 1];
    g_eid_dev[eid - 1] = -1;
    if (Group *G = group_of(eid)) {
        group_destroy(G);
        g_groups.erase(eid);
    }
    if (hipSetDevice(dev) == hipSuccess) (void)fl_device_sync();
    return FLTEE_SUCCESS;
}

// lib.rs:113-180
extern "C" fltee_status_t ecall_fl_init(fltee_eid_t eid, fltee_status_t *retval, uint32_t fl_id,
                                        const uint32_t *client_ids, size_t client_size,
                                        size_t num_of_parameters, size_t num_of_sparse_parameters,
                                        float sigma, float clipping, float alpha,
                                        float sampling_ratio, uint32_t aggregation_alg,
                                        uint8_t verbose, uint8_t dp) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    if (eid == 0 || eid > g_eid_dev.size() || g_eid_dev[eid - 1] < 0) return FLTEE_ERROR_INVALID_ENCLAVE_ID;
    if (!retval) return FLTEE_ERROR_INVALID_PARAMETER;
    FLConfig cfg;
    cfg.client_ids.assign(client_ids, client_ids + client_size);
    cfg.d = num_of_parameters;
    cfg.k = num_of_sparse_parameters;
    cfg.sigma = sigma;
    cfg.clipping = clipping;
    cfg.alpha = alpha;
    cfg.ratio = sampling_ratio;
    cfg.alg = aggregation_alg;
    cfg.verbose = verbose;
    cfg.dp = dp;
    cfg.round = 0;
    if (!g_have_keys && verbose) std::printf("[FLTEE] remote attestation mock\n");
    for (size_t i = 0; i < client_size; ++i) g_keys.insert(client_ids[i]);  // lib.rs:163-174
    g_have_keys = true;
    g_cfg[fl_id] = std::move(cfg);
    g_auth_reports.erase(fl_id);  // a verdict belongs to the config it was read under
    if (verbose) std::printf("[FLTEE] make fl config id %u\n", fl_id);
    *retval = FLTEE_SUCCESS;
    return FLTEE_SUCCESS;
}

// lib.rs:182-219
extern "C" fltee_status_t ecall_start_round(fltee_eid_t eid, fltee_status_t *retval, uint32_t fl_id,
                                            uint32_t round, size_t sample_size,
                                            uint32_t *sampled_client_ids) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    if (eid == 0 || eid > g_eid_dev.size() || g_eid_dev[eid - 1] < 0) return FLTEE_ERROR_INVALID_ENCLAVE_ID;
    if (!retval) return FLTEE_ERROR_INVALID_PARAMETER;
    auto it = g_cfg.find(fl_id);
    if (it == g_cfg.end()) { *retval = FLTEE_ERROR_UNEXPECTED; return FLTEE_SUCCESS; }
    FLConfig &cfg = it->second;
    if (cfg.round != round) { *retval = FLTEE_ERROR_INVALID_PARAMETER; return FLTEE_SUCCESS; }
    std::memset(sampled_client_ids, 0, sample_size * 4);  // [out] zero-fill
    const size_t calc = f32_to_usize_sat((float)cfg.client_ids.size() * cfg.ratio);
    if (calc != sample_size) { *retval = FLTEE_ERROR_INVALID_PARAMETER; return FLTEE_SUCCESS; }
    std::vector<uint32_t> sampled;
    sample_client_ids(cfg.client_ids, calc, next_seed(), sampled);
    std::copy(sampled.begin(), sampled.end(), sampled_client_ids);
    cfg.sampled = std::set<uint32_t>(sampled.begin(), sampled.end());
    if (cfg.verbose)
        std::printf("[FLTEE] sampling for round %u is done and store %zu/%zu client ids.\n", round,
                    sample_size, cfg.client_ids.size());
    *retval = FLTEE_SUCCESS;
    return FLTEE_SUCCESS;
}

// lib.rs:221-423
extern "C" fltee_status_t ecall_secure_aggregation(
    fltee_eid_t eid, fltee_status_t *retval, uint32_t fl_id, uint32_t round,
    const uint32_t *client_ids, size_t client_size, const uint8_t *encrypted_parameters_data,
    size_t encrypted_parameters_size, size_t num_of_parameters, size_t num_of_sparse_parameters,
    uint32_t aggregation_alg, float *updated_parameters_data, float *execution_time_results) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    if (!retval) return FLTEE_ERROR_INVALID_PARAMETER;
    DeviceCtx *c = eid_ctx(eid);
    if (!c) return FLTEE_ERROR_INVALID_ENCLAVE_ID;
    const size_t d = num_of_parameters;
    // Enclave_t.c:626 zero-fills [out]: every successful path writes all of it, so the
    // zeros are written where a call fails (200 KB at MLP-MNIST: ~10 us saved per call)
    std::memset(execution_time_results, 0, 3 * sizeof(float));
    auto fail = [&](uint32_t st) {
        std::memset(updated_parameters_data, 0, d * sizeof(float));
        *retval = st;
        return FLTEE_SUCCESS;
    };
    auto it = g_cfg.find(fl_id);
    if (it == g_cfg.end()) return fail(FLTEE_ERROR_UNEXPECTED);
    FLConfig &cfg = it->second;
    if (cfg.round != round || cfg.alg != aggregation_alg) return fail(FLTEE_ERROR_INVALID_PARAMETER);
    const size_t n = client_size;
    if (n == 0) return fail(FLTEE_ERROR_INVALID_PARAMETER);  // lib.rs:305 would divide by zero
    if (uint32_t st = check_uploaded(cfg, client_ids, n)) return fail(st);
    for (size_t i = 0; i < n; ++i)
        if (!g_keys.count(client_ids[i])) return fail(FLTEE_ERROR_UNEXPECTED);  // lib.rs:319-322
    // lib.rs:359-397: 6 is not dispatched here (panic); 7 is bubble_sort_based (lib.rs:389),
    // answered by the stable network (k_stable.hip) with the enclave's in-order result once
    // the host has opted in (fltee_set_bubble_ecall(1)); until then it stays the 0x2 that
    // hosts of earlier versions get for it
    switch (aggregation_alg) {
    case FLTEE_ALG_ADVANCED: case FLTEE_ALG_NIPS19: case FLTEE_ALG_BASELINE:
    case FLTEE_ALG_NON_OBLIVIOUS: case FLTEE_ALG_PATH_ORAM: break;
    case FLTEE_ALG_BUBBLE:
        if (bubble_ecall_default()) break;
        [[fallthrough]];
    default: return fail(FLTEE_ERROR_INVALID_PARAMETER);
    }
    // lib.rs:305-306: bytes per client floored, records per client floored; slice i
    // starts at i*bpc even when that is not a record boundary (ragged payloads)
    // with authenticated uploads (fltee_set_upload_aead) a slice is B bytes || a 16-byte tag:
    // bpc is the stride B + 16, the records are B's, and the payload is n whole slices
    const bool aead = g_upload_aead;
    const size_t bpc = encrypted_parameters_size / n;
    if (aead && (bpc < FLTEE_GCM_TAG_BYTES || encrypted_parameters_size % n ||
                 !gcm_sizes_ok(bpc - FLTEE_GCM_TAG_BYTES, 16)))
        return fail(FLTEE_ERROR_INVALID_PARAMETER);
    const size_t ctb = aead ? bpc - FLTEE_GCM_TAG_BYTES : bpc;
    // value-only slices (fltee_set_upload_packed, _bf16, _fp8): loaded, decrypted,
    // verified and gathered as rpc = row_units 8-byte units per client, aggregated as rpa = d
    // records
    const UploadFmt uf = upload_format(g_upload_packed, g_upload_bf16, g_upload_fp8, d, num_of_sparse_parameters,
                                       encrypted_parameters_size % n ? 0 : ctb);
    const uint32_t fmt = uf.opt;
    const bool packed = fmt == FLTEE_OPT_PACKED, bf16 = fmt == FLTEE_OPT_BF16, fp8 = fmt == FLTEE_OPT_FP8;
    const size_t rpc = ctb / 8;
    const size_t rpa = fmt ? d : rpc;
    GcmArgs gcm;
    if (aead)
        ecall_gcm_args(fl_id, round, client_ids, n, aggregation_alg | uf.aad_bit, gcm);
    if ((aggregation_alg == FLTEE_ALG_ADVANCED || aggregation_alg == FLTEE_ALG_BUBBLE) &&
        n * num_of_sparse_parameters > n * rpa)
        return fail(FLTEE_ERROR_INVALID_PARAMETER);  // advanced.rs:72 out-of-bounds panic
    const bool flat = aggregation_alg == FLTEE_ALG_BASELINE || aggregation_alg == FLTEE_ALG_PATH_ORAM ||
                      aggregation_alg == FLTEE_ALG_NON_OBLIVIOUS;
    // robust aggregation (fltee_set_dense_trim): only a call that takes the dense or the packed
    // accumulate can be trimmed (a bf16 or fp8 call: the records trim on its unpacked copy); a host
    // that switched trimming on never gets an untrimmed
    // mean back from any other — the sort-based algs, a sparse upload, the tree, a trim count
    // past the kernel's lists (evaluated on the request as sent: n' <= n trims no more) unless
    // fltee_set_dense_trim_select answers it by selection, n <= FLTEE_TRIM_SELECT_MAX_N
    const uint32_t trim_pm = g_dense_trim;
    if (trim_pm && (!flat || !(fmt || rpc == d) || (aggregation_alg == FLTEE_ALG_PATH_ORAM && oram_tree_default()) ||
                    (trim_count(n, trim_pm) > FLTEE_TRIM_MAX &&
                     (!g_dense_trim_select || n > FLTEE_TRIM_SELECT_MAX_N))))
        return fail(FLTEE_ERROR_INVALID_PARAMETER);
    // Multi-Krum (fltee_set_dense_krum): likewise only a call on the dense path, never together
    // with the trim, and never a plain mean — evaluated on the request as sent (n' <= n keeps no
    // more); what depends on n' is the plan's refusal of the aggregate call itself
    const bool krum_on = dense_krum_on();
    if (krum_on && (!flat || !(fmt || rpc == d) || (aggregation_alg == FLTEE_ALG_PATH_ORAM && oram_tree_default()) ||
                    trim_pm || n > FLTEE_KRUM_MAX_N || n < 2 * (size_t)g_dense_krum_f + 3 || g_dense_krum_m == 0 ||
                    g_dense_krum_m > n - g_dense_krum_f))
        return fail(FLTEE_ERROR_INVALID_PARAMETER);
    // the geometric median (fltee_set_dense_gmed): likewise, and never together with the trim or
    // Multi-Krum
    const bool gmed_on = dense_gmed_on();
    if (gmed_on && (!flat || !(fmt || rpc == d) || (aggregation_alg == FLTEE_ALG_PATH_ORAM && oram_tree_default()) ||
                    trim_pm || krum_on || n > FLTEE_KRUM_MAX_N || g_dense_gmed_iters > FLTEE_GMED_MAX_ITERS ||
                    !(g_dense_gmed_nu > 0.0) || !(g_dense_gmed_nu < __builtin_inf())))
        return fail(FLTEE_ERROR_INVALID_PARAMETER);

    if (!c->outbuf.reserve(d * 4 + 16)) return fail(FLTEE_ERROR_OUT_OF_MEMORY);
    float *d_out = (float *)c->outbuf.ptr;
    const size_t k_req = num_of_sparse_parameters;
    const float coef = 1.0f / (float)n;
    Group *G = group_of(eid);
    // an authenticated upload over a multi-GPU eid: the call's keys, computed once on the host
    // (round keys, H || E_K(J0), the AAD padded), for the ranks that verify their shards
    std::vector<uint8_t> gkeys;
    GcmHost gh;
    if (G && aead) {
        gcm_host_keys(client_ids, n, gcm.iv, gcm.aad.data(), gcm.aad_len, gkeys);
        gh.sub = gkeys.data() + n * 44 * 4;
        gh.aad64 = gh.sub + n * 32;
        gh.iv = gcm.iv;
        gh.aad_len = gcm.aad_len;
    }
    const size_t tagb = aead ? FLTEE_GCM_TAG_BYTES : 0;
    uint32_t st = FLTEE_GROUP_FALLBACK;
    double t2 = 0;
    // REPORT / DROP: the per-client verdict is kept.  A group path that read a failing verdict
    // stopped before any aggregation launch, as under ABORT; the call then continues on the
    // root alone (below), which loads and verifies the whole payload again for the fail words
    const bool keepv = keeps_verdict(aead);
    bool verdict_stored = false;
    bool group_tried = false;  // a shape the group declined (or failed on) is not offered to it again
    const bool tree = ecall_takes_tree(aggregation_alg, n, rpa, d);
    // (a packed, bf16 or fp8 call is loaded on the root: the dense group path shards records by
    // column, under the robust switches too)
    // Under fltee_set_dense_trim / _krum / _gmed the ranks aggregate their columns by the call's
    // one-GPU route: a trimmed column needs no other; Multi-Krum and the geometric median share one
    // Gram matrix, added up over the ranks in the one-GPU order, and the root's selection on it.
    // The refusals above came first, and what the root's plan would still refuse (a shape past
    // the 32-bit positions) is left to the root; n' = n in the group (a failing verdict under
    // REPORT / DROP leaves for the root below)
    GroupRobust rb;
    if (const size_t t = trim_count(n, trim_pm))
        rb.kind = t > FLTEE_TRIM_MAX ? GroupRobust::kTrimSelect : GroupRobust::kTrim, rb.trim = t;
    if (krum_on) rb.kind = GroupRobust::kKrum, rb.krum_f = g_dense_krum_f, rb.krum_m = g_dense_krum_m;
    if (gmed_on) rb.kind = GroupRobust::kGmed, rb.gmed_iters = g_dense_gmed_iters, rb.gmed_nu = g_dense_gmed_nu;
    // aggregate()'s divisor: the n - 2 t clients a trimmed mean keeps, Multi-Krum's m (the
    // geometric median's weights sum to one: its accumulate takes no factor)
    const float group_coef = rb.trim ? 1.0f / (float)(n - 2 * rb.trim) : krum_on ? 1.0f / (float)g_dense_krum_m : coef;
    if (G && flat && !tree && !fmt && rpc == d && bpc == d * 8 + tagb &&
        (rb.kind == GroupRobust::kPlain ||
         plan_status(aggregation_alg, n, rpc, d,
                     ecall_opts(aggregation_alg, n, rpc, d, k_req, 0, 0, 0, trim_count(n, trim_pm))) == FLTEE_SUCCESS)) {
        // dense uploads over a multi-GPU eid: every GPU loads and decrypts its own
        // parameter range (group.hip); "Loading" = the parallel H2D, "Decryption" = the
        // decrypt + aggregate + gather.  Authenticated: every GPU also hashes its range, the
        // root merges and checks the tags before any GPU aggregates
        std::vector<uint32_t> rk;
        if (!aead) client_round_keys(client_ids, n, rk);
        st = group_dense_ecall(G, aead ? (const uint32_t *)gkeys.data() : rk.data(), n,
                               encrypted_parameters_data, d, group_coef, d_out,
                               &execution_time_results[0], &execution_time_results[1],
                               false,  // out of position: the root's sparse rerun, every alg
                               aead ? &gh : nullptr, rb);
        t2 = now_s();
        if (st == FLTEE_ERROR_MAC_MISMATCH && keepv) {
            st = FLTEE_GROUP_FALLBACK;
            group_tried = true;
        }
        if (st != FLTEE_SUCCESS && st != FLTEE_GROUP_FALLBACK) return fail(st);
    }
    // (the exact-runs policy folds on one GPU: one sequential walk of the sorted array)
    // (alg 7, once the host has opted in, shards like advanced: the same fold and tail)
    // (a bf16 or fp8 call is not sharded: the root runs it whole, the one-GPU bits)
    const bool sharded = G && !bf16 && !fp8 &&
                         (((aggregation_alg == FLTEE_ALG_ADVANCED ||
                                 (aggregation_alg == FLTEE_ALG_BUBBLE && bubble_ecall_default())) &&
                           k_req == rpa && !exact_runs_default()) ||
                          aggregation_alg == FLTEE_ALG_NIPS19);
    // nips19 draws its seed (Laplace counts, shuffle key) once per call, whichever path
    // runs it, so a multi-GPU eid consumes the seed sequence exactly as one GPU does
    const uint64_t seed = aggregation_alg == FLTEE_ALG_NIPS19 ? next_seed() : 0;
    if (st == FLTEE_GROUP_FALLBACK && sharded && !group_tried && !packed && group_splits_host_copy(G)) {
        // every GPU copies and decrypts (authenticated: and verifies) the clients of its own
        // position range
        std::vector<uint32_t> rk;
        if (!aead) client_round_keys(client_ids, n, rk);
        GroupInput in;
        in.enc = encrypted_parameters_data;
        in.rk = aead ? (const uint32_t *)gkeys.data() : rk.data();
        in.gcm = aead ? &gh : nullptr;
        in.bpc = bpc;
        in.t_load = &execution_time_results[0];
        in.t_dec = &execution_time_results[1];
        const double ta = now_s();
        if (aggregation_alg == FLTEE_ALG_ADVANCED)
            st = group_advanced(G, in, n, rpc, d, coef, d_out);
        else if (aggregation_alg == FLTEE_ALG_BUBBLE)
            st = group_bubble(G, in, n, rpc, d, coef, d_out);
        else
            st = group_nips19(G, c, in, n, rpc, k_req, d, seed, coef, d_out);
        group_tried = true;
        if (st == FLTEE_ERROR_MAC_MISMATCH && keepv) st = FLTEE_GROUP_FALLBACK;
        if (st != FLTEE_SUCCESS && st != FLTEE_GROUP_FALLBACK) return fail(st);
        // "Aggregation" = the call minus its load and decrypt phases
        t2 = ta + execution_time_results[0] + execution_time_results[1];
    }
    if (st == FLTEE_GROUP_FALLBACK && !G && !aead && n * bpc <= kStagedBytes) {
        // one GPU, a small payload: one DMA each way, one host synchronisation (an
        // authenticated upload needs the fail word before the aggregation: the path below)
        st = staged_ecall(c, aggregation_alg, client_ids, n, encrypted_parameters_data, bpc, d, k_req,
                          0, seed, cfg, updated_parameters_data, execution_time_results, fmt,
                          trim_count(n, trim_pm));
        if (st) {
            std::memset(updated_parameters_data, 0, d * sizeof(float));
            std::memset(execution_time_results, 0, 3 * sizeof(float));
            return fail(st);
        }
        if (cfg.verbose)
            std::printf("[FLTEE CLOCK] Loading %.6f Decryption %.6f Aggregation %.6f seconds\n",
                        execution_time_results[0], execution_time_results[1], execution_time_results[2]);
        cfg.round += 1;  // lib.rs:421
        *retval = FLTEE_SUCCESS;
        return FLTEE_SUCCESS;
    }
    size_t n_agg = n;  // DROP: n', the verified clients; everything that depends on n takes it
    if (st == FLTEE_GROUP_FALLBACK) {  // (a shape the per-GPU path declines comes here too)
        if (G && hipSetDevice(c->device) != hipSuccess) return fail(FLTEE_ERROR_UNEXPECTED);
        std::vector<uint32_t> verdict;
        st = load_and_decrypt(c, client_ids, n, encrypted_parameters_data, bpc,
                              &execution_time_results[0], &execution_time_results[1],
                              aead ? &gcm : nullptr, keepv ? &verdict : nullptr);
        const void *rec = nullptr;
        if (keepv && (st == FLTEE_SUCCESS || st == FLTEE_ERROR_MAC_MISMATCH)) {
            store_auth_report(fl_id, round, client_ids, n, verdict);
            verdict_stored = true;
            if (st && g_aead_policy == FLTEE_AEAD_DROP) st = gather_survivors(c, verdict, n, rpc, &n_agg, &rec);
        }
        if (st) return fail(st);  // (a tag mismatch: the timers stay written)
        t2 = now_s();
        st = FLTEE_GROUP_FALLBACK;
        GroupInput in;
        in.root_rec = (const uint64_t *)c->records.ptr;
        if (sharded && !group_tried && n_agg == n) {
            if (packed) {
                // the position-range routes shard records: the root unpacks its rows into the
                // engine's record scratch (no aggregate runs on the root before the ranks have
                // taken their ranges) and the group proceeds as after any root load
                if (!c->ws_rec.reserve(n * d * 8)) return fail(FLTEE_ERROR_OUT_OF_MEMORY);
                if (launch_unpack_rows(kRowsF32, c->records.ptr, n, d, (uint64_t *)c->ws_rec.ptr, c->stream) != hipSuccess ||
                    fl_stream_sync(c->stream) != hipSuccess)
                    return fail(FLTEE_ERROR_UNEXPECTED);
                in.root_rec = (const uint64_t *)c->ws_rec.ptr;
            }
            if (aggregation_alg == FLTEE_ALG_ADVANCED)
                st = group_advanced(G, in, n, rpa, d, coef, d_out);
            else if (aggregation_alg == FLTEE_ALG_BUBBLE)
                st = group_bubble(G, in, n, rpa, d, coef, d_out);
            else
                st = group_nips19(G, c, in, n, rpa, k_req, d, seed, coef, d_out);
        }
        if (st == FLTEE_GROUP_FALLBACK)  // one device (or a shape the group does not shard)
            st = aggregate_records(c, aggregation_alg, n_agg, rpa, d, k_req, 0, d_out, seed, rec, fmt,
                                   trim_count(n_agg, trim_pm));
    }
    if (!st && cfg.dp) {  // lib.rs:399-408 (a trimmed call: the n' - 2 t clients it averaged)
        // (a Multi-Krum call: the m clients it averaged; a geometric-median call: the n' it weighted)
        if (launch_dp_noise(d_out, d, cfg.sigma, cfg.clipping,
                            krum_on ? g_dense_krum_m : n_agg - 2 * trim_count(n_agg, trim_pm), next_seed(),
                            c->stream) != hipSuccess)
            st = FLTEE_ERROR_UNEXPECTED;
    }
    if (!st && fl_memcpy_async(updated_parameters_data, d_out, d * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        st = FLTEE_ERROR_UNEXPECTED;
    if (fl_stream_sync(c->stream) != hipSuccess) st = FLTEE_ERROR_UNEXPECTED;
    if (st) {
        std::memset(updated_parameters_data, 0, d * sizeof(float));
        return fail(st);
    }
    // (a group path answered the call: every rank's verdict was clean)
    if (keepv && !verdict_stored) store_auth_report(fl_id, round, client_ids, 0, {});
    execution_time_results[2] = (float)(now_s() - t2);
    if (cfg.verbose)
        std::printf("[FLTEE CLOCK] Loading %.6f Decryption %.6f Aggregation %.6f seconds\n",
                    execution_time_results[0], execution_time_results[1], execution_time_results[2]);
    cfg.round += 1;  // lib.rs:421
    *retval = FLTEE_SUCCESS;
    return FLTEE_SUCCESS;
}

// lib.rs:425-592
extern "C" fltee_status_t ecall_client_size_optimized_secure_aggregation(
    fltee_eid_t eid, fltee_status_t *retval, uint32_t fl_id, uint32_t round,
    size_t optimal_num_of_clients, const uint32_t *client_ids, size_t client_size,
    const uint8_t *encrypted_parameters_data_ptr, size_t num_of_parameters,
    size_t num_of_sparse_parameters, uint32_t aggregation_alg, float *updated_parameters_data,
    float *execution_time_results) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    if (!retval) return FLTEE_ERROR_INVALID_PARAMETER;
    DeviceCtx *c = eid_ctx(eid);
    if (!c) return FLTEE_ERROR_INVALID_ENCLAVE_ID;
    const size_t d = num_of_parameters, k = num_of_sparse_parameters, n = client_size;
    std::memset(execution_time_results, 0, 3 * sizeof(float));
    auto fail = [&](uint32_t st) {  // [out] zero-filled where the call fails (see above)
        std::memset(updated_parameters_data, 0, d * sizeof(float));
        *retval = st;
        return FLTEE_SUCCESS;
    };
    auto it = g_cfg.find(fl_id);
    if (it == g_cfg.end()) return fail(FLTEE_ERROR_UNEXPECTED);
    FLConfig &cfg = it->second;
    if (cfg.round != round || cfg.alg != aggregation_alg) return fail(FLTEE_ERROR_INVALID_PARAMETER);
    if (n == 0 || optimal_num_of_clients == 0) return fail(FLTEE_ERROR_INVALID_PARAMETER);
    if (uint32_t st = check_uploaded(cfg, client_ids, n)) return fail(st);
    for (size_t i = 0; i < n; ++i)
        if (!g_keys.count(client_ids[i])) return fail(FLTEE_ERROR_UNEXPECTED);
    // (fltee_set_dense_trim / _krum / _gmed: alg 6 is sort-based and cannot be trimmed, scored or
    // weighted — never a plain mean)
    if (g_dense_trim || dense_krum_on() || dense_gmed_on()) return fail(FLTEE_ERROR_INVALID_PARAMETER);

    const bool aead = g_upload_aead;
    if (aead && !gcm_sizes_ok(k * 8, 16)) return fail(FLTEE_ERROR_INVALID_PARAMETER);
    const size_t bpc6 = k * 8 + (aead ? FLTEE_GCM_TAG_BYTES : 0);  // the slice stride
    GcmArgs gcm;
    if (aead) ecall_gcm_args(fl_id, round, client_ids, n, aggregation_alg, gcm);
    float t_load = 0, t_dec = 0;
    const double t1 = now_s();
    const size_t halo6 = exact_runs_default() ? n * k + d : n;  // as aggregate_records
    float *d_out = nullptr;
    if (!c->outbuf.reserve(d * 4 + 16)) return fail(FLTEE_ERROR_OUT_OF_MEMORY);
    d_out = (float *)c->outbuf.ptr;
    uint32_t st = FLTEE_SUCCESS;
    Group *G = group_of(eid);
    // REPORT / DROP keep the per-client verdict: a group that read a failing one stopped before
    // any batch was launched, and the call continues on the root alone, which loads and
    // verifies the whole payload again for the fail words
    const bool keepv = keeps_verdict(aead);
    bool verdict_stored = false;
    bool on_root = true;  // load, verify and aggregate through the root's context
    size_t n_agg = n;     // DROP: n', the verified clients
    if (G && group_splits_host_copy(G)) {
        // the batches split over the eid's GPUs, each loading (authenticated: and verifying)
        // its own clients (group.hip)
        std::vector<uint32_t> rk;
        std::vector<uint8_t> gkeys;
        GcmHost gh;
        GroupInput in;
        if (aead) {
            gcm_host_keys(client_ids, n, gcm.iv, gcm.aad.data(), gcm.aad_len, gkeys);
            gh.sub = gkeys.data() + n * 44 * 4;
            gh.aad64 = gh.sub + n * 32;
            gh.iv = gcm.iv;
            gh.aad_len = gcm.aad_len;
            in.rk = (const uint32_t *)gkeys.data();
            in.gcm = &gh;
        } else {
            client_round_keys(client_ids, n, rk);
            in.rk = rk.data();
        }
        in.enc = encrypted_parameters_data_ptr;
        in.bpc = bpc6;
        in.t_load = &t_load;
        in.t_dec = &t_dec;
        st = group_optimized(G, in, n, k, d, optimal_num_of_clients, 1.0f / (float)n, d_out, halo6);
        execution_time_results[0] = t_load;
        if (st == FLTEE_ERROR_MAC_MISMATCH) execution_time_results[1] = t_dec;
        on_root = st == FLTEE_ERROR_MAC_MISMATCH && keepv;
    } else if (!G && !aead && n * k * 8 <= kStagedBytes) {
        // one GPU, a small payload: one DMA each way, one host synchronisation
        st = staged_ecall(c, FLTEE_ALG_OPTIMIZED, client_ids, n, encrypted_parameters_data_ptr, k * 8, d,
                          k, optimal_num_of_clients, 0, cfg, updated_parameters_data, execution_time_results);
        if (st) {
            std::memset(updated_parameters_data, 0, d * sizeof(float));
            std::memset(execution_time_results, 0, 3 * sizeof(float));
            return fail(st);
        }
        cfg.round += 1;
        *retval = FLTEE_SUCCESS;
        return FLTEE_SUCCESS;
    }
    if (on_root) {
        const bool group_failed = st == FLTEE_ERROR_MAC_MISMATCH;
        if (G && hipSetDevice(c->device) != hipSuccess) return fail(FLTEE_ERROR_UNEXPECTED);
        std::vector<uint32_t> verdict;
        st = load_and_decrypt(c, client_ids, n, encrypted_parameters_data_ptr, bpc6, &t_load, &t_dec,
                              aead ? &gcm : nullptr, keepv ? &verdict : nullptr);
        execution_time_results[0] = t_load;
        if (st == FLTEE_ERROR_MAC_MISMATCH) execution_time_results[1] = t_dec;
        const void *rec = nullptr;
        if (keepv && (st == FLTEE_SUCCESS || st == FLTEE_ERROR_MAC_MISMATCH)) {
            store_auth_report(fl_id, round, client_ids, n, verdict);
            verdict_stored = true;
            if (st && g_aead_policy == FLTEE_AEAD_DROP) st = gather_survivors(c, verdict, n, k, &n_agg, &rec);
        }
        if (st) return fail(st);
        if (G && !group_failed && n_agg == n) {
            GroupInput in;
            in.root_rec = (const uint64_t *)c->records.ptr;
            st = group_optimized(G, in, n, k, d, optimal_num_of_clients, 1.0f / (float)n, d_out, halo6);
        } else {
            st = aggregate_records(c, FLTEE_ALG_OPTIMIZED, n_agg, k, d, k, optimal_num_of_clients, d_out, 0, rec);
        }
    }
    if (!st && cfg.dp) {  // lib.rs:586-588
        if (launch_dp_noise(d_out, d, cfg.sigma, cfg.clipping, n_agg, next_seed(), c->stream) != hipSuccess)
            st = FLTEE_ERROR_UNEXPECTED;
    }
    if (!st && fl_memcpy_async(updated_parameters_data, d_out, d * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        st = FLTEE_ERROR_UNEXPECTED;
    if (fl_stream_sync(c->stream) != hipSuccess) st = FLTEE_ERROR_UNEXPECTED;
    if (st) {
        std::memset(updated_parameters_data, 0, d * sizeof(float));
        return fail(st);
    }
    if (keepv && !verdict_stored) store_auth_report(fl_id, round, client_ids, 0, {});  // (a clean group call)
    execution_time_results[1] = (float)(now_s() - t1) - t_load;  // decrypt + aggregate
    cfg.round += 1;
    *retval = FLTEE_SUCCESS;
    return FLTEE_SUCCESS;
}

// AES-128-CTR over n client slices with the session keys of lib.rs:312-343 (key
// bytes[4..8] = id BE; the client's 2-byte layout, utils.py:276-278, is the same for
// every id it can encode).  CTR is its own inverse: decrypt == encrypt.
static fltee_status_t aes_ctr_device(const uint32_t *client_ids, size_t n, const void *d_in,
                                     size_t bytes_per_client, void *d_out, hipStream_t s) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_INVALID_PARAMETER;
    if (!c->round_keys.reserve(n * 44 * 4)) return FLTEE_ERROR_OUT_OF_MEMORY;
    std::vector<uint32_t> rk(n * 44);
    aes128_session_round_keys(client_ids, n, rk.data());
    if (fl_memcpy_async(c->round_keys.ptr, rk.data(), rk.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    if (launch_aes_ctr((const uint8_t *)d_in, n, bytes_per_client, bytes_per_client / 8,
                       (const uint32_t *)c->round_keys.ptr, (uint8_t *)d_out, s) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    // rk lives on this stack frame: wait for the (tiny) copy + kernel
    return fl_stream_sync(s) == hipSuccess ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_decrypt_device(const uint32_t *client_ids, size_t n,
                                               const void *d_cipher, size_t bytes_per_client,
                                               void *d_records, void *stream) {
    return aes_ctr_device(client_ids, n, d_cipher, bytes_per_client, d_records, (hipStream_t)stream);
}

// AES-128-GCM over n client slices (include/fltee_agg.h).  encrypt: plaintext slices of
// ct_bytes in, (ciphertext || tag) slices out; else the reverse, with the tags verified.
static fltee_status_t gcm_device(const uint32_t *client_ids, size_t n, const void *d_in, size_t ct_bytes,
                                 const uint8_t *iv, const uint8_t *aad, size_t aad_len, void *d_out,
                                 uint32_t *d_fail, bool encrypt, hipStream_t s) {
    if (!gcm_sizes_ok(ct_bytes, aad_len) || !iv || (aad_len && !aad) || (encrypt && ct_bytes % 8))
        return FLTEE_ERROR_INVALID_PARAMETER;
    if (n == 0) return FLTEE_SUCCESS;
    if (!client_ids || (!d_in && (ct_bytes || !encrypt)) || (!d_out && (encrypt || ct_bytes >= 8)) ||
        (!encrypt && !d_fail))
        return FLTEE_ERROR_INVALID_PARAMETER;
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_INVALID_PARAMETER;
    std::vector<uint8_t> host;
    GcmDev gd = {};
    if (uint32_t st = gcm_prepare(c, client_ids, n, ct_bytes, iv, aad, aad_len, host, s, gd)) return st;
    const size_t stride = ct_bytes + FLTEE_GCM_TAG_BYTES, rpc = ct_bytes / 8;
    if (encrypt) {
        uint8_t *ct = (uint8_t *)d_out;
        if (launch_aes_ctr_gcm((const uint8_t *)d_in, n, ct_bytes, rpc, gd.rk, ct, stride, iv, s) != hipSuccess ||
            launch_ghash_bulk(ct, n, stride, ct_bytes, gd.aad, aad_len, gd.pow, gd.part, s) != hipSuccess ||
            launch_ghash_finish(ct, n, stride, ct_bytes, aad_len, gd.sub, gd.pow, gd.part, true, nullptr,
                                nullptr, s) != hipSuccess)
            return FLTEE_ERROR_UNEXPECTED;
    } else {
        const uint8_t *ct = (const uint8_t *)d_in;
        if (gcm_verify(gd, 0, n, ct, ct_bytes, aad_len, d_fail, c->status, s) ||
            launch_aes_ctr_gcm(ct, n, stride, rpc, gd.rk, (uint8_t *)d_out, rpc * 8, iv, s) != hipSuccess)
            return FLTEE_ERROR_UNEXPECTED;
    }
    // the staged keys live on this stack frame: wait for the copies + kernels
    return fl_stream_sync(s) == hipSuccess ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_decrypt_auth_device(const uint32_t *client_ids, size_t n,
                                                    const void *d_cipher, size_t ct_bytes,
                                                    const uint8_t iv[12], const uint8_t *aad,
                                                    size_t aad_len, void *d_records, uint32_t *d_fail,
                                                    void *stream) {
    return gcm_device(client_ids, n, d_cipher, ct_bytes, iv, aad, aad_len, d_records, d_fail, false,
                      (hipStream_t)stream);
}

extern "C" fltee_status_t fltee_encrypt_auth_device(const uint32_t *client_ids, size_t n,
                                                    const void *d_plain, size_t ct_bytes,
                                                    const uint8_t iv[12], const uint8_t *aad,
                                                    size_t aad_len, void *d_cipher, void *stream) {
    return gcm_device(client_ids, n, d_plain, ct_bytes, iv, aad, aad_len, d_cipher, nullptr, true,
                      (hipStream_t)stream);
}

extern "C" fltee_status_t fltee_debug_gcm_tag_host(uint32_t client_id, const uint8_t iv[12],
                                                   const uint8_t *aad, size_t aad_len,
                                                   const uint8_t *ct, size_t ct_len, uint8_t tag[16]) {
    if (!gcm_sizes_ok(ct_len, aad_len) || !iv || !tag || (aad_len && !aad) || (ct_len && !ct))
        return FLTEE_ERROR_INVALID_PARAMETER;
    uint32_t rk[44];
    uint8_t sub[32];
    aes128_session_round_keys(&client_id, 1, rk);
    aes128_gcm_subkeys(rk, 1, iv, sub);
    gcm_tag_host(sub, sub + 16, aad, aad_len, ct, ct_len, tag);
    return FLTEE_SUCCESS;
}

// ---- the pieces of a column-sharded authenticated decrypt (include/fltee_agg.h) ----------
// a window [16 first_block, 16 first_block + win_bytes) of a slice of ct_bytes: inside the
// slice, ending on a block boundary or at the slice's end
static bool gcm_window_ok(size_t ct_bytes, size_t aad_len, size_t first_block, size_t win_bytes) {
    if (!gcm_sizes_ok(ct_bytes, aad_len)) return false;
    if (first_block > ct_bytes / 16) return false;  // starts past the slice
    const size_t lo = first_block * 16;
    if (win_bytes > ct_bytes - lo) return false;  // reaches past it
    return win_bytes % 16 == 0 || lo + win_bytes == ct_bytes;
}

extern "C" size_t fltee_gcm_segments(size_t ct_bytes, size_t aad_len) {
    return ghash_segments(ct_bytes, aad_len);
}

extern "C" fltee_status_t fltee_ghash_window_device(const uint32_t *client_ids, size_t n,
                                                    const void *d_window, size_t row_stride,
                                                    size_t ct_bytes, size_t first_block,
                                                    size_t win_bytes, const uint8_t *aad, size_t aad_len,
                                                    int with_aad, void *d_part, void *stream) {
    if (!gcm_window_ok(ct_bytes, aad_len, first_block, win_bytes) || row_stride < win_bytes ||
        (with_aad && aad_len && !aad))
        return FLTEE_ERROR_INVALID_PARAMETER;
    if (n == 0) return FLTEE_SUCCESS;
    if (!client_ids || !d_part || (win_bytes && !d_window)) return FLTEE_ERROR_INVALID_PARAMETER;
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_INVALID_PARAMETER;
    hipStream_t s = (hipStream_t)stream;
    if (!c->gcm_sub.reserve(n * 96) || !c->gcm_pow.reserve(ghash_pow_bytes(n))) return FLTEE_ERROR_OUT_OF_MEMORY;
    // H needs no IV (E_K(J0), computed beside it, is not read here)
    static const uint8_t zero_iv[12] = {};
    std::vector<uint8_t> host;
    gcm_host_keys(client_ids, n, zero_iv, with_aad ? aad : nullptr, with_aad ? aad_len : 0, host);
    const uint8_t *sub = (const uint8_t *)c->gcm_sub.ptr;
    if (fl_memcpy_async(c->gcm_sub.ptr, host.data() + n * 44 * 4, n * 96, hipMemcpyHostToDevice, s) != hipSuccess ||
        launch_ghash_powers(sub, n, c->gcm_pow.ptr, s) != hipSuccess ||
        launch_ghash_window((const uint8_t *)d_window, n, row_stride, ct_bytes, first_block, win_bytes,
                            sub + n * 32, aad_len, with_aad != 0, c->gcm_pow.ptr, d_part, s) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    // the staged keys live on this stack frame
    return fl_stream_sync(s) == hipSuccess ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_ghash_merge_device(void *d_acc, const void *d_part, size_t n, size_t P,
                                                   void *stream) {
    if (n == 0 || P == 0) return FLTEE_SUCCESS;
    if (!d_acc || !d_part || (uintptr_t)d_acc % 16 || (uintptr_t)d_part % 16 || P > SIZE_MAX / 16 / n)
        return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_ghash_merge(d_acc, d_part, n, P, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_gcm_finish_device(const uint32_t *client_ids, size_t n, const void *d_part,
                                                  size_t ct_bytes, const uint8_t iv[12], size_t aad_len,
                                                  const void *d_tags, uint32_t *d_fail, void *stream) {
    if (!gcm_sizes_ok(ct_bytes, aad_len) || !iv) return FLTEE_ERROR_INVALID_PARAMETER;
    if (n == 0) return FLTEE_SUCCESS;
    if (!client_ids || !d_part || !d_tags || !d_fail) return FLTEE_ERROR_INVALID_PARAMETER;
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_INVALID_PARAMETER;
    hipStream_t s = (hipStream_t)stream;
    if (!c->gcm_sub.reserve(n * 96) || !c->gcm_pow.reserve(ghash_pow_bytes(n))) return FLTEE_ERROR_OUT_OF_MEMORY;
    std::vector<uint8_t> host;
    gcm_host_keys(client_ids, n, iv, nullptr, 0, host);
    const uint8_t *sub = (const uint8_t *)c->gcm_sub.ptr;
    if (fl_memcpy_async(c->gcm_sub.ptr, host.data() + n * 44 * 4, n * 32, hipMemcpyHostToDevice, s) != hipSuccess ||
        launch_ghash_powers(sub, n, c->gcm_pow.ptr, s) != hipSuccess ||
        launch_ghash_finish_tags((uint8_t *)const_cast<void *>(d_tags), FLTEE_GCM_TAG_BYTES, n, ct_bytes,
                                 aad_len, sub, c->gcm_pow.ptr, d_part, false, d_fail, c->status,
                                 s) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    return fl_stream_sync(s) == hipSuccess ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_decrypt_slice_auth_device(const uint32_t *client_ids, size_t n,
                                                          const void *d_window, size_t row_stride,
                                                          size_t first_block, size_t win_bytes,
                                                          const uint8_t iv[12], void *d_records,
                                                          void *stream) {
    // the window's last counter is 1 + first_block + ceil(win_bytes / 16): within 32 bits
    const uint64_t lim = ((uint64_t)1 << 36) - 32;
    if (!iv || row_stride < win_bytes || (uint64_t)first_block > lim / 16 ||
        (uint64_t)win_bytes > lim - 16 * (uint64_t)first_block)
        return FLTEE_ERROR_INVALID_PARAMETER;
    if (n == 0 || win_bytes < 8) return FLTEE_SUCCESS;
    if (!client_ids || !d_window || !d_records) return FLTEE_ERROR_INVALID_PARAMETER;
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_INVALID_PARAMETER;
    hipStream_t s = (hipStream_t)stream;
    if (!c->round_keys.reserve(n * 44 * 4)) return FLTEE_ERROR_OUT_OF_MEMORY;
    std::vector<uint32_t> rk(n * 44);
    aes128_session_round_keys(client_ids, n, rk.data());
    const size_t rpc = win_bytes / 8;
    if (fl_memcpy_async(c->round_keys.ptr, rk.data(), rk.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        launch_aes_ctr_gcm_slice((const uint8_t *)d_window, n, row_stride, rpc,
                                 (const uint32_t *)c->round_keys.ptr, (uint8_t *)d_records, rpc * 8, iv,
                                 first_block, 0, s) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    return fl_stream_sync(s) == hipSuccess ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_debug_ghash_window_host(uint32_t client_id, const uint8_t *aad,
                                                        size_t aad_len, int with_aad,
                                                        const uint8_t *ct_window, size_t ct_bytes,
                                                        size_t first_block, size_t win_bytes,
                                                        uint8_t *part_out) {
    if (!gcm_window_ok(ct_bytes, aad_len, first_block, win_bytes) || !part_out ||
        (with_aad && aad_len && !aad) || (win_bytes && !ct_window))
        return FLTEE_ERROR_INVALID_PARAMETER;
    static const uint8_t zero_iv[12] = {};
    uint32_t rk[44];
    uint8_t sub[32];
    aes128_session_round_keys(&client_id, 1, rk);
    aes128_gcm_subkeys(rk, 1, zero_iv, sub);
    ghash_window_host(sub, aad, aad_len, with_aad != 0, ct_window, ct_bytes, first_block, win_bytes, part_out);
    return FLTEE_SUCCESS;
}

extern "C" void fltee_set_upload_aead(int on) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    g_upload_aead = on != 0;
}

extern "C" void fltee_set_upload_packed(int on) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    g_upload_packed = on != 0;
}

extern "C" size_t fltee_trim_count(size_t n, uint32_t per_mille) { return trim_count(n, per_mille); }

extern "C" void fltee_set_dense_trim_select(int on) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    g_dense_trim_select = on != 0;
}

extern "C" void fltee_set_dense_gmed(uint32_t iters, double nu) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    g_dense_gmed_iters = iters, g_dense_gmed_nu = nu;
}

extern "C" void fltee_set_dense_krum(uint32_t f, uint32_t m) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    g_dense_krum_f = f, g_dense_krum_m = m;
}

extern "C" void fltee_set_dense_trim(uint32_t per_mille) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    g_dense_trim = per_mille > 500 ? 500 : per_mille;
}

extern "C" int fltee_upload_is_packed(int on, size_t d, size_t k_req, size_t ct_bytes) {
    return upload_is_rows(kRowsF32, on != 0, d, k_req, ct_bytes) ? 1 : 0;
}

extern "C" void fltee_set_upload_bf16(int on) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    g_upload_bf16 = on != 0;
}

extern "C" int fltee_upload_is_bf16(int on, size_t d, size_t k_req, size_t ct_bytes) {
    return upload_is_rows(kRowsBf16, on != 0, d, k_req, ct_bytes) ? 1 : 0;
}

extern "C" void fltee_set_upload_fp8(int on) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    g_upload_fp8 = on != 0;
}

extern "C" int fltee_upload_is_fp8(int on, size_t d, size_t k_req, size_t ct_bytes) {
    return upload_is_rows(kRowsFp8, on != 0, d, k_req, ct_bytes) ? 1 : 0;
}

extern "C" void fltee_set_upload_aead_policy(int policy, size_t min_survivors) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    // (an unknown value is the default: a host never gets a weaker contract by mistake)
    g_aead_policy = policy == FLTEE_AEAD_REPORT || policy == FLTEE_AEAD_DROP ? policy : FLTEE_AEAD_ABORT;
    g_aead_min_survivors = min_survivors ? min_survivors : 1;
}

extern "C" fltee_status_t fltee_auth_report(fltee_eid_t eid, uint32_t fl_id, uint32_t *round,
                                            uint32_t *failed_ids, size_t cap, size_t *n_failed) {
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    if (!n_failed || (cap && !failed_ids)) return FLTEE_ERROR_INVALID_PARAMETER;
    *n_failed = 0;
    // the configs (and so the verdicts) are keyed by fl_id for the whole process, like
    // FL_CONFIG_MAP: an unknown fl_id is answered first, whatever the eid
    auto cf = g_cfg.find(fl_id);
    if (cf == g_cfg.end()) return FLTEE_ERROR_UNEXPECTED;
    if (eid == 0 || eid > g_eid_dev.size() || g_eid_dev[eid - 1] < 0) return FLTEE_ERROR_INVALID_ENCLAVE_ID;
    auto it = g_auth_reports.find(fl_id);
    if (it == g_auth_reports.end()) {  // no verdict stored (ABORT, AEAD off, no call yet)
        if (round) *round = cf->second.round;
        return FLTEE_SUCCESS;
    }
    const AuthReport &r = it->second;
    if (round) *round = r.round;
    *n_failed = r.failed.size();
    std::copy(r.failed.begin(), r.failed.begin() + std::min(cap, r.failed.size()), failed_ids);
    return FLTEE_SUCCESS;
}

extern "C" fltee_status_t fltee_gather_clients_device(const void *d_records, size_t n, size_t k,
                                                      const uint32_t *d_keep, size_t n_keep,
                                                      void *d_out, void *stream) {
    if (!d_records || !d_keep || !d_out || n_keep > n || k == 0 || n > (((size_t)1 << 31) - 1) / k)
        return FLTEE_ERROR_INVALID_PARAMETER;
    if (n_keep == 0) return FLTEE_SUCCESS;
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_gather_clients(d_records, n, k, d_keep, n_keep, d_out, c->status,
                                 (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS : FLTEE_ERROR_UNEXPECTED;
}

// CPU self-test hooks: the one GF(2^128) multiply (GCM byte order), the subkeys H ||
// E_K(J0) by the AES-NI or the portable path, the bulk kernel's segment size
extern "C" void fltee_debug_gf128_mul(const uint8_t a[16], const uint8_t b[16], uint8_t out[16]) {
    fltee::gf128_mul_host(a, b, out);
}
extern "C" int fltee_debug_gcm_subkeys(uint32_t client_id, const uint8_t iv[12], uint8_t sub[32],
                                       int portable) {
    uint32_t rk[44];
    fltee::aes128_session_round_keys_portable(&client_id, 1, rk);
    if (portable || !fltee::host_has_aesni()) {
        fltee::aes128_gcm_subkeys_portable(rk, 1, iv, sub);
        return 0;
    }
    fltee::aes128_gcm_subkeys(rk, 1, iv, sub);
    return 1;
}
extern "C" size_t fltee_debug_gcm_segment_blocks(void) { return FLTEE_GCM_SEGMENT_BLOCKS; }

// ------------------------------------------- client-side producers (§8f.4) ----
extern "C" fltee_status_t fltee_encrypt_device(const uint32_t *client_ids, size_t n,
                                               const void *d_plain, size_t bytes_per_client,
                                               void *d_cipher, void *stream) {
    for (size_t i = 0; i < n; ++i)  // encrypt_parameters: int(id).to_bytes(2, 'big')
        if (client_ids[i] > 0xFFFFu) return FLTEE_ERROR_INVALID_PARAMETER;
    return aes_ctr_device(client_ids, n, d_plain, bytes_per_client, d_cipher, (hipStream_t)stream);
}

namespace fltee {
hipError_t launch_client_topk(const float *values, size_t n, size_t d, size_t k, uint64_t *keys,
                              uint64_t *rec, hipStream_t s);
size_t client_topk_workspace(size_t n, size_t d);
hipError_t launch_client_dense(const float *values, size_t n, size_t d, uint64_t *rec,
                               hipStream_t s);
}  // namespace fltee

extern "C" fltee_status_t fltee_client_topk_device(const float *d_values, size_t n, size_t d,
                                                   size_t k, void *d_records, void *stream) {
    if (n == 0 || d == 0 || k > d || d > 0xFFFFFFFFull) return FLTEE_ERROR_INVALID_PARAMETER;
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_INVALID_PARAMETER;
    if (k == 0) return FLTEE_SUCCESS;
    if (!c->ws_client.reserve(client_topk_workspace(n, d))) return FLTEE_ERROR_OUT_OF_MEMORY;
    return launch_client_topk(d_values, n, d, k, (uint64_t *)c->ws_client.ptr,
                              (uint64_t *)d_records, (hipStream_t)stream) == hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_client_serialize_dense_device(const float *d_values, size_t n,
                                                              size_t d, void *d_records,
                                                              void *stream) {
    if (n == 0 || d == 0 || d > 0xFFFFFFFFull) return FLTEE_ERROR_INVALID_PARAMETER;
    return launch_client_dense(d_values, n, d, (uint64_t *)d_records, (hipStream_t)stream) ==
                   hipSuccess
               ? FLTEE_SUCCESS
               : FLTEE_ERROR_UNEXPECTED;
}

extern "C" fltee_status_t fltee_client_clip_device(void *d_records, size_t n, size_t k,
                                                   float clipping, void *stream) {
    if (n == 0) return FLTEE_ERROR_INVALID_PARAMETER;
    std::lock_guard<std::recursive_mutex> lk(api_mutex());
    DeviceCtx *c = current_ctx();
    if (!c) return FLTEE_ERROR_INVALID_PARAMETER;
    if (!c->ws_client_coef.reserve(n * 4)) return FLTEE_ERROR_OUT_OF_MEMORY;
    hipStream_t s = (hipStream_t)stream;
    float *cf = (float *)c->ws_client_coef.ptr;
    if (launch_client_clip_coef(d_records, n, k, clipping, cf, s) != hipSuccess ||
        launch_apply_clip(d_records, n, k, cf, s) != hipSuccess)
        return FLTEE_ERROR_UNEXPECTED;
    return FLTEE_SUCCESS;
}

// CPU self-test hook: the clients' round keys by the AES-NI schedule (when the CPU has
// it) or by the portable bitsliced one (portable != 0); returns 1 when AES-NI was used.
namespace fltee {
void aes128_session_round_keys_portable(const uint32_t *ids, size_t n, uint32_t *rk);
bool host_has_aesni();
}
extern "C" int fltee_debug_session_round_keys(const uint32_t *ids, size_t n, uint32_t *rk, int portable) {
    if (portable || !fltee::host_has_aesni()) {
        fltee::aes128_session_round_keys_portable(ids, n, rk);
        return 0;
    }
    fltee::aes128_session_round_keys(ids, n, rk);
    return 1;
}

// CPU self-test hook: one AES-128 block with the library's tables (no GPU).
namespace fltee { void aes128_encrypt_block_host(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]); }
extern "C" void fltee_debug_aes_block(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
    fltee::aes128_encrypt_block_host(key, in, out);
}
