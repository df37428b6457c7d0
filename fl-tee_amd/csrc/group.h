// group.h — an enclave id spanning several GPUs (group.hip).
#pragma once
#include "common.h"
#include "engine.h"

namespace fltee {

struct Group;
// returned by the group paths when the shape is not sharded there (the caller runs
// the single-device path on the root)
constexpr uint32_t FLTEE_GROUP_FALLBACK = 0xFFFFFFFEu;

Group *group_create(const int *devs, int n, uint32_t *status);
void group_destroy(Group *G);
int group_size(const Group *G);
int group_root_device(const Group *G);
hipStream_t group_root_stream(const Group *G);

// An authenticated call's keys on the host (fltee_set_upload_aead): per client H || E_K(J0)
// (32 bytes) and the AAD zero padded to 64 bytes, the two arrays one behind the other (sub,
// then aad64 = sub + 32 n), and the call's IV.  The slices then carry a 16-byte tag.
struct GcmHost {
    const uint8_t *sub = nullptr, *aad64 = nullptr, *iv = nullptr;
    size_t aad_len = 0;
};

// What a dense group call computes from the ranks' decrypted columns (group_dense_ecall's rb)
struct GroupRobust {
    enum Kind : uint32_t { kPlain, kTrim, kTrimSelect, kKrum, kGmed } kind = kPlain;
    size_t trim = 0;               // kTrim, kTrimSelect: t >= 1
    size_t krum_f = 0, krum_m = 0;
    size_t gmed_iters = 0;
    double gmed_nu = 0.0;
};

// dense uploads straight from the host ciphertext, parameter-range sharded; rk_host =
// the n clients' AES round keys (44 words each); d_out_root gets the averaged f32[d].
// A record out of position: reject_order (baseline / path_oram, fixed cost) -> 0x2, else
// FLTEE_GROUP_FALLBACK (non_oblivious reruns it with scatter semantics on the root).
// gcm: the slices are d * 8 bytes of ciphertext || tag.  Every rank decrypts its columns with
// the GCM counters and hashes them as a window of the slices (k_ghash.hip); the root takes
// the tags, XORs the ranks' partials and finishes; one auth word is read, and only then is
// any rank's accumulate launched: FLTEE_ERROR_MAC_MISMATCH otherwise.
// rb (the robust switches; the default is the plain mean, launch for launch what it was): after
// the same load, decrypt and verdict every rank runs the call's one-GPU route on its columns — the
// trimmed mean (kTrim: the list kernel, kTrimSelect: the selection kernel, trim = t clients a
// side), or under kKrum / kGmed the columns are cut on the Gram pass's chunk boundaries, the
// ranks' Gram partials are added by a carry chain in the one-GPU order, the root selects on G and
// sends the keep (alpha, valid) words to the ranks, which sum their columns.  Nothing reads a
// plaintext value before the verdict.  A record out of position then ends the call with 0x2
// whatever reject_order says (the sparse rerun would be a plain mean).
uint32_t group_dense_ecall(Group *G, const uint32_t *rk_host, size_t n, const uint8_t *enc,
                           size_t d, float coef, float *d_out_root, float *t_load, float *t_dec,
                           bool reject_order, const GcmHost *gcm = nullptr,
                           const GroupRobust &rb = GroupRobust());
// Where the client-major n x k records come from: decrypted into the root device's HBM
// (root_rec), or the host ciphertext (enc, bpc bytes per client, rk = the clients' round
// keys): then every GPU of the eid copies and decrypts the clients covering its own
// range (t_load / t_dec: the ECALL's "Loading" / "Decryption" times).  gcm (with enc): bpc is
// the stride B + 16, and every GPU also verifies the tags of the clients it loaded (a client
// on a range boundary by both of its ranks); the ranks' auth words are read before anything
// is aggregated, and a mismatch on any of them ends the call: FLTEE_ERROR_MAC_MISMATCH.
struct GroupInput {
    const uint64_t *root_rec = nullptr;
    const uint8_t *enc = nullptr;
    const uint32_t *rk = nullptr;
    size_t bpc = 0;
    float *t_load = nullptr, *t_dec = nullptr;
    const GcmHost *gcm = nullptr;
};
uint32_t group_advanced(Group *G, const GroupInput &in, size_t n, size_t k, size_t d, float coef,
                        float *d_out_root);
// alg 7 (k fold entries per client = the request's k): the stable network of k_stable.hip
// over position ranges (pairwise exchanges), then group_advanced's tail
uint32_t group_bubble(Group *G, const GroupInput &in, size_t n, size_t k, size_t d, float coef,
                      float *d_out_root);
uint32_t group_nips19(Group *G, DeviceCtx *root, const GroupInput &in, size_t n, size_t k,
                      size_t k_req, size_t d, uint64_t seed, float coef, float *d_out_root);
// halo: the fold halo of every batch (n, or the exact-runs policy's worst case)
uint32_t group_optimized(Group *G, const GroupInput &in, size_t n, size_t k, size_t d,
                         size_t batch, float coef, float *d_out_root, size_t halo);
// true when the group loads the host ciphertext per GPU (eids of > 1 rank)
bool group_splits_host_copy(const Group *G);

}  // namespace fltee
