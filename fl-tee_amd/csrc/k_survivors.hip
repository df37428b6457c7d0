// k_survivors.hip — the survivors gather of authenticated rounds (fltee_set_upload_aead_policy,
// FLTEE_AEAD_DROP): the decrypted records of the clients whose tags verified, compacted
// client-major into a second buffer, so that the unchanged aggregation routes run on
// (n', k):
//     dst[s][0..k) = src[keep[s]][0..k),  s < n_keep, keep ascending, in device memory.
// Never in place: with client 0 dropped dst[c] overlaps src[c - 1], and blocks run in any
// order.  A pure copy, read once (nontemporal loads) and written once; the grid covers
// (survivor, 16 KB chunk of its slice), so one long slice still fills the chip, and every
// wave moves 1 KB of consecutive bytes per instruction.
//
// Vector width, per slice: a source and a destination slice whose addresses agree modulo 16
// move as 16-byte vectors (an 8-byte record in front where both start 8 past a 16-byte
// boundary, an 8-byte record behind where one is left over: k odd, or the head taken); a
// pair that disagrees — k odd and keep[s] - s odd, or bases 8 apart — moves as 8-byte
// records.  The choice follows the public k, the addresses and keep (the failed set, which
// the host gets from the report anyway), never the records.
#include "common.h"

namespace fltee {

constexpr int kGatherThreads = 256;
constexpr int kGatherVecs = 4;                                          // 16-byte vectors per lane
constexpr uint32_t kGatherChunk = kGatherThreads * kGatherVecs * 2;     // records per block (16 KB)

typedef uint32_t gather_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t gather_u32x2 __attribute__((ext_vector_type(2)));

// an index >= n in keep (the host cannot see it): clamped, so nothing is read out of bounds,
// and reported with FLTEE_DEV_ERR_LAUNCH in *status
__global__ __launch_bounds__(kGatherThreads) void gather_clients_kernel(
    const uint2 *__restrict__ src, uint2 *__restrict__ dst, const uint32_t *__restrict__ keep,
    uint32_t n, uint32_t k, uint32_t chunks, uint32_t *__restrict__ status) {
    const uint32_t s = blockIdx.x / chunks, ch = blockIdx.x - s * chunks;
    uint32_t c = keep[s];
    if (c >= n) {
        if (ch == 0 && threadIdx.x == 0) atomicOr(status, FLTEE_DEV_ERR_LAUNCH);
        c = n - 1;
    }
    const uint32_t r0 = ch * kGatherChunk;
    const uint32_t len = (k - r0 < kGatherChunk) ? k - r0 : kGatherChunk;  // records of this chunk
    const uint2 *sp = src + (size_t)c * k + r0;
    uint2 *dp = dst + (size_t)s * k + r0;
    const uint32_t t = threadIdx.x;
    if ((((uintptr_t)sp ^ (uintptr_t)dp) & 8u) == 0) {
        const uint32_t head = (uint32_t)(((uintptr_t)sp >> 3) & 1u);  // (len >= 1)
        const uint32_t nv = (len - head) >> 1, tail = (len - head) & 1u;
        const gather_u32x4 *sv = reinterpret_cast<const gather_u32x4 *>(sp + head);
        gather_u32x4 *dv = reinterpret_cast<gather_u32x4 *>(dp + head);
        gather_u32x4 x[kGatherVecs];
#pragma unroll
        for (int u = 0; u < kGatherVecs; ++u) {
            const uint32_t v = t + u * kGatherThreads;
            if (v < nv) x[u] = __builtin_nontemporal_load(sv + v);
        }
#pragma unroll
        for (int u = 0; u < kGatherVecs; ++u) {
            const uint32_t v = t + u * kGatherThreads;
            if (v < nv) dv[v] = x[u];
        }
        if (t == 0 && head) dp[0] = sp[0];
        if (t == 64 && tail) dp[len - 1] = sp[len - 1];
        return;
    }
    const gather_u32x2 *s2 = reinterpret_cast<const gather_u32x2 *>(sp);
    gather_u32x2 *d2 = reinterpret_cast<gather_u32x2 *>(dp);
    gather_u32x2 y[2 * kGatherVecs];
#pragma unroll
    for (int u = 0; u < 2 * kGatherVecs; ++u) {
        const uint32_t r = t + u * kGatherThreads;
        if (r < len) y[u] = __builtin_nontemporal_load(s2 + r);
    }
#pragma unroll
    for (int u = 0; u < 2 * kGatherVecs; ++u) {
        const uint32_t r = t + u * kGatherThreads;
        if (r < len) d2[r] = y[u];
    }
}

// what one launch covers: 32-bit n and k, and n_keep * chunks blocks in a 1-D grid (every
// n * k < 2^31 with n_keep <= n does)
bool gather_clients_fits(size_t n, size_t k, size_t n_keep) {
    if (n > 0xFFFFFFFFull || k > 0xFFFFFFFFull || n_keep > n) return false;
    const size_t chunks = (k + kGatherChunk - 1) / kGatherChunk;
    return chunks == 0 || n_keep <= 0x7FFFFFFFull / chunks;
}

// the callers check gather_clients_fits
hipError_t launch_gather_clients(const void *rec, size_t n, size_t k, const uint32_t *keep,
                                 size_t n_keep, void *out, uint32_t *status, hipStream_t s) {
    if (n_keep == 0 || k == 0) return hipSuccess;
    const uint32_t chunks = (uint32_t)((k + kGatherChunk - 1) / kGatherChunk);
    FLTEE_LAUNCH(gather_clients_kernel, dim3((unsigned)(n_keep * chunks)), dim3(kGatherThreads), 0, s,
                 (const uint2 *)rec, (uint2 *)out, keep, (uint32_t)n, (uint32_t)k, chunks, status);
    return hipGetLastError();
}

}  // namespace fltee
