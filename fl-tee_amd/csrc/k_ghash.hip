// k_ghash.hip — GHASH of AES-128-GCM over the uploaded client slices (gfx950), constant time.
//
// With fltee_set_upload_aead(1) a client's slice is ciphertext (B bytes) || tag (16 bytes) of
// standard AES-128-GCM (NIST SP 800-38D, 96-bit IV): H = E_K(0^128), J0 = IV || 0x00000001,
// T = GHASH_H(AAD || pad || C || pad || BE64(8 |AAD|) || BE64(8 |C|)) ^ E_K(J0).  The CTR half
// is k_aes.hip's bitsliced kernels with the IV as constant counter planes; this file is the
// MAC.  The multiply is ghash.h's gf128_mul (integer multiplies with holes, Karatsuba), the
// same function on the host (fltee_debug_gcm_tag_host) and in every kernel here.
//
// VALU cost of one gf128_mul, counted in this file's gfx950 ISA (the bulk kernel's loop
// body): 288 v_mul_lo_u32 + ~510 other VALU (v_xor / v_bitop3 / v_and / v_bfrev / shifts) =
// ~800 VALU instructions per lane.  The bulk kernel spends one multiply per 16-byte block
// plus one per lane per segment (1 / 8 more): ~900 VALU per block, i.e. ~14 wave-instructions
// per block (the multiplies issue at half rate: ~19 issue slots per block).
//
// Layout.  A client's GHASH input AAD blocks || C blocks (the closing length block apart)
// is RIGHT-aligned in P segments of S = kGhashSeg blocks: pad = P S - (a + m) virtual zero
// blocks in front change nothing, and every segment is whole.  With x_j the virtual block j,
//     Y = sum_j x_j H^(P S - j) = sum_s part_s G^(P - 1 - s),   G = H^S,
//     part_s = sum_{j < S} x_{s S + j} H^(S - j).
//   ghash_powers_kernel   one wave per client: H^0..H^64 and G^0..G^64 by doubling through
//                         LDS (6 + log2(S / 64) + 6 dependent multiplies).
//   ghash_bulk_kernel     one wave per (client, segment): lane l runs the Horner chain over
//                         the blocks l, l + 64, ... of the segment (multiplier H^64; the
//                         wave's 64 loads of 16 B are 1 KB contiguous), multiplies by
//                         H^(64 - l) and the wave XORs its lanes: part_s, 16 bytes to scratch.
//                         The ciphertext is read, never written.
//   ghash_finish_kernel   one wave per client: the same chain over the partials (multiplier
//                         G^64, weights G^(63 - l)), then (Y ^ lengths) H ^ E_K(J0).  Verify:
//                         the OR of the XOR with the received tag -> fail[c] (0 / 1) and
//                         FLTEE_DEV_ERR_AUTH into the status word, no early exit, and the
//                         computed tag stays in registers.  Emit (the client producer):
//                         the tag is written behind the ciphertext.
//   ghash_window_kernel the bulk kernel on a WINDOW of every slice (a multi-GPU eid's column
//                         shard, group.hip): a rank holds the ciphertext blocks [first_block,
//                         first_block + ceil(win_bytes / 16)) of each client at a row stride
//                         of its own and writes part_s in the WHOLE slice's segment layout.
//                         part_s is XOR-linear in the segment's blocks, so blocks outside the
//                         window count as zero and the XOR of the ranks' partial vectors
//                         (ghash_merge_kernel, 16-B lanes) is the slice's, bit for bit.  Only
//                         the segments the window (and, on the one window that carries them,
//                         the AAD blocks) touches are launched — an untouched segment would
//                         cost its S multiplies for a zero — and the others are a memset;
//                         inside a touched segment the blocks before and behind the window are
//                         masked by position (v_cmp / v_cndmask on public values).
// Every size, grid and loop bound is a function of (n, B, |AAD|) — for a window, of (n, B,
// |AAD|, first_block, win_bytes) — only.
#include <vector>

#include "common.h"
#include "ghash.h"

namespace fltee {

static_assert(FLTEE_GCM_SEGMENT_BLOCKS == 512, "kGhashSegLog follows the header's constant");
constexpr int kGhashSeg = FLTEE_GCM_SEGMENT_BLOCKS;  // S: blocks per segment (8 KB)
constexpr int kGhashChain = kGhashSeg / 64;          // blocks per lane
constexpr int kGhashSegLog = 3;                      // S = 64 << 3: G = (H^64)^(2^3)
constexpr int kGhashPow = 130;                       // per client: H^0..H^64, G^0..G^64
constexpr int kGhashAadBytes = 64;                   // per client, zero padded

size_t ghash_segments(size_t ct_bytes, size_t aad_len) {
    const size_t blocks = (ct_bytes + 15) / 16 + (aad_len + 15) / 16;
    return (blocks + kGhashSeg - 1) / kGhashSeg;
}
size_t ghash_pow_bytes(size_t n) { return n * kGhashPow * sizeof(gf128); }
size_t ghash_part_bytes(size_t n, size_t ct_bytes, size_t aad_len) {
    return n * ghash_segments(ct_bytes, aad_len) * sizeof(gf128);
}

// ---------------------------------------------------------------- host: the same multiply
void gf128_mul_host(const uint8_t a[16], const uint8_t b[16], uint8_t out[16]) {
    const gf128 r = gf128_mul(gf128_from_bytes(a), gf128_from_bytes(b));
    for (int j = 0; j < 4; ++j) {
        const uint32_t v = gf128_le_word(r, j);
        for (int i = 0; i < 4; ++i) out[4 * j + i] = (uint8_t)(v >> (8 * i));
    }
}

// GHASH_H(AAD || pad || C || pad || lengths) ^ ej0, block after block
void gcm_tag_host(const uint8_t h[16], const uint8_t ej0[16], const uint8_t *aad, size_t aad_len,
                  const uint8_t *ct, size_t ct_len, uint8_t tag[16]) {
    const gf128 H = gf128_from_bytes(h);
    gf128 y = gf128_zero();
    auto absorb = [&](const uint8_t *p, size_t len) {
        for (size_t o = 0; o < len; o += 16) {
            uint8_t blk[16] = {};
            for (size_t i = 0; i < 16 && o + i < len; ++i) blk[i] = p[o + i];
            y = gf128_mul(gf128_xor(y, gf128_from_bytes(blk)), H);
        }
    };
    absorb(aad, aad_len);
    absorb(ct, ct_len);
    y = gf128_mul(gf128_xor(y, gf128_lengths(aad_len, ct_len)), H);
    for (int j = 0; j < 4; ++j) {
        const uint32_t v = gf128_le_word(y, j);
        for (int i = 0; i < 4; ++i) tag[4 * j + i] = (uint8_t)(v >> (8 * i)) ^ ej0[4 * j + i];
    }
}

// One window's partial vector on the host, block after block with the same multiply: part_s =
// sum over the window's (and, with_aad, the AAD's) virtual blocks j of segment s of
// x_j H^(S - j mod S); ct_window holds the window's win_bytes bytes
void ghash_window_host(const uint8_t h[16], const uint8_t *aad, size_t aad_len, bool with_aad,
                       const uint8_t *ct_window, size_t ct_bytes, uint64_t first_block,
                       size_t win_bytes, uint8_t *part_out) {
    const gf128 H = gf128_from_bytes(h);
    const uint64_t P = ghash_segments(ct_bytes, aad_len), ab = (aad_len + 15) / 16;
    const uint64_t pad = P * kGhashSeg - ((ct_bytes + 15) / 16 + ab);
    auto block = [&](uint64_t v) {
        uint8_t blk[16] = {};
        if (v >= pad && v - pad < ab) {
            const size_t o = 16 * (v - pad);
            for (size_t i = 0; with_aad && i < 16 && o + i < aad_len; ++i) blk[i] = aad[o + i];
        } else if (v >= pad + ab && v - pad - ab >= first_block) {
            const uint64_t o = 16 * (v - pad - ab - first_block);
            for (size_t i = 0; i < 16 && o + i < win_bytes; ++i) blk[i] = ct_window[o + i];
        }
        return gf128_from_bytes(blk);
    };
    for (uint64_t s = 0; s < P; ++s) {
        gf128 y = gf128_zero();  // Horner over the segment: ends with every block times H^(S - j)
        for (uint64_t j = 0; j < (uint64_t)kGhashSeg; ++j)
            y = gf128_mul(gf128_xor(y, block(s * kGhashSeg + j)), H);
        // as the kernels store a partial: the element's words (every byte of the GCM block
        // with its bits reversed)
        for (int j = 0; j < 4; ++j)
            for (int i = 0; i < 4; ++i) part_out[16 * s + 4 * j + i] = (uint8_t)(y.w[j] >> (8 * i));
    }
}

// ------------------------------------------------------------------------------ device
__device__ __forceinline__ gf128 wave_xor(gf128 v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) v.w[i] ^= (uint32_t)__shfl_xor((int)v.w[i], m, 64);
    return v;
}

// T[0] = 1 and T[1] = g given: T[2..64] = g^2..g^64, each step doubling the known range
__device__ __forceinline__ void powers_by_doubling(gf128 *T, uint32_t lane) {
#pragma unroll 1
    for (uint32_t base = 1; base < 64; base <<= 1) {
        __syncthreads();
        const gf128 pr = gf128_mul(T[base], T[(lane & (base - 1)) + 1]);
        if (lane < base) T[base + lane + 1] = pr;
    }
    __syncthreads();
}

// sub: per client H (16 bytes) then E_K(J0) (16 bytes)
__global__ __launch_bounds__(64) void ghash_powers_kernel(const uint8_t *__restrict__ sub,
                                                          gf128 *__restrict__ pow) {
    __shared__ gf128 T[65];
    const uint32_t lane = threadIdx.x, c = blockIdx.x;
    gf128 *out = pow + (size_t)c * kGhashPow;
    if (lane == 0) {
        T[0] = gf128_one();
        T[1] = gf128_from_bytes(sub + (size_t)c * 32);
    }
    powers_by_doubling(T, lane);
    out[lane] = T[lane];
    if (lane == 0) out[64] = T[64];
    gf128 g = T[64];
#pragma unroll 1
    for (int i = 0; i < kGhashSegLog; ++i) g = gf128_mul(g, g);
    __syncthreads();
    if (lane == 0) T[1] = g;
    powers_by_doubling(T, lane);
    out[65 + lane] = T[lane];
    if (lane == 0) out[65 + 64] = T[64];
}

// the virtual block v of client data: zero, an AAD block, or a ciphertext block (the last
// one zero padded)
template <int ALIGN>
__device__ __forceinline__ gf128 ghash_block(uint64_t v, uint64_t pad, uint32_t ablocks,
                                             const uint8_t *__restrict__ aad,
                                             const uint8_t *__restrict__ ct, uint64_t ct_bytes) {
    if (v < pad) return gf128_zero();
    const uint64_t t = v - pad;
    if (t < ablocks) {
        const uint4 q = *reinterpret_cast<const uint4 *>(aad + 16 * t);
        return gf128_from_le_words(q.x, q.y, q.z, q.w);
    }
    const uint64_t o = 16 * (t - ablocks);
    const uint8_t *p = ct + o;
    if (o + 16 <= ct_bytes) {
        if (ALIGN == 16) {
            const uint4 q = *reinterpret_cast<const uint4 *>(p);
            return gf128_from_le_words(q.x, q.y, q.z, q.w);
        }
        if (ALIGN == 8) {
            const uint2 q0 = *reinterpret_cast<const uint2 *>(p);
            const uint2 q1 = *reinterpret_cast<const uint2 *>(p + 8);
            return gf128_from_le_words(q0.x, q0.y, q1.x, q1.y);
        }
        return gf128_from_bytes(p);
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; ++i)
        if (o + i < ct_bytes) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    return gf128_from_le_words(w[0], w[1], w[2], w[3]);
}

template <int ALIGN>
__global__ __launch_bounds__(256) void ghash_bulk_kernel(const uint8_t *__restrict__ cipher,
                                                         size_t stride, uint64_t ct_bytes,
                                                         const uint8_t *__restrict__ aad,
                                                         uint32_t ablocks,
                                                         const gf128 *__restrict__ pow,
                                                         gf128 *__restrict__ part, uint64_t P,
                                                         uint64_t waves) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t pad = P * kGhashSeg - ((ct_bytes + 15) / 16 + ablocks);
    for (uint64_t gw = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); gw < waves;
         gw += (uint64_t)gridDim.x * 4) {
        const uint64_t c = gw / P, s = gw - c * P;
        const uint8_t *ct = cipher + c * stride;
        const uint8_t *ad = aad + c * kGhashAadBytes;
        const gf128 *pw = pow + c * kGhashPow;
        // every block of the lane's chain first: the loads overlap the multiplies
        gf128 x[kGhashChain];
#pragma unroll
        for (int r = 0; r < kGhashChain; ++r)
            x[r] = ghash_block<ALIGN>(s * kGhashSeg + 64 * r + lane, pad, ablocks, ad, ct, ct_bytes);
        const gf128 h64 = pw[64];
        gf128 y = x[0];
#pragma unroll 1
        for (int r = 1; r < kGhashChain; ++r) {
            y = gf128_xor(gf128_mul(y, h64), x[1]);
#pragma unroll
            for (int i = 1; i + 1 < kGhashChain; ++i) x[i] = x[i + 1];  // the next block first
        }
        y = wave_xor(gf128_mul(y, pw[64 - lane]));
        if (lane == 0) part[gw] = y;
    }
}

// the virtual block v of a client's slice as one window of it sees it: zero in front of the
// slice, outside the window, and (unless this window carries them) on the AAD blocks; the
// window's last block zero padded (a window ends off a block boundary only at ct_bytes)
template <int ALIGN>
__device__ __forceinline__ gf128 ghash_window_block(uint64_t v, uint64_t pad, uint32_t ablocks,
                                                    bool with_aad, const uint8_t *__restrict__ aad,
                                                    const uint8_t *__restrict__ win,
                                                    uint64_t first_block, uint64_t win_bytes) {
    if (v < pad) return gf128_zero();
    const uint64_t t = v - pad;
    if (t < ablocks) {
        if (!with_aad) return gf128_zero();
        const uint4 q = *reinterpret_cast<const uint4 *>(aad + 16 * t);
        return gf128_from_le_words(q.x, q.y, q.z, q.w);
    }
    const uint64_t cb = t - ablocks;
    if (cb < first_block) return gf128_zero();
    const uint64_t o = 16 * (cb - first_block);
    if (o >= win_bytes) return gf128_zero();
    const uint8_t *p = win + o;
    if (o + 16 <= win_bytes) {
        if (ALIGN == 16) {
            const uint4 q = *reinterpret_cast<const uint4 *>(p);
            return gf128_from_le_words(q.x, q.y, q.z, q.w);
        }
        if (ALIGN == 8) {
            const uint2 q0 = *reinterpret_cast<const uint2 *>(p);
            const uint2 q1 = *reinterpret_cast<const uint2 *>(p + 8);
            return gf128_from_le_words(q0.x, q0.y, q1.x, q1.y);
        }
        return gf128_from_bytes(p);
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; ++i)
        if (o + i < win_bytes) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    return gf128_from_le_words(w[0], w[1], w[2], w[3]);
}

// one wave per (client, segment s0 + j), j < ns: the bulk kernel's chain on the window's view
// of the segment; pad and P are the whole slice's
template <int ALIGN>
__global__ __launch_bounds__(256) void ghash_window_kernel(const uint8_t *__restrict__ window,
                                                           size_t stride, uint64_t first_block,
                                                           uint64_t win_bytes, uint64_t pad,
                                                           const uint8_t *__restrict__ aad,
                                                           uint32_t ablocks, bool with_aad,
                                                           const gf128 *__restrict__ pow,
                                                           gf128 *__restrict__ part, uint64_t P,
                                                           uint64_t s0, uint64_t ns, uint64_t waves) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t gw = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); gw < waves;
         gw += (uint64_t)gridDim.x * 4) {
        const uint64_t c = gw / ns, s = s0 + (gw - c * ns);
        const uint8_t *win = window + c * stride;
        const uint8_t *ad = aad + c * kGhashAadBytes;
        const gf128 *pw = pow + c * kGhashPow;
        gf128 x[kGhashChain];
#pragma unroll
        for (int r = 0; r < kGhashChain; ++r)
            x[r] = ghash_window_block<ALIGN>(s * kGhashSeg + 64 * r + lane, pad, ablocks, with_aad, ad,
                                             win, first_block, win_bytes);
        const gf128 h64 = pw[64];
        gf128 y = x[0];
#pragma unroll 1
        for (int r = 1; r < kGhashChain; ++r) {
            y = gf128_xor(gf128_mul(y, h64), x[1]);
#pragma unroll
            for (int i = 1; i + 1 < kGhashChain; ++i) x[i] = x[i + 1];  // the next block first
        }
        y = wave_xor(gf128_mul(y, pw[64 - lane]));
        if (lane == 0) part[c * P + s] = y;
    }
}

// acc ^= part, 16 bytes per lane: the ranks' partial vectors into the root's
__global__ __launch_bounds__(256) void ghash_merge_kernel(uint4 *__restrict__ acc,
                                                          const uint4 *__restrict__ part, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
        const uint4 a = acc[i], b = part[i];
        acc[i] = make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
    }
}


// EMIT: write the tag at tags + c * tag_stride (behind the ciphertext); else compare with the
// one received there (a column shard's tags lie in a buffer of their own, n x 16 bytes)
template <bool EMIT>
__global__ __launch_bounds__(64) void ghash_finish_kernel(uint8_t *__restrict__ tags, size_t tag_stride,
                                                          uint64_t ct_bytes, uint64_t aad_len,
                                                          const uint8_t *__restrict__ sub,
                                                          const gf128 *__restrict__ pow,
                                                          const gf128 *__restrict__ part, uint64_t P,
                                                          uint32_t *__restrict__ fail,
                                                          uint32_t *__restrict__ status) {
    const uint32_t lane = threadIdx.x, c = blockIdx.x;
    const gf128 *pw = pow + (size_t)c * kGhashPow, *gp = pw + 65;
    const gf128 *pc = part + (size_t)c * P;
    const uint64_t Q = (P + 63) / 64, padq = 64 * Q - P;
    const gf128 g64 = gp[64];
    gf128 y = gf128_zero();
#pragma unroll 1
    for (uint64_t q = 0; q < Q; ++q) {
        const uint64_t v = 64 * q + lane;
        gf128 x = gf128_zero();
        if (v >= padq) x = pc[v - padq];
        y = gf128_xor(gf128_mul(y, g64), x);
    }
    y = wave_xor(gf128_mul(y, gp[63 - lane]));
    y = gf128_mul(gf128_xor(y, gf128_lengths(aad_len, ct_bytes)), pw[1]);
    uint8_t *tagp = tags + (size_t)c * tag_stride;
    const uint8_t *ej0 = sub + (size_t)c * 32 + 16;
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t e = (uint32_t)ej0[4 * j] | ((uint32_t)ej0[4 * j + 1] << 8) |
                           ((uint32_t)ej0[4 * j + 2] << 16) | ((uint32_t)ej0[4 * j + 3] << 24);
        const uint32_t t = gf128_le_word(y, j) ^ e;
        if (EMIT) {
            if (lane == 0)
#pragma unroll
                for (int i = 0; i < 4; ++i) tagp[4 * j + i] = (uint8_t)(t >> (8 * i));
        } else {
            const uint32_t got = (uint32_t)tagp[4 * j] | ((uint32_t)tagp[4 * j + 1] << 8) |
                                 ((uint32_t)tagp[4 * j + 2] << 16) | ((uint32_t)tagp[4 * j + 3] << 24);
            diff |= t ^ got;
        }
    }
    if (!EMIT && lane == 0) {
        const uint32_t f = diff != 0u ? 1u : 0u;
        fail[c] = f;
        atomicOr(status, f * FLTEE_DEV_ERR_AUTH);  // every client, whatever f is
    }
}

hipError_t launch_ghash_powers(const uint8_t *sub, size_t n, void *pow, hipStream_t s) {
    if (n == 0) return hipSuccess;
    FLTEE_LAUNCH(ghash_powers_kernel, dim3((unsigned)n), dim3(64), 0, s, sub, (gf128 *)pow);
    return hipGetLastError();
}

// part_s of every (client, segment): cipher holds n slices at `stride`, ct_bytes of
// ciphertext each; aad: n x 64 bytes (zero padded); part: ghash_part_bytes()
hipError_t launch_ghash_bulk(const uint8_t *cipher, size_t n, size_t stride, size_t ct_bytes,
                             const uint8_t *aad, size_t aad_len, const void *pow, void *part,
                             hipStream_t s) {
    const uint64_t P = ghash_segments(ct_bytes, aad_len), waves = (uint64_t)n * P;
    if (waves == 0) return hipSuccess;
    uint64_t blocks = (waves + 3) / 4;
    if (blocks > 32768) blocks = 32768;  // grid-stride beyond
    const uint32_t ab = (uint32_t)((aad_len + 15) / 16);
    const int align = ((uintptr_t)cipher % 16 == 0 && stride % 16 == 0) ? 16
                    : ((uintptr_t)cipher % 8 == 0 && stride % 8 == 0)   ? 8 : 1;
    if (align == 16)
        FLTEE_LAUNCH(ghash_bulk_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, s, cipher, stride,
                     (uint64_t)ct_bytes, aad, ab, (const gf128 *)pow, (gf128 *)part, P, waves);
    else if (align == 8)
        FLTEE_LAUNCH(ghash_bulk_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, s, cipher, stride,
                     (uint64_t)ct_bytes, aad, ab, (const gf128 *)pow, (gf128 *)part, P, waves);
    else
        FLTEE_LAUNCH(ghash_bulk_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, cipher, stride,
                     (uint64_t)ct_bytes, aad, ab, (const gf128 *)pow, (gf128 *)part, P, waves);
    return hipGetLastError();
}

// the window [first_block, first_block + ceil(win_bytes / 16)) of every slice, n rows at
// `stride`: part (n x P, the whole slice's layout) = zeros but for the segments the window
// (with_aad: and the AAD blocks) touches.  The caller has checked the window against the slice.
hipError_t launch_ghash_window(const uint8_t *window, size_t n, size_t stride, size_t ct_bytes,
                               uint64_t first_block, size_t win_bytes, const uint8_t *aad,
                               size_t aad_len, bool with_aad, const void *pow, void *part,
                               hipStream_t s) {
    const uint64_t P = ghash_segments(ct_bytes, aad_len);
    if (n == 0 || P == 0) return hipSuccess;
    const hipError_t e = fl_memset_async(part, 0, n * P * sizeof(gf128), s);
    if (e != hipSuccess) return e;
    const uint32_t ab = (uint32_t)((aad_len + 15) / 16);
    const uint64_t pad = P * kGhashSeg - ((ct_bytes + 15) / 16 + ab);
    const uint64_t wb = ((uint64_t)win_bytes + 15) / 16;
    // virtual blocks [lo, hi): the window's, and in front of them the AAD's where carried
    uint64_t lo = pad + ab + first_block, hi = lo + wb;
    if (with_aad && ab) {
        if (wb == 0) lo = pad, hi = pad + ab;
        else lo = pad;  // (a window that carries the AAD away from block 0: the hull)
    }
    if (hi == lo) return hipSuccess;
    const uint64_t s0 = lo / kGhashSeg, ns = (hi - 1) / kGhashSeg - s0 + 1, waves = (uint64_t)n * ns;
    uint64_t blocks = (waves + 3) / 4;
    if (blocks > 32768) blocks = 32768;  // grid-stride beyond
    const int align = ((uintptr_t)window % 16 == 0 && stride % 16 == 0) ? 16
                    : ((uintptr_t)window % 8 == 0 && stride % 8 == 0)   ? 8 : 1;
    if (align == 16)
        FLTEE_LAUNCH(ghash_window_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, s, window, stride,
                     first_block, (uint64_t)win_bytes, pad, aad, ab, with_aad, (const gf128 *)pow,
                     (gf128 *)part, P, s0, ns, waves);
    else if (align == 8)
        FLTEE_LAUNCH(ghash_window_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, s, window, stride,
                     first_block, (uint64_t)win_bytes, pad, aad, ab, with_aad, (const gf128 *)pow,
                     (gf128 *)part, P, s0, ns, waves);
    else
        FLTEE_LAUNCH(ghash_window_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, window, stride,
                     first_block, (uint64_t)win_bytes, pad, aad, ab, with_aad, (const gf128 *)pow,
                     (gf128 *)part, P, s0, ns, waves);
    return hipGetLastError();
}

// acc ^= part over n x P partials (both 16-byte aligned)
hipError_t launch_ghash_merge(void *acc, const void *part, size_t n, size_t P, hipStream_t s) {
    const size_t n16 = n * P;
    if (n16 == 0) return hipSuccess;
    size_t blocks = (n16 + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    FLTEE_LAUNCH(ghash_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (uint4 *)acc,
                 (const uint4 *)part, n16);
    return hipGetLastError();
}

// tags: client c's tag at tags + c * tag_stride (emit: written there)
hipError_t launch_ghash_finish_tags(uint8_t *tags, size_t tag_stride, size_t n, size_t ct_bytes,
                                    size_t aad_len, const uint8_t *sub, const void *pow,
                                    const void *part, bool emit, uint32_t *fail, uint32_t *status,
                                    hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t P = ghash_segments(ct_bytes, aad_len);
    if (emit)
        FLTEE_LAUNCH(ghash_finish_kernel<true>, dim3((unsigned)n), dim3(64), 0, s, tags, tag_stride,
                     (uint64_t)ct_bytes, (uint64_t)aad_len, sub, (const gf128 *)pow,
                     (const gf128 *)part, P, fail, status);
    else
        FLTEE_LAUNCH(ghash_finish_kernel<false>, dim3((unsigned)n), dim3(64), 0, s, tags, tag_stride,
                     (uint64_t)ct_bytes, (uint64_t)aad_len, sub, (const gf128 *)pow,
                     (const gf128 *)part, P, fail, status);
    return hipGetLastError();
}

hipError_t launch_ghash_finish(uint8_t *cipher, size_t n, size_t stride, size_t ct_bytes,
                               size_t aad_len, const uint8_t *sub, const void *pow, const void *part,
                               bool emit, uint32_t *fail, uint32_t *status, hipStream_t s) {
    return launch_ghash_finish_tags(cipher + ct_bytes, stride, n, ct_bytes, aad_len, sub, pow, part,
                                    emit, fail, status, s);
}

}  // namespace fltee
