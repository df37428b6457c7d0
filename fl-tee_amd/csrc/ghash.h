// ghash.h — GF(2^128) arithmetic of GCM (NIST SP 800-38D), constant time, host and device.
//
// One element is four 32-bit words in NATURAL bit order: bit i of w[j] is the coefficient
// of x^(32 j + i).  GCM's own byte order is reflected (the coefficient of x^0 is the most
// significant bit of byte 0), so a 16-byte block enters as w[j] = bitreverse(BE32(bytes
// 4 j .. 4 j + 3)) — one byte swap and one bit reverse per word — and leaves the same way.
//
// gf128_mul is the only multiply in the library: the kernels of k_ghash.hip and the host
// tag of fltee_debug_gcm_tag_host run this one function.  gfx950 has no carry-less multiply,
// so a 32 x 32 carry-less product is built from integer multiplies "with holes": each
// operand is cut into four words that keep every fourth bit; in the integer product of two
// such words every fourth bit receives at most eight partial products, whose count stays
// inside the three empty bits above it, so the kept bit is their parity — the carry-less
// product bit.  16 integer multiplies give the low 32 bits; the high 31 bits are the low
// bits of the product of the bit-reversed operands, reversed back.  A 128 x 128 product is
// two levels of Karatsuba: 9 of those 64-bit products = 18 x 16 = 288 v_mul_lo_u32, then the
// fold by x^128 = x^7 + x^2 + x + 1.  No table, no branch, no address depends on the
// operands.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#endif

namespace fltee {

struct gf128 {
    uint32_t w[4];
};

__host__ __device__ __forceinline__ uint32_t rev32(uint32_t x) { return __builtin_bitreverse32(x); }

// low 32 bits of the carry-less product x (*) y
__host__ __device__ __forceinline__ uint32_t bmul32(uint32_t x, uint32_t y) {
    const uint32_t x0 = x & 0x11111111u, x1 = x & 0x22222222u, x2 = x & 0x44444444u,
                   x3 = x & 0x88888888u;
    const uint32_t y0 = y & 0x11111111u, y1 = y & 0x22222222u, y2 = y & 0x44444444u,
                   y3 = y & 0x88888888u;
    const uint32_t z0 = (x0 * y0) ^ (x1 * y3) ^ (x2 * y2) ^ (x3 * y1);
    const uint32_t z1 = (x0 * y1) ^ (x1 * y0) ^ (x2 * y3) ^ (x3 * y2);
    const uint32_t z2 = (x0 * y2) ^ (x1 * y1) ^ (x2 * y0) ^ (x3 * y3);
    const uint32_t z3 = (x0 * y3) ^ (x1 * y2) ^ (x2 * y1) ^ (x3 * y0);
    return (z0 & 0x11111111u) | (z1 & 0x22222222u) | (z2 & 0x44444444u) | (z3 & 0x88888888u);
}

// the 63-bit carry-less product x (*) y: bit k of rev(x) (*) rev(y) is bit 62 - k of it
__host__ __device__ __forceinline__ void clmul32(uint32_t x, uint32_t y, uint32_t &lo, uint32_t &hi) {
    lo = bmul32(x, y);
    hi = rev32(bmul32(rev32(x), rev32(y))) >> 1;
}

// (a0 + a1 X)(b0 + b1 X), X = x^32: three products
__host__ __device__ __forceinline__ void clmul64(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1,
                                                 uint32_t r[4]) {
    uint32_t l0, l1, h0, h1, m0, m1;
    clmul32(a0, b0, l0, l1);
    clmul32(a1, b1, h0, h1);
    clmul32(a0 ^ a1, b0 ^ b1, m0, m1);
    m0 ^= l0 ^ h0;
    m1 ^= l1 ^ h1;
    r[0] = l0;
    r[1] = l1 ^ m0;
    r[2] = h0 ^ m1;
    r[3] = h1;
}

__host__ __device__ __forceinline__ gf128 gf128_mul(const gf128 &a, const gf128 &b) {
    uint32_t L[4], H[4], M[4], p[8];
    clmul64(a.w[0], a.w[1], b.w[0], b.w[1], L);
    clmul64(a.w[2], a.w[3], b.w[2], b.w[3], H);
    clmul64(a.w[0] ^ a.w[2], a.w[1] ^ a.w[3], b.w[0] ^ b.w[2], b.w[1] ^ b.w[3], M);
#pragma unroll
    for (int i = 0; i < 4; ++i) M[i] ^= L[i] ^ H[i];
    p[0] = L[0];
    p[1] = L[1];
    p[2] = L[2] ^ M[0];
    p[3] = L[3] ^ M[1];
    p[4] = H[0] ^ M[2];
    p[5] = H[1] ^ M[3];
    p[6] = H[2];
    p[7] = H[3];
    // x^128 = x^7 + x^2 + x + 1: word 4 + j folds into words j and j + 1, top word first
#pragma unroll
    for (int j = 3; j >= 0; --j) {
        const uint32_t v = p[4 + j];
        p[j] ^= v ^ (v << 1) ^ (v << 2) ^ (v << 7);
        p[j + 1] ^= (v >> 31) ^ (v >> 30) ^ (v >> 25);
    }
    gf128 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = p[i];
    return r;
}

__host__ __device__ __forceinline__ gf128 gf128_xor(const gf128 &a, const gf128 &b) {
    gf128 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = a.w[i] ^ b.w[i];
    return r;
}

__host__ __device__ __forceinline__ gf128 gf128_zero() { return gf128{{0u, 0u, 0u, 0u}}; }
__host__ __device__ __forceinline__ gf128 gf128_one() { return gf128{{1u, 0u, 0u, 0u}}; }

// a block's four words as loaded little-endian <-> the element
__host__ __device__ __forceinline__ gf128 gf128_from_le_words(uint32_t a, uint32_t b, uint32_t c,
                                                              uint32_t d) {
    return gf128{{rev32(__builtin_bswap32(a)), rev32(__builtin_bswap32(b)),
                  rev32(__builtin_bswap32(c)), rev32(__builtin_bswap32(d))}};
}
__host__ __device__ __forceinline__ uint32_t gf128_le_word(const gf128 &x, int j) {
    return __builtin_bswap32(rev32(x.w[j]));
}
__host__ __device__ __forceinline__ gf128 gf128_from_bytes(const uint8_t *p) {
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        v[j] = (uint32_t)p[4 * j] | ((uint32_t)p[4 * j + 1] << 8) | ((uint32_t)p[4 * j + 2] << 16) |
               ((uint32_t)p[4 * j + 3] << 24);
    return gf128_from_le_words(v[0], v[1], v[2], v[3]);
}

// the closing block BE64(8 |AAD|) || BE64(8 |C|)
__host__ __device__ __forceinline__ gf128 gf128_lengths(uint64_t aad_bytes, uint64_t ct_bytes) {
    const uint64_t a = aad_bytes * 8, c = ct_bytes * 8;
    return gf128{{rev32((uint32_t)(a >> 32)), rev32((uint32_t)a), rev32((uint32_t)(c >> 32)),
                  rev32((uint32_t)c)}};
}

}  // namespace fltee
