// rows.h — value-only dense slices: the one description of a row format (gfx950).
//
// A value row of d parameters is U = row_units(fmt, d) units of 8 bytes: the d values in
// position order, then padding up to the unit (written +0.0 by the client, ignored by every
// kernel).  n slices are n rows, row_stride(d) elements apart.
//   f32  rows (FLTEE_OPT_PACKED): 2 values a unit.
//   bf16 rows (FLTEE_OPT_BF16)  : 4 little-endian halves a unit; widening is exact for every
//        bit pattern (f32 bits = (uint32)h << 16).  The halves stay packed while in flight
//        and are widened at the add.
//   fp8  rows (FLTEE_OPT_FP8)   : 8 OCP e4m3fn codes a unit, and one unit more behind the
//        values: the client's f32 scale s, then 4 ignored bytes.  A code widens exactly
//        (w(q), integer ops and selects: no branch and no address depends on a value) and
//        x = __fmul_rn(w(q), s) is the value — the one rounding the format adds.  The scale
//        lies at the fixed element row_scale_at(d) of its row: a function of d alone.
// Host code takes the format as a RowFmt; a kernel takes it as a tag type (RowF32, RowBf16,
// RowFp8): the element type, the stride rule, a W-wide non-temporal load into raw dwords,
// value(raw, w), the scalar widen / narrow, and kScaled with scale(row, stride) for a format
// that carries a per-row scale.  rows_width is the alignment -> W rule and rows_store
// the epilogue that k_rows.hip's accumulate and k_trim.hip's trimmed mean share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fltee {

enum RowFmt { kRowsNone = 0, kRowsF32, kRowsBf16, kRowsFp8 };

constexpr size_t rows_per_unit(RowFmt f) { return f == kRowsFp8 ? 8 : f == kRowsBf16 ? 4 : 2; }
constexpr size_t rows_elem_bytes(RowFmt f) { return 8 / rows_per_unit(f); }
// units behind the values: the fp8 trailer (f32 scale, 4 ignored bytes)
constexpr size_t rows_trailer_units(RowFmt f) { return f == kRowsFp8 ? 1 : 0; }
// the only place that rounds d up
constexpr size_t row_units(RowFmt f, size_t d) {
    return (d + rows_per_unit(f) - 1) / rows_per_unit(f) + rows_trailer_units(f);
}
// the shortest row a format answers to: below it a slice has the size of a record (d = 1) or,
// bf16, of an f32 slice (d = 2); from there the sizes differ.  fp8: P + 1 units, P = ceil(d / 8),
// against bf16's Q = ceil(d / 4).  Q >= 2 P - 1, so Q > P + 1 as soon as P >= 3 (d >= 17); P = 2
// (d = 9..16) has Q = 3 = P + 1 for d <= 12 and Q = 4 from d = 13; P = 1 (d <= 8) has P + 1 = 2 =
// Q at d = 5..8 and more units than Q below.  So 13 is the smallest d from which every fp8 slice
// differs from the bf16 slice; f32 slices (ceil(d / 2)) and records (d) are larger there.
constexpr size_t rows_min_d(RowFmt f) { return f == kRowsFp8 ? 13 : f == kRowsBf16 ? 3 : 2; }
// bf16 rows take their widest group (8 outputs, a 16-byte load) only from here on: below,
// too few waves for fewer loads each (A/B: profiles/r13/bf16.jsonl)
constexpr size_t kBf16SmallD = (size_t)1 << 19;
// fp8 rows are decoded, not just loaded: the accumulate waits for the vector ALU, and what it
// wants is waves.  Below kFp8SmallD outputs a lane owns one output; from there on up to 4 (a
// 4-byte load).  8 outputs tie with 4 at 100 x 1M and lose below; 16 (a 16-byte load) lose
// everywhere (A/B at 50,888 / 50,890 / 262,152 / 1,000,000 / 1,000,008 outputs:
// profiles/r16/fp8.jsonl; the crossing of 1 and 4 outputs a lane lies between 262,152 and 10^6)
constexpr size_t kFp8SmallD = (size_t)1 << 19;
// the widest group a format ships at d outputs
constexpr size_t rows_max_width(RowFmt f, size_t d) {
    return f == kRowsFp8 ? (d < kFp8SmallD ? 1 : 4) : f == kRowsBf16 ? (d < kBf16SmallD ? 4 : 8) : 4;
}

// The alignment -> W rule: the outputs a lane owns.  W elements are one load of the row
// (its base and every row W elements aligned) and one store of 4 W bytes, in 16-byte pieces
// from W = 4 on; the widest group of f32 and bf16 rows is a 16-byte load, of fp8 rows a 4-byte
// load (rows_max_width).  (Rows are always 8-byte
// multiples apart: stride % W only decides the 16-byte load.)
static inline int rows_width(RowFmt f, const void *rows, const void *out, size_t stride, size_t d) {
    const uintptr_t a = (uintptr_t)rows, b = (uintptr_t)out;
    const size_t es = rows_elem_bytes(f), wmax = rows_max_width(f, d);
    int W = 1;
    for (size_t w = 2; w <= wmax; w *= 2) {
        if (a % (w * es) == 0 && b % (w < 4 ? w * 4 : 16) == 0 && stride % w == 0) W = (int)w;
    }
    return W;
}

typedef uint32_t rows_u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t rows_u32x2_t __attribute__((ext_vector_type(2)));
typedef float rows_f32x4_t __attribute__((ext_vector_type(4)));
typedef float rows_f32x2_t __attribute__((ext_vector_type(2)));

// BYTES (1, 2, 4, 8 or 16) at p, aligned to BYTES, as they lie in memory: one non-temporal load
template <int BYTES>
static __device__ __forceinline__ void rows_load(const void *p, uint32_t (&r)[(BYTES + 3) / 4]) {
    if constexpr (BYTES == 1) {
        r[0] = __builtin_nontemporal_load(reinterpret_cast<const uint8_t *>(p));
    } else if constexpr (BYTES == 2) {
        r[0] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(p));
    } else if constexpr (BYTES == 4) {
        r[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p));
    } else {
        typedef typename std::conditional<BYTES == 16, rows_u32x4_t, rows_u32x2_t>::type V;
        const V v = __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
#pragma unroll
        for (int w = 0; w < BYTES / 4; ++w) r[w] = v[w];
    }
}

struct RowF32 {
    typedef float elem;
    static constexpr RowFmt kFmt = kRowsF32;
    static constexpr size_t row_stride(size_t d) { return row_units(kFmt, d) * rows_per_unit(kFmt); }
    template <int W> static constexpr int raw_words() { return W; }
    template <int W>
    static __device__ __forceinline__ void load(const elem *p, uint32_t (&r)[W]) { rows_load<4 * W>(p, r); }
    template <int W>
    static __device__ __forceinline__ float value(const uint32_t (&r)[W], int w) { return __uint_as_float(r[w]); }
    static __device__ __forceinline__ float widen(elem e) { return e; }
    static __device__ __forceinline__ elem narrow(float x) { return x; }
    static constexpr bool kScaled = false;
};

struct RowBf16 {
    typedef uint16_t elem;
    static constexpr RowFmt kFmt = kRowsBf16;
    static constexpr size_t row_stride(size_t d) { return row_units(kFmt, d) * rows_per_unit(kFmt); }
    template <int W> static constexpr int raw_words() { return (W + 1) / 2; }
    // half w in the low (w even) or high (w odd) 16 bits of dword w / 2
    template <int W>
    static __device__ __forceinline__ void load(const elem *p, uint32_t (&r)[(W + 1) / 2]) { rows_load<2 * W>(p, r); }
    template <int W>
    static __device__ __forceinline__ float value(const uint32_t (&r)[(W + 1) / 2], int w) {
        return __uint_as_float((w & 1) ? r[w / 2] & 0xFFFF0000u : r[w / 2] << 16);
    }
    static __device__ __forceinline__ float widen(elem e) { return __uint_as_float((uint32_t)e << 16); }
    // f32 -> bf16 in integer ops: round to nearest even (values just under FLT_MAX round to
    // inf); a NaN keeps its sign and its upper payload and is quieted
    static __device__ __forceinline__ elem narrow(float x) {
        const uint32_t u = __float_as_uint(x);
        if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
        return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    }
    static constexpr bool kScaled = false;
};

// OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities, S.1111.111 is NaN,
// the largest finite value 448 (0x7E), the smallest subnormal 2^-9.
struct RowFp8 {
    typedef uint8_t elem;
    static constexpr RowFmt kFmt = kRowsFp8;
    static constexpr size_t row_stride(size_t d) { return row_units(kFmt, d) * rows_per_unit(kFmt); }
    template <int W> static constexpr int raw_words() { return (W + 3) / 4; }
    // code w in byte w % 4 of dword w / 4
    template <int W>
    static __device__ __forceinline__ void load(const elem *p, uint32_t (&r)[(W + 3) / 4]) { rows_load<W>(p, r); }
    // w(q), exact, in integer ops and selects.  A normal code's 7 magnitude bits are an f32's
    // exponent and top mantissa bits 120 exponents lower; a subnormal code is m * 2^-9 (an exact
    // conversion and an exact product); the NaN code gives the quiet NaN 0x7FC00000.
    static __device__ __forceinline__ float widen(elem e) {
        const uint32_t q = e, mag = q & 0x7Fu;
        const uint32_t normal = (mag << 20) + (120u << 23);
        const uint32_t sub = __float_as_uint(__fmul_rn((float)(int)(q & 7u), 0.001953125f));
        uint32_t b = mag < 8u ? sub : normal;
        b = mag == 0x7Fu ? 0x7FC00000u : b;
        return __uint_as_float(b | ((q & 0x80u) << 24));
    }
    template <int W>
    static __device__ __forceinline__ float value(const uint32_t (&r)[(W + 3) / 4], int w) {
        return widen((elem)((r[w / 4] >> (8 * (w & 3))) & 0xFFu));
    }
    // y (the value already divided by the row's scale) -> the code: NaN -> sign | 0x7F; |y| > 448
    // (+-inf too) -> sign | 0x7E; else the nearest e4m3 magnitude, ties to the even code.  From
    // 2^-6 on that is round-to-nearest-even of the f32's low 20 mantissa bits (a carry moves
    // into the exponent as it should); below, |y| * 2^9 (exact) rounded to an integer 0..8 by
    // the adder (+ 2^23), which is the code itself (8 = 0x08 = 2^-6).
    static __device__ __forceinline__ elem narrow(float y) {
        const uint32_t u = __float_as_uint(y), mag = u & 0x7FFFFFFFu;
        const uint32_t normal = ((mag + 0x7FFFFu + ((mag >> 20) & 1u)) >> 20) - (120u << 3);
        const uint32_t sub = __float_as_uint(__fadd_rn(__fmul_rn(__uint_as_float(mag), 512.0f), 8388608.0f)) & 0xFu;
        uint32_t q = mag < 0x3C800000u ? sub : normal;  // 2^-6
        q = mag > 0x43E00000u ? 0x7Eu : q;              // 448
        q = mag > 0x7F800000u ? 0x7Fu : q;
        return (elem)(q | (u >> 31 << 7));
    }
    // the per-row scale: the f32 at the fixed element 8 P = stride - 8 of the row (4-byte
    // aligned: rows are 8-byte multiples apart and their base is 4-byte aligned)
    static constexpr bool kScaled = true;
    static __device__ __forceinline__ float scale(const elem *row, size_t stride) {
        return *reinterpret_cast<const float *>(row + stride - 8);
    }
};

// widen(e) under the row's scale s (a format without one: widen alone; s is not read)
template <class F>
static __device__ __forceinline__ float rows_scaled(float w, float s) {
    if constexpr (F::kScaled) return __fmul_rn(w, s);
    else return w;
}

// The epilogue of a lane that owns outputs [j0, j0 + W): out = acc * coef, or out += acc.  A
// whole group is stored in pieces of at most 16 bytes (out is aligned for them: rows_width);
// the group that reaches past d takes the scalar d tail, where the columns past d — the
// row's padding — are dropped.
template <int W>
static __device__ __forceinline__ void rows_store(float *out, size_t j0, size_t d,
                                                  const float (&acc)[W], float coef, bool accumulate) {
    float *o = out + j0;
    if constexpr (W > 1) {
        if (j0 + W <= d) {
            constexpr int SW = W >= 4 ? 4 : 2;
            typedef typename std::conditional<SW == 4, rows_f32x4_t, rows_f32x2_t>::type V;
#pragma unroll
            for (int g = 0; g < W / SW; ++g) {
                V r;
                if (accumulate) {
                    const V prev = *reinterpret_cast<const V *>(o + g * SW);
#pragma unroll
                    for (int w = 0; w < SW; ++w) r[w] = __fadd_rn(prev[w], acc[g * SW + w]);
                } else {
#pragma unroll
                    for (int w = 0; w < SW; ++w) r[w] = __fmul_rn(acc[g * SW + w], coef);
                }
                *reinterpret_cast<V *>(o + g * SW) = r;
            }
            return;
        }
    }
#pragma unroll
    for (int w = 0; w < W; ++w)
        if (j0 + w < d) o[w] = accumulate ? __fadd_rn(o[w], acc[w]) : __fmul_rn(acc[w], coef);
}

}  // namespace fltee
