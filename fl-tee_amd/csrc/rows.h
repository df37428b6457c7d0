// rows.h — value-only dense slices: the one description of a row format (gfx950).
//
// A value row of d parameters is U = row_units(fmt, d) units of 8 bytes: the d values in
// position order, then padding up to the unit (written +0.0 by the client, ignored by every
// kernel).  n slices are n rows, row_stride(d) elements apart.
//   f32  rows (FLTEE_OPT_PACKED): 2 values a unit.
//   bf16 rows (FLTEE_OPT_BF16)  : 4 little-endian halves a unit; widening is exact for every
//        bit pattern (f32 bits = (uint32)h << 16).  The halves stay packed while in flight
//        and are widened at the add.
// Host code takes the format as a RowFmt; a kernel takes it as a tag type (RowF32, RowBf16):
// the element type, the stride rule, a W-wide non-temporal load into raw dwords, value(raw,
// w), and the scalar widen / narrow.  rows_width is the alignment -> W rule and rows_store
// the epilogue that k_rows.hip's accumulate and k_trim.hip's trimmed mean share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fltee {

enum RowFmt { kRowsNone = 0, kRowsF32, kRowsBf16 };

constexpr size_t rows_per_unit(RowFmt f) { return f == kRowsBf16 ? 4 : 2; }
constexpr size_t rows_elem_bytes(RowFmt f) { return 8 / rows_per_unit(f); }
// the only place that rounds d up
constexpr size_t row_units(RowFmt f, size_t d) { return (d + rows_per_unit(f) - 1) / rows_per_unit(f); }
// the shortest row a format answers to: below it a slice has the size of a record (d = 1) or,
// bf16, of an f32 slice (d = 2); from there the sizes differ
constexpr size_t rows_min_d(RowFmt f) { return f == kRowsBf16 ? 3 : 2; }
// bf16 rows take their widest group (8 outputs, a 16-byte load) only from here on: below,
// too few waves for fewer loads each (A/B: profiles/r13/bf16.jsonl)
constexpr size_t kBf16SmallD = (size_t)1 << 19;

// The alignment -> W rule: the outputs a lane owns.  W elements are one load of the row
// (its base and every row W elements aligned) and one store of 4 W bytes, in 16-byte pieces
// from W = 4 on; the widest group of a format is a 16-byte load.  (Rows are always 8-byte
// multiples apart: stride % W only decides the 16-byte load.)
static inline int rows_width(RowFmt f, const void *rows, const void *out, size_t stride, size_t d) {
    const uintptr_t a = (uintptr_t)rows, b = (uintptr_t)out;
    const size_t es = rows_elem_bytes(f), wmax = 16 / es;
    int W = 1;
    for (size_t w = 2; w <= wmax; w *= 2) {
        if (f == kRowsBf16 && w == wmax && d < kBf16SmallD) break;
        if (a % (w * es) == 0 && b % (w < 4 ? w * 4 : 16) == 0 && stride % w == 0) W = (int)w;
    }
    return W;
}

typedef uint32_t rows_u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t rows_u32x2_t __attribute__((ext_vector_type(2)));
typedef float rows_f32x4_t __attribute__((ext_vector_type(4)));
typedef float rows_f32x2_t __attribute__((ext_vector_type(2)));

// BYTES (2, 4, 8 or 16) at p, aligned to BYTES, as they lie in memory: one non-temporal load
template <int BYTES>
static __device__ __forceinline__ void rows_load(const void *p, uint32_t (&r)[(BYTES + 3) / 4]) {
    if constexpr (BYTES == 2) {
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
};

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
