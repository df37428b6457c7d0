// k_rows.hip — value-only dense uploads (gfx950): f32 rows at half the bytes of records
// (FLTEE_OPT_PACKED), bf16 rows at a quarter (FLTEE_OPT_BF16), fp8 rows with a per-row f32 scale
// at an eighth (FLTEE_OPT_FP8).  rows.h describes the three formats; every body here is written
// once over that description, and the __global__ entry points below only name a format (their
// names are what the launch trace and a profiler show).
//
// rows_accumulate (dense_accumulate_p / _h / _q): k_accumulate.hip's dense_accumulate_v on value
//   rows, under the same contract: out[j] = the in-order client sum ((+0.0 + v_0[j]) +
//   v_1[j]) + ... with __fadd_rn over the (exactly widened) values, then * coef (or out +=
//   with ACC; per-client clip coefficients with CLIP, v * cc rounded before the add as on the
//   records route).  A lane owns W adjacent outputs and issues one non-temporal load of W
//   elements per client, UC clients in flight; the clients past the last full batch go out as
//   one more batch whose loads and adds are guarded by c + u < n (a wave-uniform test of the
//   public n: the loads still issue back to back, no row is read twice).  Every element is
//   read once at a fixed address: the access pattern depends on (n, d) and the pointers'
//   alignment only.  There is no index, so there is no status word.  W by rows_width: the
//   widest group the row base, the out base and the stride are aligned for — f32: 4 on 16
//   bytes (U even), 2 on 8 (U odd — MLP-MNIST: d = 50,890, U = 25,445 — or a base at 8 mod
//   16: the survivors buffer can land there), 1 below; bf16: 8 on 16 bytes and a large d, 4 on
//   8, 2 on 4, 1 (a scalar 2-byte load) below; fp8: 1 at a small d, else 4 on 4 bytes (out on 16),
//   and 2 or 1 where the out base is off.  The lanes of the last group past d never
//   store: the padding reaches no output.  A format with a per-row scale (fp8) reads it at the
//   fixed element stride - 8 of the client's row — a wave-uniform load, once per client per lane
//   group — and multiplies the widened value by it before the clip coefficient: two roundings.
// rows_norm (packed_norm_kernel / bf16_norm_kernel): client_norm_kernel (k_dp.hip) on a value
//   row: the same f64 sum of squares in the same lane order over the d widened values, so
//   CLIP takes the same coefficients.
// rows_unpack (unpack_dense_kernel / unpack_bf16_kernel): rows -> records (j, widen(v[j]))
//   (launch_client_dense with a row stride); rows_pack (pack_dense_kernel / pack_bf16_kernel):
//   the client producer, f32 values [n][d] -> rows, narrowed by the format (f32: as they are;
//   bf16: round to nearest even in integer ops), padding +0.0.
#include "common.h"

namespace fltee {

// stride: elements between rows; lane j0 / W owns outputs [j0, j0 + W) — where W > 1 the
// group of the last lane may reach past d into the row's padding (j0 + W <= stride holds:
// stride is a multiple of W on the paths that take W), never past the row.
template <class F, int W, int UC, bool CLIP, bool ACC>
static __device__ __forceinline__ void rows_accumulate(size_t j0, const typename F::elem *rows,
                                                       size_t stride, size_t d, uint32_t n, float coef,
                                                       float *out,
                                                       const float *ccoef) {
    if (j0 >= d) return;
    constexpr int R = F::template raw_words<W>();
    const typename F::elem *p = rows + j0;
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0.0f;
    uint32_t c = 0;
    for (; c + UC <= n; c += UC) {
        uint32_t x[UC][R];
        float sc[UC];
#pragma unroll
        for (int u = 0; u < UC; ++u) F::template load<W>(p + (size_t)(c + u) * stride, x[u]);
        if constexpr (F::kScaled) {
#pragma unroll
            for (int u = 0; u < UC; ++u) sc[u] = F::scale(rows + (size_t)(c + u) * stride, stride);
        }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const float cc = CLIP ? ccoef[c + u] : 1.0f;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float q = F::template value<W>(x[u], w);
                const float v = F::kScaled ? __fmul_rn(q, sc[u]) : q;  // (before the clip: two roundings)
                acc[w] = __fadd_rn(acc[w], CLIP ? __fmul_rn(v, cc) : v);
            }
        }
    }
    if (c < n) {  // the n tail: one guarded batch (wave-uniform tests of the public n)
        uint32_t x[UC][R];
        float sc[UC];
#pragma unroll
        for (int u = 0; u < UC; ++u)
            if (c + u < n) F::template load<W>(p + (size_t)(c + u) * stride, x[u]);
        if constexpr (F::kScaled) {
#pragma unroll
            for (int u = 0; u < UC; ++u)
                if (c + u < n) sc[u] = F::scale(rows + (size_t)(c + u) * stride, stride);
        }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (c + u < n) {
                const float cc = CLIP ? ccoef[c + u] : 1.0f;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const float q = F::template value<W>(x[u], w);
                    const float v = F::kScaled ? __fmul_rn(q, sc[u]) : q;  // (before the clip: two roundings)
                    acc[w] = __fadd_rn(acc[w], CLIP ? __fmul_rn(v, cc) : v);
                }
            }
        }
    }
    rows_store<W>(out, j0, d, acc, coef, ACC);
}

// client_norm_kernel's sums, lane for lane: thread t takes values t, t + 256, ...
template <class F>
static __device__ __forceinline__ void rows_norm(const typename F::elem *rows, size_t stride,
                                                 size_t d, float clipping, float *coef) {
    __shared__ double part[4];
    const typename F::elem *src = rows + (size_t)blockIdx.x * stride;
    float s = 1.0f;
    if constexpr (F::kScaled) s = F::scale(src, stride);
    double ss = 0.0;
    for (size_t e = threadIdx.x; e < d; e += 256) {
        const double v = (double)rows_scaled<F>(F::widen(src[e]), s);
        ss += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = part[0] + part[1] + part[2] + part[3];
        const float norm = (float)sqrt(t);
        float cf = clipping / norm;
        if (!(cf < 1.0f)) cf = 1.0f;  // Python min(1, tensor): NaN / inf / >=1 -> 1
        coef[blockIdx.x] = cf;
    }
}

template <class F>
static __device__ __forceinline__ void rows_unpack(const typename F::elem *rows, size_t n, size_t d,
                                                   size_t stride, uint64_t *rec) {
    const size_t total = n * d;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t c = t / d, i = t - c * d;
        float s = 1.0f;
        if constexpr (F::kScaled) s = F::scale(rows + c * stride, stride);
        rec[t] = make_rec((uint32_t)i, rows_scaled<F>(F::widen(rows[c * stride + i]), s));
    }
}

template <class F>
static __device__ __forceinline__ void rows_pack(const float *values, size_t n, size_t d,
                                                 size_t stride, typename F::elem *rows) {
    const size_t total = n * stride;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t c = t / stride, i = t - c * stride;
        rows[t] = i < d ? F::narrow(values[c * d + i]) : (typename F::elem)0;
    }
}

// The fp8 producer, two launches.  fp8_scale_kernel (a block a client): a = the largest finite
// |v| of the row — a maximum over the bit patterns, so the order it is taken in changes nothing
// — and s = a / 448 (f32, RN) where that is a normal, nonzero f32, else 1.  fp8_quantise_kernel:
// a thread a byte of the row — the code of v / s (f32, RN), 0x00 padding up to 8 P, then the
// trailer: s little-endian and 4 zero bytes.
static __device__ __forceinline__ void fp8_row_scale(const float *values, size_t d, float *scale) {
    __shared__ uint32_t part[4];
    const float *src = values + (size_t)blockIdx.x * d;
    uint32_t m = 0;
    for (size_t e = threadIdx.x; e < d; e += 256) {
        const uint32_t a = __float_as_uint(src[e]) & 0x7FFFFFFFu;
        m = a < 0x7F800000u && a > m ? a : m;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_down((int)m, o, 64);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) m = part[w] > m ? part[w] : m;
        const float q = __fdiv_rn(__uint_as_float(m), 448.0f);
        scale[blockIdx.x] = __float_as_uint(q) >= 0x00800000u ? q : 1.0f;  // (a is finite: so is q)
    }
}

static __device__ __forceinline__ void fp8_row_quantise(const float *values, const float *scale, size_t n,
                                                        size_t d, size_t stride, uint8_t *rows) {
    const size_t total = n * stride;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t c = t / stride, i = t - c * stride;
        const float s = scale[c];
        uint8_t b = 0;
        if (i < d) b = RowFp8::narrow(__fdiv_rn(values[c * d + i], s));
        else if (i >= stride - 8 && i < stride - 4) b = (uint8_t)(__float_as_uint(s) >> (8 * (i - (stride - 8))));
        rows[t] = b;
    }
}

// ---- the entry points: a format each, nothing else ------------------------------------
template <int W, int UC, bool CLIP, bool ACC, int NTH>
__global__ __launch_bounds__(NTH) void dense_accumulate_p(const float *__restrict__ pk, size_t stride,
                                                          size_t d, uint32_t n, float coef,
                                                          float *__restrict__ out,
                                                          const float *__restrict__ ccoef) {
    rows_accumulate<RowF32, W, UC, CLIP, ACC>(((size_t)blockIdx.x * NTH + threadIdx.x) * W, pk, stride, d, n,
                                              coef, out, ccoef);
}
template <int W, int UC, bool CLIP, bool ACC, int NTH>
__global__ __launch_bounds__(NTH) void dense_accumulate_h(const uint16_t *__restrict__ rows, size_t stride,
                                                          size_t d, uint32_t n, float coef,
                                                          float *__restrict__ out,
                                                          const float *__restrict__ ccoef) {
    rows_accumulate<RowBf16, W, UC, CLIP, ACC>(((size_t)blockIdx.x * NTH + threadIdx.x) * W, rows, stride, d, n,
                                               coef, out, ccoef);
}
template <int W, int UC, bool CLIP, bool ACC, int NTH>
__global__ __launch_bounds__(NTH) void dense_accumulate_q(const uint8_t *__restrict__ rows, size_t stride,
                                                          size_t d, uint32_t n, float coef,
                                                          float *__restrict__ out,
                                                          const float *__restrict__ ccoef) {
    rows_accumulate<RowFp8, W, UC, CLIP, ACC>(((size_t)blockIdx.x * NTH + threadIdx.x) * W, rows, stride, d, n,
                                              coef, out, ccoef);
}
__global__ __launch_bounds__(256) void packed_norm_kernel(const float *__restrict__ pk, size_t stride,
                                                          size_t d, float clipping,
                                                          float *__restrict__ coef) {
    rows_norm<RowF32>(pk, stride, d, clipping, coef);
}
__global__ __launch_bounds__(256) void bf16_norm_kernel(const uint16_t *__restrict__ rows, size_t stride,
                                                        size_t d, float clipping,
                                                        float *__restrict__ coef) {
    rows_norm<RowBf16>(rows, stride, d, clipping, coef);
}
__global__ __launch_bounds__(256) void fp8_norm_kernel(const uint8_t *__restrict__ rows, size_t stride,
                                                       size_t d, float clipping,
                                                       float *__restrict__ coef) {
    rows_norm<RowFp8>(rows, stride, d, clipping, coef);
}
__global__ void unpack_dense_kernel(const float *__restrict__ pk, size_t n, size_t d, size_t stride,
                                    uint64_t *__restrict__ rec) {
    rows_unpack<RowF32>(pk, n, d, stride, rec);
}
__global__ void unpack_bf16_kernel(const uint16_t *__restrict__ rows, size_t n, size_t d, size_t stride,
                                   uint64_t *__restrict__ rec) {
    rows_unpack<RowBf16>(rows, n, d, stride, rec);
}
__global__ void unpack_fp8_kernel(const uint8_t *__restrict__ rows, size_t n, size_t d, size_t stride,
                                  uint64_t *__restrict__ rec) {
    rows_unpack<RowFp8>(rows, n, d, stride, rec);
}
__global__ void pack_dense_kernel(const float *__restrict__ values, size_t n, size_t d, size_t stride,
                                  float *__restrict__ pk) {
    rows_pack<RowF32>(values, n, d, stride, pk);
}
__global__ void pack_bf16_kernel(const float *__restrict__ values, size_t n, size_t d, size_t stride,
                                 uint16_t *__restrict__ rows) {
    rows_pack<RowBf16>(values, n, d, stride, rows);
}

__global__ __launch_bounds__(256) void fp8_scale_kernel(const float *__restrict__ values, size_t d,
                                                        float *__restrict__ scale) {
    fp8_row_scale(values, d, scale);
}
__global__ void fp8_quantise_kernel(const float *__restrict__ values, const float *__restrict__ scale, size_t n,
                                    size_t d, size_t stride, uint8_t *__restrict__ rows) {
    fp8_row_quantise(values, scale, n, d, stride, rows);
}

// ---- the shipped launch shapes ---------------------------------------------------------
struct AccArgs {
    const void *rows;
    size_t stride, n, d;
    float coef;
    float *out;
    const float *ccoef;
    hipStream_t s;
};
static unsigned acc_blocks(size_t d, int W, int NTH) { return (unsigned)(((d + W - 1) / W + NTH - 1) / NTH); }

template <int W, int UC, bool CLIP, bool ACC, int NTH>
static void launch_p(const AccArgs &a) {
    FLTEE_LAUNCH((dense_accumulate_p<W, UC, CLIP, ACC, NTH>), dim3(acc_blocks(a.d, W, NTH)), dim3(NTH), 0, a.s,
                 (const float *)a.rows, a.stride, a.d, (uint32_t)a.n, a.coef, a.out, a.ccoef);
}
template <int W, int UC, bool CLIP, bool ACC, int NTH>
static void launch_h(const AccArgs &a) {
    FLTEE_LAUNCH((dense_accumulate_h<W, UC, CLIP, ACC, NTH>), dim3(acc_blocks(a.d, W, NTH)), dim3(NTH), 0, a.s,
                 (const uint16_t *)a.rows, a.stride, a.d, (uint32_t)a.n, a.coef, a.out, a.ccoef);
}
template <int W, int UC, bool CLIP, bool ACC, int NTH>
static void launch_q(const AccArgs &a) {
    FLTEE_LAUNCH((dense_accumulate_q<W, UC, CLIP, ACC, NTH>), dim3(acc_blocks(a.d, W, NTH)), dim3(NTH), 0, a.s,
                 (const uint8_t *)a.rows, a.stride, a.d, (uint32_t)a.n, a.coef, a.out, a.ccoef);
}

// Every shape computes the same adds in the same order: the same bits.  The A/B runs that
// chose these are recorded in profiles/r11/packed.jsonl and profiles/r13/bf16.jsonl, not
// kept in the code.
//
// f32 rows.  Fewer than kPackedSmallD outputs: too few waves for 16 loads a lane to cover the
// HBM latency (MLP-MNIST: 25,445 pairs = 398 waves for 1,024 SIMDs), so a lane keeps 64
// clients in flight instead — 64 x 4 W bytes of registers, what dense_accumulate_w spends on
// 16 clients of records.  From there on 512-lane blocks with 16 clients in flight, as the
// records kernel ships (256-lane blocks and 32 in flight are 1-3 % slower at 100 x 1M).
constexpr size_t kPackedSmallD = (size_t)1 << 18;
struct PackedShapes {
    typedef RowF32 F;
    template <bool CLIP, bool ACC>
    static void launch(int W, const AccArgs &a) {
        if (a.d < kPackedSmallD) {
            if (W >= 2) launch_p<2, 64, CLIP, ACC, 64>(a);
            else launch_p<1, 64, CLIP, ACC, 64>(a);
        } else if (W == 4) launch_p<4, 16, CLIP, ACC, 512>(a);
        else if (W == 2) launch_p<2, 32, CLIP, ACC, 256>(a);
        else launch_p<1, 32, CLIP, ACC, 256>(a);
    }
};
// bf16 rows.  At 100 x 1M every shape tried (8 or 4 outputs a lane; 16, 32 or 64 clients in
// flight; 64-, 256- or 512-lane blocks) lies within 1 us of 34 us, the spread of two runs of
// one shape: the loads are what the kernel waits for.  At 50,890 outputs 64 clients in flight
// in 64-lane blocks take 8.4 us where 256-lane blocks with 32 in flight take 11.0 and 512-lane
// blocks with 16 take 14.4: too few waves (199 at 4 outputs a lane, for 1,024 SIMDs) for
// fewer loads each.  So: 16-byte loads, 16 in flight, 512-lane blocks (the records and f32
// rows' shape) from kBf16SmallD outputs on — one wave a SIMD at 8 outputs a lane — where the
// alignment allows them (rows_width), and the 64-lane shape everywhere else.
struct Bf16Shapes {
    typedef RowBf16 F;
    template <bool CLIP, bool ACC>
    static void launch(int W, const AccArgs &a) {
        if (W == 8) launch_h<8, 16, CLIP, ACC, 512>(a);
        else if (W == 4) launch_h<4, 64, CLIP, ACC, 64>(a);
        else if (W == 2) launch_h<2, 64, CLIP, ACC, 64>(a);
        else launch_h<1, 64, CLIP, ACC, 64>(a);
    }
};
// fp8 rows.  The decode is a dozen vector instructions a value, so the load-bound shapes of the
// other formats are the wrong ones here (bf16's 64 in flight in 64-lane blocks: 60.4 us at
// 100 x 1M and 40.6 us at 100 x 50,890 with 8 outputs a lane).  Measured over 14 to 18 shapes at
// five sizes (profiles/r16/fp8.jsonl): 16 clients in flight win at every size; at
// 100 x 1M 4 outputs a lane in 512-lane blocks take 44.5 us (8 outputs: 45.0 to 45.7; 16
// outputs: 48.1 at best); at 100 x 50,890 one output a lane in 256-lane blocks takes 12.5 us
// (2: 15.0; 4: 20.3 at best; 8: 27.6; 16: 46.2), at 100 x 262,152 22.3 us (4: 27.8).  So: one
// output a lane below kFp8SmallD, up to 4 from there on where the alignment allows
// (rows_width), 16 in flight throughout.  The scale of a client is one wave-uniform f32 load
// beside its row's load.
struct Fp8Shapes {
    typedef RowFp8 F;
    template <bool CLIP, bool ACC>
    static void launch(int W, const AccArgs &a) {
        if (W == 4) launch_q<4, 16, CLIP, ACC, 512>(a);
        else if (W == 2) launch_q<2, 16, CLIP, ACC, 256>(a);
        else launch_q<1, 16, CLIP, ACC, 256>(a);
    }
};

template <class S>
static hipError_t accumulate_rows(AccArgs a, bool accumulate) {
    if (a.d == 0) return hipSuccess;
    a.stride = S::F::row_stride(a.d);
    const int W = rows_width(S::F::kFmt, a.rows, a.out, a.stride, a.d);
    if (a.ccoef) {
        if (accumulate) S::template launch<true, true>(W, a);
        else S::template launch<true, false>(W, a);
    } else {
        if (accumulate) S::template launch<false, true>(W, a);
        else S::template launch<false, false>(W, a);
    }
    return hipGetLastError();
}

hipError_t launch_dense_accumulate_rows(RowFmt fmt, const void *rows, size_t n, size_t d, float coef, float *out,
                                        const float *client_coef, bool accumulate, hipStream_t s) {
    const AccArgs a = {rows, 0, n, d, coef, out, client_coef, s};
    return fmt == kRowsFp8    ? accumulate_rows<Fp8Shapes>(a, accumulate)
           : fmt == kRowsBf16 ? accumulate_rows<Bf16Shapes>(a, accumulate)
                              : accumulate_rows<PackedShapes>(a, accumulate);
}

hipError_t launch_rows_clip_coef(RowFmt fmt, const void *rows, size_t n, size_t d, float clipping, float *coef,
                                 hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (fmt == kRowsFp8)
        FLTEE_LAUNCH(fp8_norm_kernel, dim3((unsigned)n), dim3(256), 0, s, (const uint8_t *)rows,
                     RowFp8::row_stride(d), d, clipping, coef);
    else if (fmt == kRowsBf16)
        FLTEE_LAUNCH(bf16_norm_kernel, dim3((unsigned)n), dim3(256), 0, s, (const uint16_t *)rows,
                     RowBf16::row_stride(d), d, clipping, coef);
    else
        FLTEE_LAUNCH(packed_norm_kernel, dim3((unsigned)n), dim3(256), 0, s, (const float *)rows,
                     RowF32::row_stride(d), d, clipping, coef);
    return hipGetLastError();
}

static unsigned rows_grid(size_t total) {
    const size_t b = (total + 255) / 256;
    return (unsigned)(b < 65536 ? (b ? b : 1) : 65536);
}

hipError_t launch_unpack_rows(RowFmt fmt, const void *rows, size_t n, size_t d, uint64_t *rec, hipStream_t s) {
    if (n * d == 0) return hipSuccess;
    if (fmt == kRowsFp8)
        FLTEE_LAUNCH(unpack_fp8_kernel, dim3(rows_grid(n * d)), dim3(256), 0, s, (const uint8_t *)rows, n, d,
                     RowFp8::row_stride(d), rec);
    else if (fmt == kRowsBf16)
        FLTEE_LAUNCH(unpack_bf16_kernel, dim3(rows_grid(n * d)), dim3(256), 0, s, (const uint16_t *)rows, n, d,
                     RowBf16::row_stride(d), rec);
    else
        FLTEE_LAUNCH(unpack_dense_kernel, dim3(rows_grid(n * d)), dim3(256), 0, s, (const float *)rows, n, d,
                     RowF32::row_stride(d), rec);
    return hipGetLastError();
}

hipError_t launch_pack_rows(RowFmt fmt, const float *values, size_t n, size_t d, void *rows, hipStream_t s) {
    if (n * d == 0) return hipSuccess;
    if (fmt == kRowsBf16) {
        const size_t stride = RowBf16::row_stride(d);
        FLTEE_LAUNCH(pack_bf16_kernel, dim3(rows_grid(n * stride)), dim3(256), 0, s, values, n, d, stride,
                     (uint16_t *)rows);
    } else {
        const size_t stride = RowF32::row_stride(d);
        FLTEE_LAUNCH(pack_dense_kernel, dim3(rows_grid(n * stride)), dim3(256), 0, s, values, n, d, stride,
                     (float *)rows);
    }
    return hipGetLastError();
}

// the fp8 producer: scale, n floats of scratch (launch 1 writes them, launch 2 reads them)
hipError_t launch_pack_fp8(const float *values, size_t n, size_t d, float *scale, void *rows, hipStream_t s) {
    if (n * d == 0) return hipSuccess;
    const size_t stride = RowFp8::row_stride(d);
    FLTEE_LAUNCH(fp8_scale_kernel, dim3((unsigned)n), dim3(256), 0, s, values, d, scale);
    FLTEE_LAUNCH(fp8_quantise_kernel, dim3(rows_grid(n * stride)), dim3(256), 0, s, values, scale, n, d, stride,
                 (uint8_t *)rows);
    return hipGetLastError();
}

}  // namespace fltee
