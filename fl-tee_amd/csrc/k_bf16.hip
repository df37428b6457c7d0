// k_bf16.hip — bf16 dense uploads (gfx950): value-only slices at a quarter of the bytes.
//
// A BF16 slice of d parameters is Q = ceil(d / 4) units of 8 bytes: the d little-endian
// bf16 values in position order, then 4 Q - d bf16 of padding (written +0.0 by the client,
// ignored here).  n slices are n rows, 4 Q halves apart.  Widening is exact for every bit
// pattern: f32 bits = (uint32)h << 16 — the server adds no error to what the client sent.
//
// dense_accumulate_h : k_packed.hip's dense_accumulate_p on bf16 rows, under the same
//   contract: out[j] = the in-order client sum ((+0.0 + x_0[j]) + x_1[j]) + ... with
//   __fadd_rn over the widened values, then * coef (or out += with ACC; per-client clip
//   coefficients with CLIP, x * cc rounded before the add as on the records route).  A lane
//   owns W adjacent outputs and issues one 2 W-byte non-temporal load per client, UC clients
//   in flight; the clients past the last full batch go out as one more batch whose loads
//   and adds are guarded by c + u < n (a wave-uniform test of the public n).  Every half is
//   read once at a fixed address: the access pattern depends on (n, d) and the pointers'
//   alignment only.  There is no index, so there is no status word.  W = 8 where the rows
//   and the base are 16-byte aligned (Q even) and d is large (bf16_dispatch), W = 4 on
//   8-byte alignment (Q odd — MLP-MNIST: d = 50,890, Q = 12,723 — or a base at 8 mod 16: the
//   survivors buffer can land there), W = 2 on 4 bytes, W = 1 (a scalar 2-byte load) below
//   that.  The lanes of the last group past d never store: the padding reaches no output.
// bf16_norm_kernel : client_norm_kernel (k_dp.hip) on a bf16 row: the same f64 sum of
//   squares in the same lane order over the d widened values, so CLIP takes the same
//   coefficients.
// unpack_bf16_kernel : rows -> records (j, widen(h[j])); pack_bf16_kernel: the client
//   producer, f32 values [n][d] -> rows, narrowed in integer ops (round to nearest even; a
//   NaN keeps its sign and is quieted), padding +0.0.
#include "common.h"

namespace fltee {

typedef uint32_t hu32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t hu32x2_t __attribute__((ext_vector_type(2)));
typedef float hf32x4_t __attribute__((ext_vector_type(4)));
typedef float hf32x2_t __attribute__((ext_vector_type(2)));

static __device__ __forceinline__ float widen_lo(uint32_t u) { return __uint_as_float(u << 16); }
static __device__ __forceinline__ float widen_hi(uint32_t u) { return __uint_as_float(u & 0xFFFF0000u); }

// W halves at p (2 W-byte aligned) as they lie in memory: (W + 1) / 2 dwords, half w in the
// low (w even) or high (w odd) 16 bits of dword w / 2.  They stay packed while in flight and
// are widened at the add.
template <int W>
static __device__ __forceinline__ void bh_load(const uint16_t *p, uint32_t (&r)[(W + 1) / 2]) {
    if constexpr (W == 1) {
        r[0] = __builtin_nontemporal_load(p);
    } else if constexpr (W == 2) {
        r[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p));
    } else {
        typedef typename std::conditional<W == 8, hu32x4_t, hu32x2_t>::type V;
        const V v = __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
#pragma unroll
        for (int w = 0; w < W / 2; ++w) r[w] = v[w];
    }
}

template <int W>
static __device__ __forceinline__ float bh_value(const uint32_t (&r)[(W + 1) / 2], int w) {
    return (w & 1) ? widen_hi(r[w / 2]) : widen_lo(r[w / 2]);
}

// stride: halves between rows (4 Q); lane g owns outputs [g W, g W + W) — where W > 1 the
// group of the last lane may reach past d into the row's padding (g W + W <= stride holds:
// stride is a multiple of W on the paths that take W), never past the row.
template <int W, int UC, bool CLIP, bool ACC, int NTH>
__global__ __launch_bounds__(NTH) void dense_accumulate_h(const uint16_t *__restrict__ rows, size_t stride,
                                                          size_t d, uint32_t n, float coef,
                                                          float *__restrict__ out,
                                                          const float *__restrict__ ccoef) {
    const size_t j0 = ((size_t)blockIdx.x * NTH + threadIdx.x) * W;
    if (j0 >= d) return;
    const uint16_t *p = rows + j0;
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0.0f;
    uint32_t c = 0;
    for (; c + UC <= n; c += UC) {
        uint32_t x[UC][(W + 1) / 2];
#pragma unroll
        for (int u = 0; u < UC; ++u) bh_load<W>(p + (size_t)(c + u) * stride, x[u]);
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const float cc = CLIP ? ccoef[c + u] : 1.0f;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float v = bh_value<W>(x[u], w);
                acc[w] = __fadd_rn(acc[w], CLIP ? __fmul_rn(v, cc) : v);
            }
        }
    }
    if (c < n) {  // the n tail: one guarded batch (wave-uniform tests of the public n)
        uint32_t x[UC][(W + 1) / 2];
#pragma unroll
        for (int u = 0; u < UC; ++u)
            if (c + u < n) bh_load<W>(p + (size_t)(c + u) * stride, x[u]);
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (c + u < n) {
                const float cc = CLIP ? ccoef[c + u] : 1.0f;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const float v = bh_value<W>(x[u], w);
                    acc[w] = __fadd_rn(acc[w], CLIP ? __fmul_rn(v, cc) : v);
                }
            }
        }
    }
    float *o = out + j0;
    if constexpr (W > 1) {
        if (j0 + W <= d) {  // a whole group: 16-byte stores (8-byte for W = 2); out is aligned for them
            constexpr int SW = W >= 4 ? 4 : 2;
            typedef typename std::conditional<SW == 4, hf32x4_t, hf32x2_t>::type V;
#pragma unroll
            for (int g = 0; g < W / SW; ++g) {
                V r;
                if (ACC) {
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
    for (int w = 0; w < W; ++w)  // the d tail: the columns past d are dropped here
        if (j0 + w < d) o[w] = ACC ? __fadd_rn(o[w], acc[w]) : __fmul_rn(acc[w], coef);
}

template <int W, int UC, bool CLIP, bool ACC, int NTH>
static void launch_h(const uint16_t *rows, size_t stride, size_t n, size_t d, float coef, float *out,
                     const float *ccoef, hipStream_t s) {
    const size_t groups = (d + W - 1) / W;
    FLTEE_LAUNCH((dense_accumulate_h<W, UC, CLIP, ACC, NTH>), dim3((unsigned)((groups + NTH - 1) / NTH)),
                 dim3(NTH), 0, s, rows, stride, d, (uint32_t)n, coef, out, ccoef);
}

// The launch shape (A/B at 100 x 1M and 100 x 50,890, profiles/r13/bf16.jsonl).  At 100 x 1M
// every shape tried (8 or 4 outputs a lane; 16, 32 or 64 clients in flight; 64-, 256- or
// 512-lane blocks) lies within 1 us of 34 us, the spread of two runs of one shape: the loads
// are what the kernel waits for.  At 50,890 outputs 64 clients in flight in 64-lane blocks
// take 8.4 us where 256-lane blocks with 32 in flight take 11.0 and 512-lane blocks with 16
// take 14.4: too few waves (199 at 4 outputs a lane, for 1,024 SIMDs) for fewer loads each.
// So: 16-byte loads, 16 in flight, 512-lane blocks (the records and packed kernels' shape)
// from kBf16SmallD outputs on — one wave a SIMD at 8 outputs a lane — where the alignment
// allows them, and the 64-lane shape everywhere else.  The same adds in the same order: the
// same bits.
constexpr size_t kBf16SmallD = (size_t)1 << 19;

template <bool CLIP, bool ACC>
static hipError_t bf16_dispatch(const uint16_t *rows, size_t n, size_t d, float coef, float *out,
                                const float *ccoef, hipStream_t s) {
    const size_t stride = (d + 3) / 4 * 4;
    const uintptr_t a = (uintptr_t)rows, b = (uintptr_t)out;
    int W = 1;  // (rows are always 8-byte multiples apart)
    if (a % 4 == 0 && b % 8 == 0) W = 2;
    if (a % 8 == 0 && b % 16 == 0) W = 4;
    if (a % 16 == 0 && b % 16 == 0 && stride % 8 == 0 && d >= kBf16SmallD) W = 8;
    if (W == 8) launch_h<8, 16, CLIP, ACC, 512>(rows, stride, n, d, coef, out, ccoef, s);
    else if (W == 4) launch_h<4, 64, CLIP, ACC, 64>(rows, stride, n, d, coef, out, ccoef, s);
    else if (W == 2) launch_h<2, 64, CLIP, ACC, 64>(rows, stride, n, d, coef, out, ccoef, s);
    else launch_h<1, 64, CLIP, ACC, 64>(rows, stride, n, d, coef, out, ccoef, s);
    return hipGetLastError();
}

hipError_t launch_dense_accumulate_bf16(const void *rows, size_t n, size_t d, float coef, float *out,
                                        const float *client_coef, bool accumulate, hipStream_t s) {
    if (d == 0) return hipSuccess;
    const uint16_t *h = (const uint16_t *)rows;
    if (client_coef)
        return accumulate ? bf16_dispatch<true, true>(h, n, d, coef, out, client_coef, s)
                          : bf16_dispatch<true, false>(h, n, d, coef, out, client_coef, s);
    return accumulate ? bf16_dispatch<false, true>(h, n, d, coef, out, nullptr, s)
                      : bf16_dispatch<false, false>(h, n, d, coef, out, nullptr, s);
}

// client_norm_kernel's sums, lane for lane: thread t takes values t, t + 256, ...
__global__ __launch_bounds__(256) void bf16_norm_kernel(const uint16_t *__restrict__ rows, size_t stride,
                                                        size_t d, float clipping,
                                                        float *__restrict__ coef) {
    __shared__ double part[4];
    const uint16_t *src = rows + (size_t)blockIdx.x * stride;
    double ss = 0.0;
    for (size_t e = threadIdx.x; e < d; e += 256) {
        const double v = (double)widen_lo(src[e]);
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

hipError_t launch_bf16_clip_coef(const void *rows, size_t n, size_t d, float clipping, float *coef,
                                 hipStream_t s) {
    if (n == 0) return hipSuccess;
    FLTEE_LAUNCH(bf16_norm_kernel, dim3((unsigned)n), dim3(256), 0, s, (const uint16_t *)rows,
                 (d + 3) / 4 * 4, d, clipping, coef);
    return hipGetLastError();
}

__global__ void unpack_bf16_kernel(const uint16_t *__restrict__ rows, size_t n, size_t d, size_t stride,
                                   uint64_t *__restrict__ rec) {
    const size_t total = n * d;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t c = t / d, i = t - c * d;
        rec[t] = make_rec((uint32_t)i, widen_lo(rows[c * stride + i]));
    }
}

// f32 -> bf16 in integer ops: round to nearest even (values just under FLT_MAX round to
// inf); a NaN keeps its sign and its upper payload and is quieted
static __device__ __forceinline__ uint16_t narrow_bf16(float x) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

__global__ void pack_bf16_kernel(const float *__restrict__ values, size_t n, size_t d, size_t stride,
                                 uint16_t *__restrict__ rows) {
    const size_t total = n * stride;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t c = t / stride, i = t - c * stride;
        rows[t] = i < d ? narrow_bf16(values[c * d + i]) : (uint16_t)0;
    }
}

static unsigned bf16_grid(size_t total) {
    const size_t b = (total + 255) / 256;
    return (unsigned)(b < 65536 ? (b ? b : 1) : 65536);
}

hipError_t launch_unpack_bf16(const void *rows, size_t n, size_t d, uint64_t *rec, hipStream_t s) {
    if (n * d == 0) return hipSuccess;
    FLTEE_LAUNCH(unpack_bf16_kernel, dim3(bf16_grid(n * d)), dim3(256), 0, s, (const uint16_t *)rows, n, d,
                 (d + 3) / 4 * 4, rec);
    return hipGetLastError();
}

hipError_t launch_pack_bf16(const float *values, size_t n, size_t d, void *rows, hipStream_t s) {
    if (n * d == 0) return hipSuccess;
    const size_t stride = (d + 3) / 4 * 4;
    FLTEE_LAUNCH(pack_bf16_kernel, dim3(bf16_grid(n * stride)), dim3(256), 0, s, values, n, d, stride,
                 (uint16_t *)rows);
    return hipGetLastError();
}

}  // namespace fltee
