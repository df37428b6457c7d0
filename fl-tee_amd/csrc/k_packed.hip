// k_packed.hip — packed dense uploads (gfx950): value-only slices at half the bytes.
//
// A dense upload's record (j, v[j]) carries an index that says nothing.  A PACKED slice
// of d parameters is U = ceil(d / 2) units of 8 bytes: the d f32 values in position
// order, then one f32 of padding when d is odd (written +0.0 by the client, ignored
// here).  n slices are n rows, 2 U floats apart.
//
// dense_accumulate_p : the packed form of k_accumulate.hip's dense_accumulate_v, under
//   the same contract: out[j] = the in-order client sum ((+0.0 + v_0[j]) + v_1[j]) + ...
//   with __fadd_rn, then * coef (or out += with ACC; per-client clip coefficients with
//   CLIP, v * cc rounded before the add as on the records route).  A lane owns W adjacent
//   outputs and issues one 4 W-byte non-temporal load per client, UC clients in flight;
//   the clients past the last full batch go out as one more batch whose loads and adds
//   are guarded by c + u < n (a wave-uniform test of the public n: the loads still issue
//   back to back, no row is read twice).  Every float is read once at a fixed address:
//   the access pattern depends on (n, d) and the pointers' alignment only.  There is no
//   index, so there is no status word.  W = 4 where the rows and the base are 16-byte
//   aligned (U even), W = 2 on 8-byte alignment (U odd — MLP-MNIST: d = 50,890,
//   U = 25,445 — or a base at 8 mod 16: the survivors buffer can land there), W = 1
//   below that.  The lanes of the last group past d never store: the padding float of an
//   odd d reaches no output.
// packed_norm_kernel : client_norm_kernel (k_dp.hip) on a packed row: the same f64 sum
//   of squares in the same order over the d values, so CLIP takes the same coefficients.
// unpack_dense_kernel : rows -> records (j, v[j]) (launch_client_dense with a row
//   stride); pack_dense_kernel: the client producer, values [n][d] -> rows, padding +0.0.
#include "common.h"

namespace fltee {

typedef float pf32x4_t __attribute__((ext_vector_type(4)));
typedef float pf32x2_t __attribute__((ext_vector_type(2)));

template <int W> struct PVec;
template <> struct PVec<4> { typedef pf32x4_t type; };
template <> struct PVec<2> { typedef pf32x2_t type; };
template <> struct PVec<1> { typedef float type; };

template <int W>
static __device__ __forceinline__ void pk_load(const float *p, float (&x)[W]) {
    typedef typename PVec<W>::type V;
    const V v = __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
    if constexpr (W == 1) {
        x[0] = v;
    } else {
#pragma unroll
        for (int w = 0; w < W; ++w) x[w] = v[w];
    }
}

// stride: floats between rows (2 U); lane g owns outputs [g W, g W + W) — where W > 1 the
// group of the last lane may reach past d into the row's padding (g W + W <= stride holds:
// stride is a multiple of W on the paths that take W), never past the row.
template <int W, int UC, bool CLIP, bool ACC, int NTH>
__global__ __launch_bounds__(NTH) void dense_accumulate_p(const float *__restrict__ pk, size_t stride,
                                                          size_t d, uint32_t n, float coef,
                                                          float *__restrict__ out,
                                                          const float *__restrict__ ccoef) {
    const size_t j0 = ((size_t)blockIdx.x * NTH + threadIdx.x) * W;
    if (j0 >= d) return;
    const float *p = pk + j0;
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0.0f;
    uint32_t c = 0;
    for (; c + UC <= n; c += UC) {
        float x[UC][W];
#pragma unroll
        for (int u = 0; u < UC; ++u) pk_load<W>(p + (size_t)(c + u) * stride, x[u]);
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const float cc = CLIP ? ccoef[c + u] : 1.0f;
#pragma unroll
            for (int w = 0; w < W; ++w)
                acc[w] = __fadd_rn(acc[w], CLIP ? __fmul_rn(x[u][w], cc) : x[u][w]);
        }
    }
    if (c < n) {  // the n tail: one guarded batch (wave-uniform tests of the public n)
        float x[UC][W];
#pragma unroll
        for (int u = 0; u < UC; ++u)
            if (c + u < n) pk_load<W>(p + (size_t)(c + u) * stride, x[u]);
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (c + u < n) {
                const float cc = CLIP ? ccoef[c + u] : 1.0f;
#pragma unroll
                for (int w = 0; w < W; ++w)
                    acc[w] = __fadd_rn(acc[w], CLIP ? __fmul_rn(x[u][w], cc) : x[u][w]);
            }
        }
    }
    float *o = out + j0;
    if constexpr (W > 1) {
        if (j0 + W <= d) {  // a whole group: one 4 W-byte store (out is 4 W-byte aligned)
            typedef typename PVec<W>::type V;
            V r;
            if (ACC) {
                const V prev = *reinterpret_cast<const V *>(o);
#pragma unroll
                for (int w = 0; w < W; ++w) r[w] = __fadd_rn(prev[w], acc[w]);
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) r[w] = __fmul_rn(acc[w], coef);
            }
            *reinterpret_cast<V *>(o) = r;
            return;
        }
    }
#pragma unroll
    for (int w = 0; w < W; ++w)  // the d tail: the columns past d are dropped here
        if (j0 + w < d) o[w] = ACC ? __fadd_rn(o[w], acc[w]) : __fmul_rn(acc[w], coef);
}

template <int W, int UC, bool CLIP, bool ACC, int NTH>
static void launch_p(const float *pk, size_t stride, size_t n, size_t d, float coef, float *out,
                     const float *ccoef, hipStream_t s) {
    const size_t groups = (d + W - 1) / W;
    FLTEE_LAUNCH((dense_accumulate_p<W, UC, CLIP, ACC, NTH>), dim3((unsigned)((groups + NTH - 1) / NTH)),
                 dim3(NTH), 0, s, pk, stride, d, (uint32_t)n, coef, out, ccoef);
}

// Tuning hook (fltee_debug_set_packed_variant): 0 is the shipped configuration.
static int g_packed_variant = 0;
void set_packed_variant(int v) { g_packed_variant = v; }

// Fewer than this many outputs: too few waves for 16 loads a lane to cover the HBM
// latency (MLP-MNIST: 25,445 pairs = 398 waves for 1,024 SIMDs), so a lane keeps 64
// clients in flight instead — 64 x 4 W bytes of registers, what dense_accumulate_w
// spends on 16 clients of records.  The same adds in the same order: the same bits.
constexpr size_t kPackedSmallD = (size_t)1 << 18;

template <bool CLIP, bool ACC>
static hipError_t packed_dispatch(const float *pk, size_t n, size_t d, float coef, float *out,
                                  const float *ccoef, hipStream_t s) {
    const size_t stride = (d + 1) / 2 * 2;
    const uintptr_t a = (uintptr_t)pk, b = (uintptr_t)out;
    int W = 1;
    if (a % 8 == 0 && b % 8 == 0) W = 2;  // (rows are always 8-byte multiples apart)
    if (a % 16 == 0 && b % 16 == 0 && stride % 4 == 0) W = 4;
    const bool small = d < kPackedSmallD;
    switch (g_packed_variant) {  // A/B shapes; every one computes the same bits
    case 1: if (W == 4) { launch_p<4, 32, CLIP, ACC, 256>(pk, stride, n, d, coef, out, ccoef, s); return hipGetLastError(); } break;
    case 2: if (W == 4) { launch_p<4, 16, CLIP, ACC, 256>(pk, stride, n, d, coef, out, ccoef, s); return hipGetLastError(); } break;
    case 3: if (W >= 2) { launch_p<2, 32, CLIP, ACC, 256>(pk, stride, n, d, coef, out, ccoef, s); return hipGetLastError(); } break;
    case 4: if (W >= 2) { launch_p<2, 16, CLIP, ACC, 256>(pk, stride, n, d, coef, out, ccoef, s); return hipGetLastError(); } break;
    case 5: launch_p<1, 64, CLIP, ACC, 64>(pk, stride, n, d, coef, out, ccoef, s); return hipGetLastError();
    case 6: if (W >= 2) { launch_p<2, 64, CLIP, ACC, 256>(pk, stride, n, d, coef, out, ccoef, s); return hipGetLastError(); } break;
    case 7: if (W == 4) { launch_p<4, 32, CLIP, ACC, 64>(pk, stride, n, d, coef, out, ccoef, s); return hipGetLastError(); } break;
    default: break;
    }
    if (small) {
        if (W >= 2) launch_p<2, 64, CLIP, ACC, 64>(pk, stride, n, d, coef, out, ccoef, s);
        else launch_p<1, 64, CLIP, ACC, 64>(pk, stride, n, d, coef, out, ccoef, s);
    } else if (W == 4) {
        // 512-lane blocks, 16 clients in flight, as the records kernel ships (A/B at 100 x 1M,
        // profiles/r11/packed.jsonl: 256-lane blocks (variant 2) and 32 clients in flight
        // (variant 1) are 1-3 % slower)
        launch_p<4, 16, CLIP, ACC, 512>(pk, stride, n, d, coef, out, ccoef, s);
    } else if (W == 2) {
        launch_p<2, 32, CLIP, ACC, 256>(pk, stride, n, d, coef, out, ccoef, s);
    } else {
        launch_p<1, 32, CLIP, ACC, 256>(pk, stride, n, d, coef, out, ccoef, s);
    }
    return hipGetLastError();
}

hipError_t launch_dense_accumulate_packed(const void *packed, size_t n, size_t d, float coef, float *out,
                                          const float *client_coef, bool accumulate, hipStream_t s) {
    if (d == 0) return hipSuccess;
    const float *pk = (const float *)packed;
    if (client_coef)
        return accumulate ? packed_dispatch<true, true>(pk, n, d, coef, out, client_coef, s)
                          : packed_dispatch<true, false>(pk, n, d, coef, out, client_coef, s);
    return accumulate ? packed_dispatch<false, true>(pk, n, d, coef, out, nullptr, s)
                      : packed_dispatch<false, false>(pk, n, d, coef, out, nullptr, s);
}

// client_norm_kernel's sums, lane for lane: thread t takes values t, t + 256, ...
__global__ __launch_bounds__(256) void packed_norm_kernel(const float *__restrict__ pk, size_t stride,
                                                          size_t d, float clipping,
                                                          float *__restrict__ coef) {
    __shared__ double part[4];
    const float *src = pk + (size_t)blockIdx.x * stride;
    double ss = 0.0;
    for (size_t e = threadIdx.x; e < d; e += 256) {
        const double v = (double)src[e];
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

hipError_t launch_packed_clip_coef(const void *packed, size_t n, size_t d, float clipping, float *coef,
                                   hipStream_t s) {
    if (n == 0) return hipSuccess;
    FLTEE_LAUNCH(packed_norm_kernel, dim3((unsigned)n), dim3(256), 0, s, (const float *)packed,
                 (d + 1) / 2 * 2, d, clipping, coef);
    return hipGetLastError();
}

__global__ void unpack_dense_kernel(const float *__restrict__ pk, size_t n, size_t d, size_t stride,
                                    uint64_t *__restrict__ rec) {
    const size_t total = n * d;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t c = t / d, i = t - c * d;
        rec[t] = make_rec((uint32_t)i, pk[c * stride + i]);
    }
}

__global__ void pack_dense_kernel(const float *__restrict__ values, size_t n, size_t d, size_t stride,
                                  float *__restrict__ pk) {
    const size_t total = n * stride;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t c = t / stride, i = t - c * stride;
        pk[t] = i < d ? values[c * d + i] : 0.0f;
    }
}

static unsigned packed_grid(size_t total) {
    const size_t b = (total + 255) / 256;
    return (unsigned)(b < 65536 ? (b ? b : 1) : 65536);
}

hipError_t launch_unpack_dense(const void *packed, size_t n, size_t d, uint64_t *rec, hipStream_t s) {
    if (n * d == 0) return hipSuccess;
    FLTEE_LAUNCH(unpack_dense_kernel, dim3(packed_grid(n * d)), dim3(256), 0, s, (const float *)packed, n,
                 d, (d + 1) / 2 * 2, rec);
    return hipGetLastError();
}

hipError_t launch_pack_dense(const float *values, size_t n, size_t d, void *packed, hipStream_t s) {
    if (n * d == 0) return hipSuccess;
    const size_t stride = (d + 1) / 2 * 2;
    FLTEE_LAUNCH(pack_dense_kernel, dim3(packed_grid(n * stride)), dim3(256), 0, s, values, n, d, stride,
                 (float *)packed);
    return hipGetLastError();
}

}  // namespace fltee
