// k_trim.hip — coordinate-wise trimmed mean / median of dense uploads (gfx950), oblivious.
//
// FLTEE_OPT_TRIM with trim = t (1 <= t <= FLTEE_TRIM_MAX, 2 t < n) on the dense routes: per
// output j, with x_c = client c's value at j (FLTEE_OPT_CLIP: __fmul_rn(v, coef_c)) and
//     ord(x) = bits(x) ^ (bits(x) >> 31 ? 0xFFFFFFFF : 0x80000000)
// (a total order on every bit pattern: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN),
// the t clients smallest by (ord ascending, c ascending) are removed, then from the rest the
// t clients largest by (ord descending, c ascending); out[j] = the in-order __fadd_rn sum
// ((+0.0 + x_c1) + x_c2) + ... of the kept clients, times coef (or out += with ACC).
//
// trimmed_mean_kernel: a lane owns W adjacent outputs and reads its columns twice.
//   Pass A streams the n clients in order (UC loads in flight, the n tail one guarded batch
//   as in dense_accumulate_p) and keeps, per output, the T smallest and the T largest ord
//   values in two sorted register lists (T: the compile-time capacity >= t), each updated by
//   a min / max insertion chain — two VALU per slot, no index: equal ords are
//   indistinguishable there, and the tie rule only needs the threshold (entry t - 1) and how
//   many of the first t entries equal it (m_lo, m_hi).  Both are picked out of the lists by
//   select chains on the public t: no register is indexed at run time.
//   Pass B re-reads the columns in upload order with two counters of equal-to-threshold
//   values seen: x is dropped low when ord < lo, or ord == lo and fewer than m_lo equals were
//   seen; of what is left, high when ord > hi, or ord == hi and fewer than m_hi equals (not
//   dropped low) were seen.  A dropped value is replaced by a selected +0.0 (the accumulator
//   starts at +0.0 and is never -0.0: the same bits as leaving the add out; a 0 / 1 mask
//   multiply would turn inf into NaN).
// Every row element is read at a fixed address, twice; every loop bound is a function of
// (n, d, t) and the pointers' alignment; compares feed selects: no data-dependent branch,
// address or early exit.  The layouts:
//   records : 8-byte (idx, val) loads, W = 1; idx != position raises
//             FLTEE_DEV_ERR_DENSE_ORDER (reported, not followed), as dense_accumulate_v does.
//   packed  : f32 rows (rows.h: the load, the stride, the store); W = 4 / 2 / 1 by rows_width,
//             capped by the lists' registers (T = 16: W <= 2; T = 64: W = 1, the lists alone
//             are 128 registers an output).
//             The lanes of the last group past d never store: the padding float of an odd d
//             reaches no output.
#include "common.h"

namespace fltee {

typedef uint32_t tu32x2_t __attribute__((ext_vector_type(2)));

static __device__ __forceinline__ uint32_t trim_ord(float x) {
    const uint32_t b = __float_as_uint(x);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}

// one client's W values of this lane's columns; records: bad |= idx ^ position
template <bool PACKED, int W>
static __device__ __forceinline__ void trim_load(const void *row, size_t j0, float (&x)[W], uint32_t &bad) {
    if constexpr (PACKED) {
        uint32_t r[W];
        RowF32::load<W>((const float *)row + j0, r);
#pragma unroll
        for (int w = 0; w < W; ++w) x[w] = RowF32::value<W>(r, w);
    } else {
        static_assert(PACKED || W == 1, "records: one 8-byte record a lane");
        const tu32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const tu32x2_t *>(row) + j0);
        bad |= v.x ^ (uint32_t)j0;
        x[0] = __uint_as_float(v.y);
    }
}

// stride: bytes between rows (records: 8 d; packed: 8 ceil(d / 2))
template <bool PACKED, int W, int T, int UC>
__global__ __launch_bounds__(256) void trimmed_mean_kernel(const uint8_t *__restrict__ in, size_t stride,
                                                           size_t d, uint32_t n, uint32_t t, float coef,
                                                           float *__restrict__ out,
                                                           const float *__restrict__ ccoef, int acc_out,
                                                           uint32_t *__restrict__ status) {
    const size_t j0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * W;
    if (j0 >= d) return;
    const bool clip = ccoef != nullptr;  // wave-uniform, public
    uint32_t bad = 0;

    // ---- pass A: the T smallest (ascending) and the T largest (descending) ords per output
    uint32_t L[W][T], H[W][T];
#pragma unroll
    for (int w = 0; w < W; ++w) {
#pragma unroll
        for (int i = 0; i < T; ++i) L[w][i] = 0xFFFFFFFFu, H[w][i] = 0u;
    }
    for (uint32_t c = 0; c < n; c += UC) {  // (the last batch: guarded by the public n)
        float x[UC][W];
#pragma unroll
        for (int u = 0; u < UC; ++u)
            if (c + u < n) trim_load<PACKED, W>(in + (size_t)(c + u) * stride, j0, x[u], bad);
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (c + u < n) {
                const float cc = clip ? ccoef[c + u] : 1.0f;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const uint32_t o = trim_ord(clip ? __fmul_rn(x[u][w], cc) : x[u][w]);
                    uint32_t up = o, dn = o;
#pragma unroll
                    for (int i = 0; i < T; ++i) {
                        const uint32_t l = L[w][i], h = H[w][i];
                        L[w][i] = l < up ? l : up;
                        up = l < up ? up : l;
                        H[w][i] = h > dn ? h : dn;
                        dn = h > dn ? dn : h;
                    }
                }
            }
        }
    }
    // the thresholds (entry t - 1) and their multiplicity among the first t entries
    uint32_t lo[W], hi[W], m_lo[W], m_hi[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        uint32_t a = 0, b = 0;
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const bool at = (uint32_t)i + 1 == t;
            a = at ? L[w][i] : a;
            b = at ? H[w][i] : b;
        }
        uint32_t ma = 0, mb = 0;
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const bool in_t = (uint32_t)i < t;
            ma += (in_t && L[w][i] == a) ? 1u : 0u;
            mb += (in_t && H[w][i] == b) ? 1u : 0u;
        }
        lo[w] = a, hi[w] = b, m_lo[w] = ma, m_hi[w] = mb;
    }

    // ---- pass B: the kept clients' in-order sum
    float acc[W];
    uint32_t seen_lo[W], seen_hi[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0.0f, seen_lo[w] = 0, seen_hi[w] = 0;
    uint32_t bad2 = 0;  // (pass A checked every index)
    for (uint32_t c = 0; c < n; c += UC) {
        float x[UC][W];
#pragma unroll
        for (int u = 0; u < UC; ++u)
            if (c + u < n) trim_load<PACKED, W>(in + (size_t)(c + u) * stride, j0, x[u], bad2);
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (c + u < n) {
                const float cc = clip ? ccoef[c + u] : 1.0f;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const float v = clip ? __fmul_rn(x[u][w], cc) : x[u][w];
                    const uint32_t o = trim_ord(v);
                    const bool eq_lo = o == lo[w];
                    const bool drop_lo = o < lo[w] || (eq_lo && seen_lo[w] < m_lo[w]);
                    seen_lo[w] += eq_lo ? 1u : 0u;
                    const bool eq_hi = !drop_lo && o == hi[w];
                    const bool drop_hi = !drop_lo && (o > hi[w] || (eq_hi && seen_hi[w] < m_hi[w]));
                    seen_hi[w] += eq_hi ? 1u : 0u;
                    acc[w] = __fadd_rn(acc[w], (drop_lo || drop_hi) ? 0.0f : v);
                }
            }
        }
    }

    rows_store<W>(out, j0, d, acc, coef, acc_out != 0);
    if (!PACKED && bad) atomicOr(status, FLTEE_DEV_ERR_DENSE_ORDER);
}

// Fewer outputs than this: too few waves to fill the SIMDs with 256-lane blocks (k_rows.hip's
// small-d reasoning), so the lanes go out in 64-lane blocks — one wave a block, spread over
// every CU.  The same work per lane: the same bits.
constexpr size_t kTrimSmallD = (size_t)1 << 18;

template <bool PACKED, int W, int T, int UC>
static void launch_t(const void *in, size_t stride, size_t n, size_t d, size_t t, float coef, float *out,
                     const float *ccoef, bool acc, uint32_t *status, hipStream_t s) {
    const size_t groups = (d + W - 1) / W;
    const unsigned nth = d < kTrimSmallD ? 64 : 256;
    FLTEE_LAUNCH((trimmed_mean_kernel<PACKED, W, T, UC>), dim3((unsigned)((groups + nth - 1) / nth)), dim3(nth), 0,
                 s, (const uint8_t *)in, stride, d, (uint32_t)n, (uint32_t)t, coef, out, ccoef, acc ? 1 : 0,
                 status);
}

// the list capacity for t: 4, 16 or 64 (FLTEE_TRIM_MAX)
template <bool PACKED, int W>
static void launch_by_t(const void *in, size_t stride, size_t n, size_t d, size_t t, float coef, float *out,
                        const float *ccoef, bool acc, uint32_t *status, hipStream_t s) {
    // (T = 16 at W = 4 allocates 266 registers, one wave a SIMD; W = 2 takes 144: three waves)
    constexpr int W16 = W == 4 ? 2 : W;
    if (t <= 4) launch_t<PACKED, W, 4, 16>(in, stride, n, d, t, coef, out, ccoef, acc, status, s);
    else launch_t<PACKED, W16, 16, 8>(in, stride, n, d, t, coef, out, ccoef, acc, status, s);
}

hipError_t launch_trimmed_mean(const void *in, bool packed, size_t n, size_t d, size_t t, float coef,
                               float *out, const float *client_coef, bool accumulate, uint32_t *status,
                               hipStream_t s) {
    if (d == 0) return hipSuccess;
    if (t == 0 || t > FLTEE_TRIM_MAX || 2 * t >= n) return hipErrorInvalidValue;  // (the plan refuses these)
    if (!packed) {
        if (t > 16) launch_t<false, 1, 64, 4>(in, d * 8, n, d, t, coef, out, client_coef, accumulate, status, s);
        else launch_by_t<false, 1>(in, d * 8, n, d, t, coef, out, client_coef, accumulate, status, s);
        return hipGetLastError();
    }
    const size_t stride = RowF32::row_stride(d);  // floats
    const int W = rows_width(kRowsF32, in, out, stride, d);
    if (t > 16) launch_t<true, 1, 64, 4>(in, stride * 4, n, d, t, coef, out, client_coef, accumulate, status, s);
    else if (W == 4) launch_by_t<true, 4>(in, stride * 4, n, d, t, coef, out, client_coef, accumulate, status, s);
    else if (W == 2) launch_by_t<true, 2>(in, stride * 4, n, d, t, coef, out, client_coef, accumulate, status, s);
    else launch_by_t<true, 1>(in, stride * 4, n, d, t, coef, out, client_coef, accumulate, status, s);
    return hipGetLastError();
}

}  // namespace fltee
