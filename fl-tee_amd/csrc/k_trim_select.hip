// k_trim_select.hip — the trimmed mean / median of dense uploads at any trim count (gfx950),
// oblivious: the two thresholds by a bitwise descent instead of k_trim.hip's register lists.
//
// FLTEE_OPT_TRIM | FLTEE_OPT_TRIM_SELECT with trim = t (t >= 1, 2 t < n, n <=
// FLTEE_TRIM_SELECT_MAX_N): trimmed_mean_kernel's contract (k_trim.hip's header: ord, the tie
// rule by upload order on both sides, a dropped value replaced by a selected +0.0, the kept
// clients' __fadd_rn sum in upload order, coef / ACCUMULATE / the clip coefficients), the
// definition tests/trim_model.py.  What pass B needs per output, with the ord keys sorted as
// s[0 .. n): lo = s[t - 1], hi = s[n - t], m_lo = t - #{ord < lo}, m_hi = t - #{ord > hi}.
//
// trim_select_kernel<PACKED, C>: a block of kSelThreads lanes owns C adjacent columns.
//   Stage: the n x C tile goes to LDS once, as ord keys (ord is a bijection: the value comes
//   back as ord ^ (ord >> 31 ? 0x80000000 : 0xFFFFFFFF)), the clip applied before the key.  A
//   lane is (col = tid % C, g = tid / C), G = kSelThreads / C client groups; client c's C
//   values are one contiguous 4 C-byte (records: 8 C-byte) segment, read with non-temporal
//   loads, kSelInFlight clients a lane in flight, the tail of n guarded by the public n.  The
//   input is read from HBM once.  Key (c, col) lies at dword c * C + col, so lane tid's i-th
//   client is dword i * kSelThreads + tid: every LDS access of the count loops is a
//   contiguous, conflict-free row of the block.  The tile is padded to a whole number of
//   G-client rows with the key 0xFFFFFFFF, which no "x < candidate" ever counts.
//   Descent, 32 rounds, both statistics together: p = 0; for b = 31 .. 0: c = p | 1 << b;
//   p = #{x < c} <= k ? c : p  (k = t - 1 for lo, n - t for hi; afterwards p = s[k]).  A lane
//   counts its ceil(n / G) clients against both candidates from one LDS read; the two counts
//   (each <= 4096 < 2^16) travel as one dword, summed over the column's lanes of a wave by an
//   xor butterfly (ds_bpermute / DPP: no LDS memory) and over the block's waves through a
//   double-buffered LDS slot, one barrier a round.  Every lane of a column holds the same sum
//   and takes the same select.  A 33rd counting round gives #{x < lo} and #{x > hi} (the pad
//   rows excluded by the public n).
//   Walk: lane col of the block (g = 0) walks its LDS column in upload order with the two
//   seen-equal counters — pass B of k_trim.hip on fixed LDS addresses, reads issued ahead —
//   and stores the output.
// Every global and LDS address and every loop bound is a function of (n, d) alone (t enters
// only as the two compare constants k); compares feed counters and selects: no data-dependent
// branch, address or early exit.  records: idx != position raises FLTEE_DEV_ERR_DENSE_ORDER
// (reported, not followed).  packed: one 4-byte load a value, so any 4-byte aligned base; the
// columns past d are never loaded: the padding float of an odd d reaches no output.
// No scratch: the thresholds live in registers, the tile in LDS.
#include "common.h"

namespace fltee {

typedef uint32_t su32x2_t __attribute__((ext_vector_type(2)));

constexpr int kSelThreads = 256;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelInFlight = 4;
// the tile's LDS budget; in front of the tile, the waves' exchange slots (2 x waves x 32 dwords)
constexpr size_t kSelTileBytes = (size_t)64 << 10;
constexpr size_t kSelSlotBytes = 2 * kSelWaves * 32 * 4;

static __device__ __forceinline__ uint32_t sel_ord(float x) {
    const uint32_t b = __float_as_uint(x);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
static __device__ __forceinline__ float sel_value(uint32_t o) {
    return __uint_as_float(o ^ (~(uint32_t)((int32_t)o >> 31) | 0x80000000u));
}

// clients the tile holds: n rounded up to whole rows of G = kSelThreads / C clients
static inline size_t sel_padded_n(size_t n, int C) {
    const size_t G = kSelThreads / C;
    return (n + G - 1) / G * G;
}

// C, a function of n alone: the widest of {32, 16, 8, 4} whose padded tile fits kSelTileBytes
// (n <= 512: 32; <= 1024: 16; <= 2048: 8; <= 4096: 4); 0 past FLTEE_TRIM_SELECT_MAX_N
int trim_select_columns(size_t n) {
    if (n > FLTEE_TRIM_SELECT_MAX_N) return 0;
    for (int C = 32; C >= 4; C /= 2)
        if (sel_padded_n(n, C) * C * 4 <= kSelTileBytes) return C;
    return 0;
}

// stride: bytes between rows (records: 8 d; packed: 8 ceil(d / 2)); npad: sel_padded_n(n, C)
template <bool PACKED, int C>
__global__ __launch_bounds__(kSelThreads) void trim_select_kernel(const uint8_t *__restrict__ in, size_t stride,
                                                                  size_t d, uint32_t n, uint32_t npad, uint32_t t,
                                                                  float coef, float *__restrict__ out,
                                                                  const float *__restrict__ ccoef, int acc_out,
                                                                  uint32_t *__restrict__ status) {
    constexpr int G = kSelThreads / C;
    extern __shared__ uint32_t sel_lds[];
    uint32_t *slot = sel_lds;                      // [2][kSelWaves][32]
    uint32_t *tile = sel_lds + kSelSlotBytes / 4;  // [npad][C]

    const uint32_t tid = threadIdx.x, col = tid % C, g = tid / C, wave = tid / 64;
    const size_t j = (size_t)blockIdx.x * C + col;
    const bool live = j < d;                 // (the last block's columns past d: staged as pads, never stored)
    const bool clip = ccoef != nullptr;      // wave-uniform, public
    uint32_t bad = 0;

    // ---- stage: the n x C tile as ord keys, read from HBM once
    const uint8_t *colp = in + (PACKED ? j * 4 : j * 8);
    for (uint32_t c0 = 0; c0 < npad; c0 += G * kSelInFlight) {
        uint32_t key[kSelInFlight];
        float x[kSelInFlight];
#pragma unroll
        for (int u = 0; u < kSelInFlight; ++u) {
            const uint32_t c = c0 + u * G + g;
            x[u] = 0.0f;
            if (c < n && live) {
                const uint8_t *p = colp + (size_t)c * stride;
                if constexpr (PACKED) {
                    x[u] = __uint_as_float(__builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p)));
                } else {
                    const su32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const su32x2_t *>(p));
                    bad |= v.x ^ (uint32_t)j;
                    x[u] = __uint_as_float(v.y);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kSelInFlight; ++u) {
            const uint32_t c = c0 + u * G + g;
            key[u] = 0xFFFFFFFFu;
            if (c < n && live) key[u] = sel_ord(clip ? __fmul_rn(x[u], ccoef[c]) : x[u]);
            if (c < npad) tile[(size_t)c * C + col] = key[u];
        }
    }
    __syncthreads();

    // ---- the descent: lo = s[t - 1] and hi = s[n - t] together, 32 rounds
    const uint32_t iters = npad / G, k_lo = t - 1, k_hi = n - t;
    const uint32_t *mine = tile + tid;  // this lane's i-th client: mine[i * kSelThreads]
    // the sum of `v` over the column's lanes of the block, in every one of them
    auto column_sum = [&](uint32_t v, uint32_t round) -> uint32_t {
#pragma unroll
        for (int off = C; off < 64; off *= 2) v += (uint32_t)__shfl_xor((int)v, off, 64);
        uint32_t *sl = slot + (round & 1) * (kSelWaves * 32);
        if ((tid & 63) < C) sl[wave * 32 + col] = v;
        __syncthreads();
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < kSelWaves; ++w) sum += sl[w * 32 + col];
        return sum;
    };
    uint32_t p_lo = 0, p_hi = 0;
    for (int b = 31; b >= 0; --b) {
        const uint32_t c_lo = p_lo | (1u << b), c_hi = p_hi | (1u << b);
        uint32_t n_lo = 0, n_hi = 0;
#pragma unroll 8
        for (uint32_t i = 0; i < iters; ++i) {
            const uint32_t x = mine[(size_t)i * kSelThreads];
            n_lo += x < c_lo ? 1u : 0u;
            n_hi += x < c_hi ? 1u : 0u;
        }
        const uint32_t sum = column_sum(n_lo | (n_hi << 16), (uint32_t)b);
        p_lo = (sum & 0xFFFFu) <= k_lo ? c_lo : p_lo;
        p_hi = (sum >> 16) <= k_hi ? c_hi : p_hi;
    }
    // ---- the thresholds' multiplicities inside the trimmed sets
    uint32_t m_lo, m_hi;
    {
        uint32_t below = 0, above = 0;
#pragma unroll 8
        for (uint32_t i = 0; i < iters; ++i) {
            const uint32_t x = mine[(size_t)i * kSelThreads];
            below += x < p_lo ? 1u : 0u;
            above += (i * G + g < n && x > p_hi) ? 1u : 0u;  // (the pad rows: excluded by the public n)
        }
        const uint32_t sum = column_sum(below | (above << 16), 1u);  // (round 0 used slot 0)
        m_lo = t - (sum & 0xFFFFu), m_hi = t - (sum >> 16);
    }

    // ---- the walk: lane col (g = 0) adds its column's kept clients in upload order
    if (g == 0) {  // (public)
        const uint32_t lo = p_lo, hi = p_hi;
        const uint32_t *column = tile + col;
        float acc = 0.0f;
        uint32_t seen_lo = 0, seen_hi = 0;
#pragma unroll 8
        for (uint32_t c = 0; c < n; ++c) {
            const uint32_t o = column[(size_t)c * C];
            const bool eq_lo = o == lo;
            const bool drop_lo = o < lo || (eq_lo && seen_lo < m_lo);
            seen_lo += eq_lo ? 1u : 0u;
            const bool eq_hi = !drop_lo && o == hi;
            const bool drop_hi = !drop_lo && (o > hi || (eq_hi && seen_hi < m_hi));
            seen_hi += eq_hi ? 1u : 0u;
            acc = __fadd_rn(acc, (drop_lo || drop_hi) ? 0.0f : sel_value(o));
        }
        if (live) out[j] = acc_out ? __fadd_rn(out[j], acc) : __fmul_rn(acc, coef);
    }
    if (!PACKED && bad) atomicOr(status, FLTEE_DEV_ERR_DENSE_ORDER);
}

template <bool PACKED, int C>
static hipError_t launch_c(const void *in, size_t stride, size_t n, size_t d, size_t t, float coef, float *out,
                           const float *ccoef, bool acc, uint32_t *status, hipStream_t s) {
    const size_t npad = sel_padded_n(n, C), lds = kSelSlotBytes + npad * C * 4;
    // (a block's LDS past 64 KiB — n > 4032, 1 KiB of slots over the tile — is asked for by name)
    if (lds > ((size_t)64 << 10)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&trim_select_kernel<PACKED, C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    FLTEE_LAUNCH((trim_select_kernel<PACKED, C>), dim3((unsigned)((d + C - 1) / C)), dim3(kSelThreads), lds, s,
                 (const uint8_t *)in, stride, d, (uint32_t)n, (uint32_t)npad, (uint32_t)t, coef, out, ccoef,
                 acc ? 1 : 0, status);
    return hipGetLastError();
}

template <bool PACKED>
static hipError_t launch_by_n(const void *in, size_t stride, size_t n, size_t d, size_t t, float coef, float *out,
                              const float *ccoef, bool acc, uint32_t *status, hipStream_t s) {
    switch (trim_select_columns(n)) {
    case 32: return launch_c<PACKED, 32>(in, stride, n, d, t, coef, out, ccoef, acc, status, s);
    case 16: return launch_c<PACKED, 16>(in, stride, n, d, t, coef, out, ccoef, acc, status, s);
    case 8: return launch_c<PACKED, 8>(in, stride, n, d, t, coef, out, ccoef, acc, status, s);
    case 4: return launch_c<PACKED, 4>(in, stride, n, d, t, coef, out, ccoef, acc, status, s);
    default: return hipErrorInvalidValue;  // (the plan refuses n > FLTEE_TRIM_SELECT_MAX_N)
    }
}

hipError_t launch_trim_select(const void *in, bool packed, size_t n, size_t d, size_t t, float coef, float *out,
                              const float *client_coef, bool accumulate, uint32_t *status, hipStream_t s) {
    if (d == 0) return hipSuccess;
    if (t == 0 || t >= n || 2 * t >= n) return hipErrorInvalidValue;  // (the plan refuses these)
    if (!packed) return launch_by_n<false>(in, d * 8, n, d, t, coef, out, client_coef, accumulate, status, s);
    return launch_by_n<true>(in, RowF32::row_stride(d) * 4, n, d, t, coef, out, client_coef, accumulate, status, s);
}

}  // namespace fltee
