// k_gmed.hip — the geometric median of dense uploads (gfx950), oblivious: FLTEE_OPT_GMED.
//
// The smoothed Weiszfeld iteration of RFA (Pillutla, Kakade, Harchaoui 2022) on n clients' dense
// uploads x_c[0, d) (records or f32 rows; FLTEE_OPT_CLIP: __fmul_rn(v, coef_c)), R iterations with
// the smoothing floor nu (include/fltee_agg.h has the definition; the numpy model is
// tests/gmed_model.py).  The iterate z = sum_b w_b x_b / sum_b w_b is never formed: with
// G = X X^T every distance is
//     |x_a - z|^2 = G_aa - 2 (G w)_a / s + w^T G w / s^2,   s = sum w,
// so an iteration is a matvec on an n x n matrix and O(n) scalar work.  The launches:
//
//   krum_gram_kernel, krum_reduce_kernel  (k_krum.hip, launch_krum_gram) G in f64 on the matrix
//       cores, one summation order from (n, d).
//   gmed_init_kernel     valid_c = G_cc is finite (0 / ~0), w_c = valid_c ? 1 : 0.
//   R times:
//   gmed_matvec_kernel   u_a = sum64_b(valid_b ? G_ab w_b : +0.0): a wave a row, 4 rows a block;
//       lane l adds the entries b = l, l + 64, ... in ascending order — sum64's partial p_l,
//       read as 512-byte row segments — the 64 partials go through LDS and lane 0 adds them in
//       ascending l.
//   gmed_update_kernel   one wave: s = sum64(w), q = sum64(valid ? w u : +0.0), inv = s > 0 ?
//       1 / s : 0, then per client D = (G_aa - 2 (u inv)) + (q inv) inv (not finite -> +inf, not
//       above 0 -> +0.0), rho = sqrt(D), w = valid ? 1 / max(nu, rho) : 0, and — of every
//       iteration, the last one's is the call's — alpha = (f32)(s' > 0 ? w / s' : 0) with
//       s' = sum64 of the new w.  The O(n) pieces are this second small launch an iteration (not
//       recomputed in every block of the next matvec).
//   gmed_accumulate_kernel  the dense accumulate with one alpha and one valid word per client: a
//       lane owns W adjacent outputs and adds valid ? __fmul_rn(x, alpha) : +0.0 in upload order
//       (a select: an invalid client's NaN or inf reaches no sum), then k_rows.hip's epilogue
//       with coef 1 (the weights sum to one), or out +=.
//
// f64 arithmetic is __dadd_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn, no contraction.  No grid-wide
// sync, no atomics (but the Gram pass's status word); every loop bound and grid is a function of
// (n, d, R) and the pointers' alignment; valid and the clamps are selects: no data-dependent
// branch, address or trip count.  The weights stay on the device.
#include "common.h"

namespace fltee {

typedef uint32_t gu32x2_t __attribute__((ext_vector_type(2)));

// Krum's partials and G, then [NP] f64 w, u, rho, [NP] f32 alpha, [NP] u32 valid
size_t gmed_scratch_bytes(size_t n, size_t d) {
    const KrumGeom g = krum_geometry(n, d);
    return (g.chunks + 1) * g.np * g.np * 8 + g.np * (3 * 8 + 4 + 4);
}
static double *gmed_w(void *ws, const KrumGeom &g) { return krum_gram(ws, g) + g.np * g.np; }
static double *gmed_u(void *ws, const KrumGeom &g) { return gmed_w(ws, g) + g.np; }
double *gmed_rho(void *ws, size_t n, size_t d) {
    const KrumGeom g = krum_geometry(n, d);
    return gmed_w(ws, g) + 2 * g.np;
}
float *gmed_alpha(void *ws, size_t n, size_t d) {
    const KrumGeom g = krum_geometry(n, d);
    return (float *)(gmed_w(ws, g) + 3 * g.np);
}
uint32_t *gmed_valid(void *ws, size_t n, size_t d) {
    const KrumGeom g = krum_geometry(n, d);
    return (uint32_t *)(gmed_alpha(ws, n, d) + g.np);
}

static __device__ __forceinline__ bool gmed_finite(double x) {
    return fabs(x) < __longlong_as_double(0x7FF0000000000000ll);  // false for NaN
}

// ---- steps 2, 3: the valid words and the first weights ------------------------------------------
__global__ __launch_bounds__(256) void gmed_init_kernel(const double *__restrict__ G, uint32_t np, uint32_t n,
                                                        double *__restrict__ w, uint32_t *__restrict__ valid) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= np) return;
    const bool ok = c < n && gmed_finite(G[(size_t)(c < n ? c : 0) * np + (c < n ? c : 0)]);
    valid[c] = ok ? 0xFFFFFFFFu : 0u;
    w[c] = ok ? 1.0 : 0.0;
}

// ---- step 4: u = G w ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmed_matvec_kernel(const double *__restrict__ G, uint32_t np, uint32_t n,
                                                          const double *__restrict__ w,
                                                          const uint32_t *__restrict__ valid, double *__restrict__ u) {
    __shared__ double part[4][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t a = blockIdx.x * 4 + wave;
    const double *row = G + (size_t)(a < n ? a : 0) * np;  // (a wave past n reads row 0 and stores nothing)
    double p = 0.0;
    for (uint32_t b = lane; b < n; b += 64) {  // (public: n and the lane)
        const double t = __dmul_rn(row[b], w[b]);
        p = __dadd_rn(p, valid[b] != 0 ? t : 0.0);
    }
    part[wave][lane] = p;
    __syncthreads();
    if (lane == 0 && a < n) {
        double s = 0.0;
#pragma unroll 8
        for (int l = 0; l < 64; ++l) s = __dadd_rn(s, part[wave][l]);
        u[a] = s;
    }
}

// ---- step 4, 5: the O(n) pieces -----------------------------------------------------------------
// sum64's combine: the 64 lanes' partials added in ascending lane order; every lane gets the sum
static __device__ __forceinline__ double gmed_combine(double p, double *lds, uint32_t lane) {
    lds[lane] = p;
    __syncthreads();
    double s = 0.0;
#pragma unroll 8
    for (int l = 0; l < 64; ++l) s = __dadd_rn(s, lds[l]);
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(64) void gmed_update_kernel(const double *__restrict__ G, uint32_t np, uint32_t n,
                                                         double nu, double *__restrict__ w,
                                                         const double *__restrict__ u,
                                                         const uint32_t *__restrict__ valid, double *__restrict__ rho,
                                                         float *__restrict__ alpha) {
    __shared__ double lds[64];
    const uint32_t lane = threadIdx.x;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double ps = 0.0, pq = 0.0;
    for (uint32_t a = lane; a < n; a += 64) {
        const double wa = w[a], t = __dmul_rn(wa, u[a]);
        ps = __dadd_rn(ps, wa);
        pq = __dadd_rn(pq, valid[a] != 0 ? t : 0.0);
    }
    const double s = gmed_combine(ps, lds, lane), q = gmed_combine(pq, lds, lane);
    const double inv_s = __ddiv_rn(1.0, s);
    const double inv = s > 0.0 ? inv_s : 0.0;
    const double qi = __dmul_rn(__dmul_rn(q, inv), inv);
    double pn = 0.0;
    for (uint32_t a = lane; a < n; a += 64) {
        const double gaa = G[(size_t)a * np + a];
        double D = __dadd_rn(__dsub_rn(gaa, __dmul_rn(2.0, __dmul_rn(u[a], inv))), qi);
        D = gmed_finite(D) ? D : inf;
        D = D > 0.0 ? D : 0.0;
        const double r = __dsqrt_rn(D);
        const double wn = __ddiv_rn(1.0, r > nu ? r : nu);
        const double wa = valid[a] != 0 ? wn : 0.0;
        w[a] = wa, rho[a] = r;
        pn = __dadd_rn(pn, wa);
    }
    const double s2 = gmed_combine(pn, lds, lane);
    for (uint32_t a = lane; a < n; a += 64) {  // (w[a]: this lane's own store)
        const double t = __ddiv_rn(w[a], s2);
        alpha[a] = __double2float_rn(s2 > 0.0 ? t : 0.0);
    }
}

// ---- step 6: the weighted in-order sum ----------------------------------------------------------
template <bool PACKED, int W, int UC>
__global__ __launch_bounds__(256) void gmed_accumulate_kernel(const uint8_t *__restrict__ in, size_t stride, size_t d,
                                                              uint32_t n, const float *__restrict__ alpha,
                                                              const uint32_t *__restrict__ valid,
                                                              float *__restrict__ out,
                                                              const float *__restrict__ ccoef, int acc_out) {
    const size_t j0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * W;
    if (j0 >= d) return;
    const bool clip = ccoef != nullptr;  // wave-uniform, public
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0.0f;
    for (uint32_t c = 0; c < n; c += UC) {  // (the last batch: guarded by the public n)
        uint32_t x[UC][W];
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (c + u < n) {
                const uint8_t *row = in + (size_t)(c + u) * stride;
                if constexpr (PACKED) {
                    RowF32::load<W>((const float *)row + j0, x[u]);
                } else {
                    static_assert(PACKED || W == 1, "records: one 8-byte record a lane");
                    x[u][0] = __builtin_nontemporal_load(reinterpret_cast<const gu32x2_t *>(row) + j0).y;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (c + u < n) {
                const float cc = clip ? ccoef[c + u] : 1.0f;
                const float al = alpha[c + u];           // one weight and one valid word a client,
                const bool ok = valid[c + u] != 0;       // at fixed addresses
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const float v = __uint_as_float(x[u][w]);
                    const float xv = clip ? __fmul_rn(v, cc) : v;
                    const float y = __fmul_rn(xv, al);
                    acc[w] = __fadd_rn(acc[w], ok ? y : 0.0f);
                }
            }
        }
    }
    rows_store<W>(out, j0, d, acc, 1.0f, acc_out != 0);
}

// ---- launchers ------------------------------------------------------------------------------------
hipError_t launch_gmed_weights(const void *in, bool packed, size_t n, size_t d, size_t iters, double nu,
                               const float *client_coef, void *scratch, uint32_t *status, hipStream_t s) {
    // (the plan refuses these)
    if (n == 0 || n > FLTEE_KRUM_MAX_N || iters == 0 || iters > FLTEE_GMED_MAX_ITERS || !(nu > 0.0) ||
        !(nu < __builtin_inf()))
        return hipErrorInvalidValue;
    if (hipError_t e = launch_krum_gram(in, packed, n, d, client_coef, scratch, status, s)) return e;
    return launch_gmed_iterate(n, d, iters, nu, scratch, s);
}

// steps 2 - 5 on the G in the scratch (krum_gram(scratch, krum_geometry(n, d))): valid, the
// iterations and alpha, where gmed_alpha / gmed_rho / gmed_valid find them
hipError_t launch_gmed_iterate(size_t n, size_t d, size_t iters, double nu, void *scratch, hipStream_t s) {
    if (n == 0 || n > FLTEE_KRUM_MAX_N || iters == 0 || iters > FLTEE_GMED_MAX_ITERS || !(nu > 0.0) ||
        !(nu < __builtin_inf()))
        return hipErrorInvalidValue;
    const KrumGeom g = krum_geometry(n, d);
    const double *G = krum_gram(scratch, g);
    double *w = gmed_w(scratch, g), *u = gmed_u(scratch, g), *rho = gmed_rho(scratch, n, d);
    float *alpha = gmed_alpha(scratch, n, d);
    uint32_t *valid = gmed_valid(scratch, n, d);
    FLTEE_LAUNCH(gmed_init_kernel, dim3((unsigned)((g.np + 255) / 256)), dim3(256), 0, s, G, (uint32_t)g.np,
                 (uint32_t)n, w, valid);
    for (size_t r = 0; r < iters; ++r) {  // (R: the host's loop bound, public)
        FLTEE_LAUNCH(gmed_matvec_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, G, (uint32_t)g.np,
                     (uint32_t)n, (const double *)w, (const uint32_t *)valid, u);
        FLTEE_LAUNCH(gmed_update_kernel, dim3(1), dim3(64), 0, s, G, (uint32_t)g.np, (uint32_t)n, nu, w,
                     (const double *)u, (const uint32_t *)valid, rho, alpha);
    }
    return hipGetLastError();
}

// Fewer outputs than this: 64-lane blocks, one wave a block spread over every CU (k_krum.hip)
constexpr size_t kGmedSmallD = (size_t)1 << 18;

template <bool PACKED, int W, int UC>
static void launch_acc(const void *in, size_t stride, size_t n, size_t d, const float *alpha, const uint32_t *valid,
                       float *out, const float *ccoef, bool acc, hipStream_t s) {
    const size_t groups = (d + W - 1) / W;
    const unsigned nth = d < kGmedSmallD ? 64 : 256;
    FLTEE_LAUNCH((gmed_accumulate_kernel<PACKED, W, UC>), dim3((unsigned)((groups + nth - 1) / nth)), dim3(nth), 0, s,
                 (const uint8_t *)in, stride, d, (uint32_t)n, alpha, valid, out, ccoef, acc ? 1 : 0);
}

hipError_t launch_gmed_accumulate(const void *in, bool packed, size_t n, size_t d, const float *alpha,
                                  const uint32_t *valid, float *out, const float *client_coef, bool accumulate,
                                  hipStream_t s) {
    if (d == 0) return hipSuccess;
    if (!packed) {
        launch_acc<false, 1, 16>(in, d * 8, n, d, alpha, valid, out, client_coef, accumulate, s);
        return hipGetLastError();
    }
    const size_t stride = RowF32::row_stride(d);  // floats
    const int W = rows_width(kRowsF32, in, out, stride, d);
    if (W == 4) launch_acc<true, 4, 8>(in, stride * 4, n, d, alpha, valid, out, client_coef, accumulate, s);
    else if (W == 2) launch_acc<true, 2, 16>(in, stride * 4, n, d, alpha, valid, out, client_coef, accumulate, s);
    else launch_acc<true, 1, 16>(in, stride * 4, n, d, alpha, valid, out, client_coef, accumulate, s);
    return hipGetLastError();
}

}  // namespace fltee
