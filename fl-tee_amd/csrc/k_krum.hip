// k_krum.hip — Multi-Krum of dense uploads (gfx950), oblivious: FLTEE_OPT_KRUM.
//
// n clients' dense uploads x_c[0, d) (records or f32 rows; FLTEE_OPT_CLIP: __fmul_rn(v, coef_c)),
// f assumed Byzantine clients, m clients kept (include/fltee_agg.h has the definition; the
// numpy model is tests/krum_model.py).  Four steps, five launches for n <= 128, six above:
//
//   krum_gram_kernel    G = X X^T in f64 on the matrix cores: v_mfma_f64_16x16x4_f64, one
//       instruction per 16 x 16 tile pair and 4 columns.  A and B take one f64 a lane, lane l
//       holding row (l & 15), column (l >> 4) of the k-step — the same fragment for both
//       operands of a Gram product; the result's layout is the f64 one, col = l & 15,
//       row = (l >> 4) + 4 * reg (not the f32 form's (l >> 4) * 4 + reg).  n is padded to
//       NP = 16 * tiles rows of zeros.  A macro-tile is 8 tiles (128 rows); the grid is
//       (macro-tile pairs MI <= MJ) x (chunks of the column range), the diagonal pairs and —
//       above 128 clients — the pairs MI < MJ in a launch each.  Only tile pairs with
//       row-tile <= col-tile are computed (G is symmetric).  A block of 4 waves stages 16
//       columns of its 128 (diagonal) or 256 rows through LDS as f64 — widened with
//       v_cvt_f64_f32 and clipped on the way, the next stage's loads in flight under the
//       current stage's MFMAs — and its waves split the block's tile pairs round robin: at
//       most 9 (diagonal) or 16 accumulators of 8 registers a wave, independent of each other,
//       which covers the MFMA's dependent latency.  LDS rows are [column][row] with the row
//       dimension padded by 16 doubles, so the 16 lanes of a column are 128 contiguous bytes
//       and the four columns of a k-step start 128 bytes apart modulo the 256-byte bank span.
//       Every block writes its tiles to its chunk's NP x NP partial matrix.
//   krum_reduce_kernel  G[a][b] = the chunks' partials added in ascending chunk order — with
//       the fixed k-step order inside a chunk, the one summation order of every entry, a
//       function of (n, d) alone; no atomics.  Written to [a][b] and [b][a].
//   krum_score_kernel   one block per client a: row a of D = (G[a][a] + G[b][b]) - 2 G[a][b]
//       (NaN, +-inf -> +inf; not above 0 -> +0.0) as order keys in LDS — a non-negative f64's
//       bits order as a u64; the self entry and the pads get the maximum key — sorted by a
//       bitonic network over next_pow2(n) keys; lane 0 adds the first q = n - f - 2 in order.
//   krum_rank_kernel    rank_a = #{b : s_b < s_a or (s_b == s_a and b < a)}, keep_a =
//       rank_a < m ? ~0 : 0: n^2 compares feeding counts.
//   krum_accumulate_kernel  the dense accumulate with one keep word per client: a lane owns W
//       adjacent outputs and adds keep ? x : +0.0 in upload order (a select, never a product:
//       a dropped NaN or inf reaches no sum), then k_rows.hip's epilogue (coef, or out +=).
//
//   krum_reduce_carry_kernel  the same sum as a leg of a chain over column ranges cut on chunk
//       boundaries (launch_krum_gram_range: a multi-GPU eid's ranks, fltee_krum_gram_ranges_device):
//       a range's chunks added, in ascending order, onto the running sum of the ranges before it
//       (the first range: +0.0) — the additions of krum_reduce_kernel, one after the other, on
//       whichever device holds the chunk.
//
// Every value is read at a fixed address, twice (the Gram pass re-reads a macro-tile's rows
// once per partner macro-tile above 128 clients); every loop bound and grid is a function of
// (n, d) and the pointers' alignment; q and m are compare constants; compares feed selects and
// carries: no data-dependent branch, address or early exit.  The keep words stay on the device.
// The records layout checks idx == position in the Gram pass and raises
// FLTEE_DEV_ERR_DENSE_ORDER (reported, not followed), as dense_accumulate_v does.
#include "common.h"

namespace fltee {

typedef double kd4_t __attribute__((ext_vector_type(4)));
typedef uint32_t ku32x2_t __attribute__((ext_vector_type(2)));

constexpr int kKrumKC = 16;             // columns a stage
constexpr int kKrumMacroTiles = 8;      // tiles a macro-tile (128 rows)
constexpr size_t kKrumMinChunk = 256;   // columns: a chunk is never shorter (d permitting)
constexpr size_t kKrumBlocks = 512;     // the grid the chunking aims at: two blocks a CU

KrumGeom krum_geometry(size_t n, size_t d) {
    KrumGeom g;
    g.tiles = (n + 15) / 16;
    g.np = g.tiles * 16;
    g.macros = (g.tiles + kKrumMacroTiles - 1) / kKrumMacroTiles;
    const size_t pairs = g.macros * (g.macros + 1) / 2;
    const size_t target = kKrumBlocks / pairs ? kKrumBlocks / pairs : 1;
    size_t cols = ((d + target - 1) / target + kKrumKC - 1) / kKrumKC * kKrumKC;
    if (cols < kKrumMinChunk) cols = kKrumMinChunk;
    g.chunk_cols = cols;
    g.chunks = d ? (d + cols - 1) / cols : 1;
    return g;
}

// [chunks][NP][NP] f64 partials, [NP][NP] f64 G, [NP] f64 scores, [NP] u32 keep words
size_t krum_scratch_bytes(size_t n, size_t d) {
    const KrumGeom g = krum_geometry(n, d);
    return (g.chunks + 1) * g.np * g.np * 8 + g.np * 8 + g.np * 4;
}
static double *krum_part(void *ws) { return (double *)ws; }
double *krum_gram(void *ws, const KrumGeom &g) { return (double *)ws + g.chunks * g.np * g.np; }
double *krum_scores(void *ws, size_t n, size_t d) {
    const KrumGeom g = krum_geometry(n, d);
    return krum_gram(ws, g) + g.np * g.np;
}
uint32_t *krum_keep(void *ws, size_t n, size_t d) {
    const KrumGeom g = krum_geometry(n, d);
    return (uint32_t *)(krum_scores(ws, n, d) + g.np);
}

// ---- step 1: the Gram matrix ------------------------------------------------------------------
// W: elements a load (records: 1 or 2 records of 8 bytes; packed: 1, 2 or 4 f32)
template <bool PACKED, int W>
static __device__ __forceinline__ void krum_load(const uint8_t *row, size_t j, uint32_t (&r)[PACKED ? W : 2 * W]) {
    if constexpr (PACKED) rows_load<4 * W>(row + j * 4, r);
    else rows_load<8 * W>(row + j * 8, r);
}

// stride: bytes between rows.  OFF: a pair of macro-tiles MI < MJ (256 rows, 8 x TJ tile pairs);
// else the diagonal pair MI = MJ = blockIdx.x (128 rows, the tile pairs la <= lb).
template <bool PACKED, int W, bool OFF>
__global__ __launch_bounds__(256) void krum_gram_kernel(const uint8_t *__restrict__ in, size_t stride, size_t d,
                                                        uint32_t n, uint32_t tiles, uint32_t np, size_t chunk_cols,
                                                        const float *__restrict__ ccoef, double *__restrict__ part,
                                                        uint32_t *__restrict__ status) {
    constexpr int ROWS = OFF ? 256 : 128, ROWSP = ROWS + 16;
    constexpr int MAXS = OFF ? 16 : 9;               // tile pairs a wave: 64 / 4, 36 / 4
    constexpr int GROUPS = kKrumKC / W;              // loads a row and stage
    constexpr int LPT = ROWS * GROUPS / 256;         // loads a lane and stage
    constexpr int RW = PACKED ? W : 2 * W;
    __shared__ double lds[kKrumKC * ROWSP];

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the macro-tile pair (public: the grid)
    uint32_t MI = blockIdx.x, MJ = blockIdx.x;
    if constexpr (OFF) {
        const uint32_t macros = (tiles + kKrumMacroTiles - 1) / kKrumMacroTiles;
        uint32_t rem = blockIdx.x;
        MI = 0;
        while (rem >= macros - 1 - MI) rem -= macros - 1 - MI, ++MI;
        MJ = MI + 1 + rem;
    }
    const uint32_t tj_cnt = min((uint32_t)kKrumMacroTiles, tiles - MJ * kKrumMacroTiles);  // tiles of MJ
    const uint32_t pairs = OFF ? kKrumMacroTiles * tj_cnt : tj_cnt * (tj_cnt + 1) / 2;
    const uint32_t nslots = pairs > wave ? (pairs - wave + 3) / 4 : 0;
    // this wave's tile pairs, as local tiles (MI's at 0.., MJ's at 8.. when OFF)
    uint32_t ta[MAXS], tb[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        const uint32_t p = (uint32_t)s * 4 + wave;
        uint32_t a = 0, b = 0;
        if (p < pairs) {
            if constexpr (OFF) {
                a = p / tj_cnt, b = kKrumMacroTiles + p % tj_cnt;
            } else {
                uint32_t rem = p;
                while (rem >= tj_cnt - a) rem -= tj_cnt - a, ++a;
                b = a + rem;
            }
        }
        ta[s] = __builtin_amdgcn_readfirstlane(a), tb[s] = __builtin_amdgcn_readfirstlane(b);
    }
    kd4_t acc[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) acc[s] = kd4_t{0.0, 0.0, 0.0, 0.0};

    const size_t j_begin = (size_t)blockIdx.y * chunk_cols;
    const size_t j_end = j_begin + chunk_cols < d ? j_begin + chunk_cols : d;
    const uint32_t nst = (uint32_t)((j_end - j_begin + kKrumKC - 1) / kKrumKC);
    const bool clip = ccoef != nullptr;  // wave-uniform, public

    // this lane's loads of a stage: local row, global row, column group
    uint32_t raw[LPT][RW];
    uint32_t bad = 0;
    auto load_stage = [&](uint32_t st) {
        const size_t j0 = j_begin + (size_t)st * kKrumKC;
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const uint32_t e = (uint32_t)i * 256 + tid;
            const uint32_t r = e / GROUPS, col = (e % GROUPS) * W;
            const uint32_t grow = (r < 128 ? MI : MJ) * 128 + (r & 127);
            const size_t j = j0 + col;
#pragma unroll
            for (int w = 0; w < RW; ++w) raw[i][w] = 0;
            // (the whole load lies inside the row: j is W-aligned and the launcher's W rule
            // makes the row's length a multiple of W)
            if (grow < n && j < d) krum_load<PACKED, W>(in + (size_t)grow * stride, j, raw[i]);
        }
    };
    auto store_stage = [&](uint32_t st) {
        const size_t j0 = j_begin + (size_t)st * kKrumKC;
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const uint32_t e = (uint32_t)i * 256 + tid;
            const uint32_t r = e / GROUPS, col = (e % GROUPS) * W;
            const uint32_t grow = (r < 128 ? MI : MJ) * 128 + (r & 127);
            const float cc = (clip && grow < n) ? ccoef[grow] : 1.0f;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const size_t jj = j0 + col + w;
                const bool valid = grow < n && jj < d;
                float v;
                if constexpr (PACKED) {
                    v = __uint_as_float(raw[i][w]);
                } else {
                    v = __uint_as_float(raw[i][2 * w + 1]);
                    bad |= valid ? raw[i][2 * w] ^ (uint32_t)jj : 0u;
                }
                const float x = clip ? __fmul_rn(v, cc) : v;
                lds[(col + w) * ROWSP + r] = (double)(valid ? x : 0.0f);
            }
        }
    };

    if (nst) load_stage(0);
    for (uint32_t st = 0; st < nst; ++st) {
        store_stage(st);
        __syncthreads();
        if (st + 1 < nst) load_stage(st + 1);  // in flight under this stage's MFMAs
#pragma unroll
        for (int ks = 0; ks < kKrumKC / 4; ++ks) {
            const uint32_t base = (ks * 4 + (lane >> 4)) * ROWSP + (lane & 15);
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {
                if ((uint32_t)s < nslots) {
                    const double a = lds[base + ta[s] * 16], b = lds[base + tb[s] * 16];
                    acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[s], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // the partial tiles of this chunk: C/D layout col = lane & 15, row = (lane >> 4) + 4 * reg
    double *P = part + (size_t)blockIdx.y * np * np;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        if ((uint32_t)s < nslots) {
            const uint32_t ga = (MI * kKrumMacroTiles + ta[s]) * 16;
            const uint32_t gb = (OFF ? MJ * kKrumMacroTiles + (tb[s] - kKrumMacroTiles) : MI * kKrumMacroTiles + tb[s]) * 16;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                P[(size_t)(ga + (lane >> 4) + 4 * r) * np + gb + (lane & 15)] = acc[s][r];
        }
    }
    if (!PACKED && bad) atomicOr(status, FLTEE_DEV_ERR_DENSE_ORDER);
}

// G[a][b] = ((+0.0 + P_0[a][b]) + P_1[a][b]) + ... for the tile pairs ta <= tb, mirrored
__global__ __launch_bounds__(256) void krum_reduce_kernel(const double *__restrict__ part, uint32_t np,
                                                          uint32_t chunks, double *__restrict__ G) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, cells = (size_t)np * np;
    if (i >= cells) return;
    const uint32_t a = (uint32_t)(i / np), b = (uint32_t)(i % np);
    if ((a >> 4) > (b >> 4)) return;
    double s = 0.0;
    for (uint32_t c = 0; c < chunks; ++c) s = __dadd_rn(s, part[(size_t)c * cells + i]);
    G[i] = s;
    if ((a >> 4) != (b >> 4)) G[(size_t)b * np + a] = s;
}

// A leg of the chain: S[a][b] = ((carry[a][b] + P_0[a][b]) + P_1[a][b]) + ... over this range's chunks;
// carry = the running sum of the ranges before it (null: +0.0, the first range).  Every leg mirrors
// its tile pairs, so S is a whole matrix wherever the chain ends.  S may be carry (a cell is read
// and written by one lane; the mirrored cells are read by none).
__global__ __launch_bounds__(256) void krum_reduce_carry_kernel(const double *__restrict__ part, uint32_t np,
                                                                uint32_t chunks, const double *carry, double *S) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, cells = (size_t)np * np;
    if (i >= cells) return;
    const uint32_t a = (uint32_t)(i / np), b = (uint32_t)(i % np);
    if ((a >> 4) > (b >> 4)) return;
    double s = carry ? carry[i] : 0.0;
    for (uint32_t c = 0; c < chunks; ++c) s = __dadd_rn(s, part[(size_t)c * cells + i]);
    S[i] = s;
    if ((a >> 4) != (b >> 4)) S[(size_t)b * np + a] = s;
}

// ---- step 2, 3: distances and scores ----------------------------------------------------------
__global__ __launch_bounds__(1024) void krum_score_kernel(const double *__restrict__ G, uint32_t np, uint32_t n,
                                                          uint32_t q, double *__restrict__ scores) {
    __shared__ uint64_t keys[1024];
    const uint32_t a = blockIdx.x, t = threadIdx.x, P = blockDim.x;
    uint64_t key = ~0ull;  // the self entry and the pads: behind every distance, +inf included
    if (t < n && t != a) {
        const double gaa = G[(size_t)a * np + a], gbb = G[(size_t)t * np + t], gab = G[(size_t)a * np + t];
        double D = __dsub_rn(__dadd_rn(gaa, gbb), __dmul_rn(2.0, gab));
        const bool finite = fabs(D) < __longlong_as_double(0x7FF0000000000000ll);  // false for NaN
        D = finite ? D : __longlong_as_double(0x7FF0000000000000ll);
        D = D > 0.0 ? D : 0.0;
        key = (uint64_t)__double_as_longlong(D);
    }
    keys[t] = key;
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t p = t ^ j;
            if (p > t) {  // (positions: public)
                const uint64_t x = keys[t], y = keys[p];
                const bool sw = ((t & k) == 0) ? x > y : x < y;
                keys[t] = sw ? y : x;
                keys[p] = sw ? x : y;
            }
            __syncthreads();
        }
    }
    if (t == 0) {
        double s = 0.0;
        for (uint32_t i = 0; i + 1 < n; ++i) {  // every distance is visited; q is a compare constant
            const double v = __longlong_as_double((long long)keys[i]);
            const double s1 = __dadd_rn(s, v);
            s = i < q ? s1 : s;
        }
        scores[a] = s;
    }
}

// ---- step 4: the ranking ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void krum_rank_kernel(const double *__restrict__ scores, uint32_t n, uint32_t m,
                                                        uint32_t *__restrict__ keep) {
    const uint32_t a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const double sa = scores[a];
    uint32_t rank = 0;
    for (uint32_t b = 0; b < n; ++b) {
        const double sb = scores[b];
        rank += (sb < sa || (sb == sa && b < a)) ? 1u : 0u;
    }
    keep[a] = rank < m ? 0xFFFFFFFFu : 0u;
}

// ---- step 5: the kept clients' in-order sum ----------------------------------------------------
template <bool PACKED, int W, int UC>
__global__ __launch_bounds__(256) void krum_accumulate_kernel(const uint8_t *__restrict__ in, size_t stride, size_t d,
                                                              uint32_t n, const uint32_t *__restrict__ keep,
                                                              float coef, float *__restrict__ out,
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
                    x[u][0] = __builtin_nontemporal_load(reinterpret_cast<const ku32x2_t *>(row) + j0).y;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            if (c + u < n) {
                const float cc = clip ? ccoef[c + u] : 1.0f;
                const bool kept = keep[c + u] != 0;  // one word a client, a fixed address
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const float v = __uint_as_float(x[u][w]);
                    const float xv = clip ? __fmul_rn(v, cc) : v;
                    acc[w] = __fadd_rn(acc[w], kept ? xv : 0.0f);
                }
            }
        }
    }
    rows_store<W>(out, j0, d, acc, coef, acc_out != 0);
}

// ---- launchers ----------------------------------------------------------------------------------
template <bool PACKED, int W>
static void launch_gram(const void *in, size_t stride, size_t n, size_t d, const KrumGeom &g, const float *ccoef,
                        double *part, uint32_t *status, hipStream_t s) {
    FLTEE_LAUNCH((krum_gram_kernel<PACKED, W, false>), dim3((unsigned)g.macros, (unsigned)g.chunks), dim3(256), 0, s,
                 (const uint8_t *)in, stride, d, (uint32_t)n, (uint32_t)g.tiles, (uint32_t)g.np, g.chunk_cols, ccoef,
                 part, status);
    if (g.macros > 1)
        FLTEE_LAUNCH((krum_gram_kernel<PACKED, W, true>),
                     dim3((unsigned)(g.macros * (g.macros - 1) / 2), (unsigned)g.chunks), dim3(256), 0, s,
                     (const uint8_t *)in, stride, d, (uint32_t)n, (uint32_t)g.tiles, (uint32_t)g.np, g.chunk_cols,
                     ccoef, part, status);
}

// steps 1 and the reduce: G (NP x NP f64, krum_geometry(n, d)'s NP) from the chunks' partials; the
// scratch's first (chunks + 1) NP^2 doubles.  Shared with the geometric median (k_gmed.hip).
hipError_t launch_krum_gram(const void *in, bool packed, size_t n, size_t d, const float *client_coef, void *scratch,
                            uint32_t *status, hipStream_t s) {
    if (n == 0 || n > FLTEE_KRUM_MAX_N || d >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    const KrumGeom g = krum_geometry(n, d);
    double *part = krum_part(scratch), *G = krum_gram(scratch, g);
    const uintptr_t a = (uintptr_t)in;
    if (packed) {
        const size_t stride = RowF32::row_stride(d);  // floats
        if (a % 16 == 0 && stride % 4 == 0) launch_gram<true, 4>(in, stride * 4, n, d, g, client_coef, part, status, s);
        else if (a % 8 == 0) launch_gram<true, 2>(in, stride * 4, n, d, g, client_coef, part, status, s);
        else launch_gram<true, 1>(in, stride * 4, n, d, g, client_coef, part, status, s);
    } else {
        if (a % 16 == 0 && d % 2 == 0) launch_gram<false, 2>(in, d * 8, n, d, g, client_coef, part, status, s);
        else launch_gram<false, 1>(in, d * 8, n, d, g, client_coef, part, status, s);
    }
    FLTEE_LAUNCH(krum_reduce_kernel, dim3((unsigned)((g.np * g.np + 255) / 256)), dim3(256), 0, s, part,
                 (uint32_t)g.np, (uint32_t)g.chunks, G);
    return hipGetLastError();
}

// The Gram pass of a column range cut on chunk boundaries.  g: the geometry of the WHOLE call,
// krum_geometry(n, d) — the chunk length and NP; in: the range's first column of client 0, stride:
// bytes between clients (a rank's own n x cols slice, or a range of whole rows), cols: the range's
// columns, chunks = ceil(cols / g.chunk_cols) > 0 of them; part: chunks x NP x NP doubles.  The
// kernels and the k-step order inside a chunk are launch_krum_gram's.  A records range holds
// range-local indices (idx == column - first column).
hipError_t launch_krum_gram_range(const void *in, bool packed, size_t stride, size_t n, size_t cols, const KrumGeom &g,
                                  size_t chunks, const float *client_coef, double *part, uint32_t *status,
                                  hipStream_t s) {
    if (n == 0 || n > FLTEE_KRUM_MAX_N || cols >= ((size_t)1 << 31) || chunks == 0 ||
        chunks != (cols + g.chunk_cols - 1) / g.chunk_cols || g.np != (n + 15) / 16 * 16)
        return hipErrorInvalidValue;
    KrumGeom r = g;
    r.chunks = chunks;  // (the grid's y; the kernels take the chunk length and the range's columns)
    const uintptr_t a = (uintptr_t)in;
    // the load widths of launch_krum_gram, with every row's start as aligned as the first
    if (packed) {
        if (a % 16 == 0 && stride % 16 == 0) launch_gram<true, 4>(in, stride, n, cols, r, client_coef, part, status, s);
        else if (a % 8 == 0 && stride % 8 == 0) launch_gram<true, 2>(in, stride, n, cols, r, client_coef, part, status, s);
        else launch_gram<true, 1>(in, stride, n, cols, r, client_coef, part, status, s);
    } else {
        if (a % 16 == 0 && stride % 16 == 0 && cols % 2 == 0)
            launch_gram<false, 2>(in, stride, n, cols, r, client_coef, part, status, s);
        else launch_gram<false, 1>(in, stride, n, cols, r, client_coef, part, status, s);
    }
    return hipGetLastError();
}

// The range's leg of the chain: sum (NP x NP) = carry (the running sum of the ranges before it;
// null: +0.0, the first range) with the range's chunks added in ascending order.  Ranges in
// ascending order: the additions of krum_reduce_kernel one after the other, so the last range's
// sum is launch_krum_gram's G bit for bit.
hipError_t launch_krum_reduce_carry(const double *part, size_t np, size_t chunks, const double *carry, double *sum,
                                    hipStream_t s) {
    if (np == 0 || np > FLTEE_KRUM_MAX_N || chunks == 0) return hipErrorInvalidValue;
    FLTEE_LAUNCH(krum_reduce_carry_kernel, dim3((unsigned)((np * np + 255) / 256)), dim3(256), 0, s, part,
                 (uint32_t)np, (uint32_t)chunks, carry, sum);
    return hipGetLastError();
}

// steps 2 - 4 on the G in the scratch (krum_gram(scratch, krum_geometry(n, d))): the scores and the
// keep words, where krum_scores / krum_keep find them
hipError_t launch_krum_rank(size_t n, size_t d, size_t f, size_t m, void *scratch, hipStream_t s) {
    if (n > FLTEE_KRUM_MAX_N || n < 2 * f + 3 || m == 0 || m > n - f) return hipErrorInvalidValue;
    const KrumGeom g = krum_geometry(n, d);
    double *G = krum_gram(scratch, g), *scores = krum_scores(scratch, n, d);
    uint32_t *keep = krum_keep(scratch, n, d);
    size_t P = 64;
    while (P < n) P <<= 1;
    FLTEE_LAUNCH(krum_score_kernel, dim3((unsigned)n), dim3((unsigned)P), 0, s, G, (uint32_t)g.np, (uint32_t)n,
                 (uint32_t)(n - f - 2), scores);
    FLTEE_LAUNCH(krum_rank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scores, (uint32_t)n,
                 (uint32_t)m, keep);
    return hipGetLastError();
}

hipError_t launch_krum_select(const void *in, bool packed, size_t n, size_t d, size_t f, size_t m,
                              const float *client_coef, void *scratch, uint32_t *status, hipStream_t s) {
    // (the plan refuses these)
    if (n > FLTEE_KRUM_MAX_N || n < 2 * f + 3 || m == 0 || m > n - f || d >= ((size_t)1 << 31))
        return hipErrorInvalidValue;
    if (hipError_t e = launch_krum_gram(in, packed, n, d, client_coef, scratch, status, s)) return e;
    return launch_krum_rank(n, d, f, m, scratch, s);
}

// Fewer outputs than this: 64-lane blocks, one wave a block spread over every CU (k_trim.hip)
constexpr size_t kKrumSmallD = (size_t)1 << 18;

template <bool PACKED, int W, int UC>
static void launch_acc(const void *in, size_t stride, size_t n, size_t d, const uint32_t *keep, float coef, float *out,
                       const float *ccoef, bool acc, hipStream_t s) {
    const size_t groups = (d + W - 1) / W;
    const unsigned nth = d < kKrumSmallD ? 64 : 256;
    FLTEE_LAUNCH((krum_accumulate_kernel<PACKED, W, UC>), dim3((unsigned)((groups + nth - 1) / nth)), dim3(nth), 0, s,
                 (const uint8_t *)in, stride, d, (uint32_t)n, keep, coef, out, ccoef, acc ? 1 : 0);
}

hipError_t launch_krum_accumulate(const void *in, bool packed, size_t n, size_t d, const uint32_t *keep, float coef,
                                  float *out, const float *client_coef, bool accumulate, hipStream_t s) {
    if (d == 0) return hipSuccess;
    if (!packed) {
        launch_acc<false, 1, 16>(in, d * 8, n, d, keep, coef, out, client_coef, accumulate, s);
        return hipGetLastError();
    }
    const size_t stride = RowF32::row_stride(d);  // floats
    const int W = rows_width(kRowsF32, in, out, stride, d);
    if (W == 4) launch_acc<true, 4, 8>(in, stride * 4, n, d, keep, coef, out, client_coef, accumulate, s);
    else if (W == 2) launch_acc<true, 2, 16>(in, stride * 4, n, d, keep, coef, out, client_coef, accumulate, s);
    else launch_acc<true, 1, 16>(in, stride * 4, n, d, keep, coef, out, client_coef, accumulate, s);
    return hipGetLastError();
}

}  // namespace fltee
