// k_stable.hip — the stable oblivious network of aggregation_alg 7 (gfx950).
//
// The enclave's bubble_sort_based.rs sorts records ++ (i, 0.0) for i < d by idx with a
// STABLE sort, so every index's run reaches the fold in upload order with its zero entry
// last.  Here the same order comes out of a data-independent bitonic network on 16-byte
// records {u64 key; f32 val; u32 pad} (one uint4: x = key low = position, y = key high =
// idx, z = val bits, w = 0) ordered ascending by key = (u64)idx << 32 | position alone.
// Real keys are all distinct, so any correct sorting network yields this one permutation;
// pads are key = ~0, val = +0.0, all identical, so their mutual order is invisible.
//
// Every compare-exchange takes its direction from the global position (bit `stage` of
// it) and is a branch-free select of whole records; no branch, address or trip count
// depends on a key or a value.  Stage blocks made of pads alone (block start >= valid)
// are skipped: they are pads before and after the stage, and the decision depends on L
// and M only.
//
// Three kernels run the network on data[0, m) holding the global positions [pos_base,
// pos_base + m) (pos_base a multiple of m; 0 and the whole array on one GPU, one range of
// a position-sharded array on a multi-GPU eid, group.hip):
//   stable_tile_sort_kernel : stages 1..12 on one tile in LDS (init fused into its loads)
//   stable_global_kernel<R> : R <= 4 steps j >= tile of one stage per HBM pass, 2^R
//                             records in registers per lane, 16-B loads and stores
//   stable_tile_merge_kernel: the steps j < tile of one stage in LDS (strip fused into
//                             the last one's stores)
// and three more serve the ranges alone:
//   stable_exchange_kernel  : one step j >= m of a stage between a range and a copy of
//                             its partner range (two 16-B loads, one 16-B store per lane)
//   stable_init_kernel      : a range's entries (what the fused init makes), on their own
//   stable_strip_kernel     : 16-byte records -> the fold's 8-byte (idx, val)
//
// Tile: 2^12 records = 64 KiB of LDS, 256 lanes x 16 records (2 blocks per CU).  A round
// holds 2^R records per lane (R steps in registers) between one ds_read_b128 and one
// ds_write_b128 per record.  Layout: record e lives in 16-B slot e ^ ((e >> 4) & 15).
// Checked against the bank rules (ds_read_b128: four groups of 16 lanes, each made of
// aligned 4-lane pieces covering every lane residue mod 16 once, 64 banks = 16 slots;
// ds_write_b128: 8 contiguous lanes, 32 banks = 8 slots):
//   steps 0..3  (R = 4): lane t holds e = 16 t + c: slot = c ^ (t & 15) mod 16, distinct
//                        over 16 lanes of distinct residue and over 8 contiguous lanes;
//   steps >= 4         : e = t's low bits in place, so slot = (t & 15) ^ g mod 16 with g
//                        from bits 4..7 of e.  g is one value for the lanes of a group
//                        except that the lanes with t bit 4 set may hold g ^ 1 (bit 4 of
//                        e is t bit 4), which keeps the two lane subsets on disjoint
//                        slots: conflict-free.  The exception: the partial rounds of
//                        stages 6 and 7 (steps 4..5 / 4..6 alone, R = 2 / 3) put t bit 4
//                        on bit 6 / 7 of e and read 2-way conflicted — two rounds of the
//                        first pass, left as they are.
// HBM traffic: every pass reads and writes the live part of the array once, 32 B per
// record (the 8-byte network of `advanced` moves 16).  Passes for M = 2^m > 2^12:
// 1 + sum over stages s = 13..m of (ceil((s - 12) / 4) + 1).
#include "common.h"

namespace fltee {

constexpr uint32_t kStLog = 12, kStTile = 1u << kStLog, kStThreads = 256;
constexpr uint32_t kStPerLane = kStTile / kStThreads;  // 16

__device__ __forceinline__ uint32_t st_slot(uint32_t e) { return e ^ ((e >> 4) & 15u); }

__device__ __forceinline__ uint4 st_pad() { return make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u); }

// a sits at the lower position.  up: the lower position takes the smaller key.
__device__ __forceinline__ void st_cx(uint4 &a, uint4 &b, bool up) {
    const uint64_t ka = ((uint64_t)a.y << 32) | a.x, kb = ((uint64_t)b.y << 32) | b.x;
    const bool sw = up ? ka > kb : ka < kb;
    const uint4 lo = make_uint4(sw ? b.x : a.x, sw ? b.y : a.y, sw ? b.z : a.z, sw ? b.w : a.w);
    const uint4 hi = make_uint4(sw ? a.x : b.x, sw ? a.y : b.y, sw ? a.z : b.z, sw ? a.w : b.w);
    a = lo;
    b = hi;
}

// R steps on 2^R records whose register index is R consecutive position bits
template <int R>
__device__ __forceinline__ void st_butterfly(uint4 (&v)[1 << R], bool up) {
#pragma unroll
    for (int b = R - 1; b >= 0; --b)
#pragma unroll
        for (int c = 0; c < (1 << R); ++c)
            if (!(c & (1 << b))) st_cx(v[c], v[c | (1 << b)], up);
}

// 16-B stores: hipcc may let the next VALU overwrite a dwordx4 store's data registers
// before the store has read them (k_bitonic.hip tl_store2); the fenced "s_nop 1" gives
// the two wait states.
__device__ __forceinline__ void st_store(uint4 *p, const uint4 &v) {
    __builtin_amdgcn_sched_barrier(0);
    *p = v;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 1" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// entry p (a global position) of records ++ (i, +0.0) for i < d ++ pads, keyed
// (idx << 32 | p); rec points at the record of the range's first position, pl = p - that
__device__ __forceinline__ uint4 st_init(const uint64_t *__restrict__ rec, uint32_t nrec, uint32_t d,
                                         uint32_t p, uint32_t pl) {
    if (p < nrec) {
        const uint64_t r = rec[pl];
        return make_uint4(p, (uint32_t)r, (uint32_t)(r >> 32), 0u);
    }
    if (p - nrec < d) return make_uint4(p, p - nrec, 0u, 0u);
    return st_pad();
}

// the 8-byte (idx, val) record of the fold; a pad becomes (u32::MAX, +0.0)
__device__ __forceinline__ uint64_t st_strip(const uint4 &v) { return ((uint64_t)v.z << 32) | v.y; }

// one LDS round: the steps of position bits [jlo, jlo + R) of stage `stage`; pbase: the
// tile's global position (the direction's)
template <int R>
__device__ __forceinline__ void st_round(uint4 *tile, uint32_t jlo, uint32_t t, uint32_t pbase,
                                         uint32_t stage) {
#pragma unroll
    for (uint32_t g = 0; g < (kStPerLane >> R); ++g) {
        const uint32_t q = t + kStThreads * g;
        const uint32_t e0 = (q & ((1u << jlo) - 1u)) | ((q >> jlo) << (jlo + R));
        const bool up = !(((pbase + e0) >> stage) & 1u);
        uint4 v[1 << R];
#pragma unroll
        for (int c = 0; c < (1 << R); ++c) v[c] = tile[st_slot(e0 | ((uint32_t)c << jlo))];
        st_butterfly<R>(v, up);
#pragma unroll
        for (int c = 0; c < (1 << R); ++c) tile[st_slot(e0 | ((uint32_t)c << jlo))] = v[c];
    }
}

// the steps of position bits [0, top) of stage `stage` on the tile (top <= 12), the
// partial round first; every lane of the block calls it
__device__ __forceinline__ void st_tile_steps(uint4 *tile, uint32_t top, uint32_t t, uint32_t pbase,
                                              uint32_t stage) {
    uint32_t hi = top;
    while (hi > 0) {
        const uint32_t lo = (hi - 1u) & ~3u;
        switch (hi - lo) {
        case 1: st_round<1>(tile, lo, t, pbase, stage); break;
        case 2: st_round<2>(tile, lo, t, pbase, stage); break;
        case 3: st_round<3>(tile, lo, t, pbase, stage); break;
        default: st_round<4>(tile, lo, t, pbase, stage); break;
        }
        __syncthreads();
        hi = lo;
    }
}

// tile -> HBM: the 16-byte records, or (out8) the fold's 8-byte records
__device__ __forceinline__ void st_tile_out(const uint4 *tile, uint32_t t, uint32_t pbase, uint32_t m,
                                            uint4 *__restrict__ data, uint64_t *__restrict__ out8) {
#pragma unroll
    for (uint32_t c = 0; c < kStPerLane; ++c) {
        const uint32_t e = t + kStThreads * c, p = pbase + e;
        if (p < m) {
            const uint4 v = tile[st_slot(e)];
            if (out8) out8[p] = st_strip(v);
            else st_store(data + p, v);
        }
    }
}

// Stages 1..12 of every tile.  rec (or d) given: the entries come from st_init instead of
// data.  m < tile: the rest of the tile is filled with pads and sorts behind.  m, valid,
// data, rec and out8 are the range's (local positions); pos_base makes them global.
__global__ __launch_bounds__(256) void stable_tile_sort_kernel(uint4 *__restrict__ data, uint32_t m,
                                                               uint32_t valid, int init,
                                                               const uint64_t *__restrict__ rec,
                                                               uint32_t nrec, uint32_t d,
                                                               uint64_t *__restrict__ out8,
                                                               uint32_t pos_base) {
    __shared__ uint4 tile[kStTile];
    const uint32_t t = threadIdx.x, pbase = blockIdx.x * kStTile;
    if (valid && pbase >= valid) {  // pads alone (public: the position)
        if (init || out8) {
#pragma unroll
            for (uint32_t c = 0; c < kStPerLane; ++c) {
                const uint32_t p = pbase + t + kStThreads * c;
                if (p < m) {
                    if (out8) out8[p] = st_strip(st_pad());
                    else st_store(data + p, st_pad());
                }
            }
        }
        return;
    }
#pragma unroll
    for (uint32_t c = 0; c < kStPerLane; ++c) {
        const uint32_t e = t + kStThreads * c, p = pbase + e;
        uint4 v;
        if (init) v = st_init(rec, nrec, d, pos_base + p, p);
        else v = p < m ? data[p] : st_pad();
        tile[st_slot(e)] = v;
    }
    __syncthreads();
    for (uint32_t stage = 1; stage <= kStLog; ++stage)
        st_tile_steps(tile, stage, t, pos_base + pbase, stage);
    st_tile_out(tile, t, pbase, m, data, out8);
}

// The steps of position bits [jlo, jlo + R), jlo >= 12, of stage `stage`: one lane per
// group of 2^R records 2^jlo apart; consecutive lanes hold consecutive positions.
template <int R>
__global__ __launch_bounds__(256) void stable_global_kernel(uint4 *__restrict__ data, uint32_t jlo,
                                                            uint32_t stage, uint32_t valid,
                                                            uint32_t pos_base) {
    const uint32_t q = blockIdx.x * kStThreads + threadIdx.x;
    const uint32_t p0 = (q & ((1u << jlo) - 1u)) | ((q >> jlo) << (jlo + R));
    if (valid && ((p0 >> stage) << stage) >= valid) return;  // a stage block of pads alone
    const bool up = !(((pos_base + p0) >> stage) & 1u);
    uint4 v[1 << R];
#pragma unroll
    for (int c = 0; c < (1 << R); ++c) v[c] = data[(size_t)(p0 | ((uint32_t)c << jlo))];
    st_butterfly<R>(v, up);
#pragma unroll
    for (int c = 0; c < (1 << R); ++c) st_store(data + (size_t)(p0 | ((uint32_t)c << jlo)), v[c]);
}

// The steps j < tile of stage `stage` (> 12) on every tile.
__global__ __launch_bounds__(256) void stable_tile_merge_kernel(uint4 *__restrict__ data, uint32_t m,
                                                                uint32_t stage, uint32_t valid,
                                                                uint64_t *__restrict__ out8,
                                                                uint32_t pos_base) {
    __shared__ uint4 tile[kStTile];
    const uint32_t t = threadIdx.x, pbase = blockIdx.x * kStTile;
    if (valid && ((pbase >> stage) << stage) >= valid) {  // a stage block of pads alone
        if (out8) {
#pragma unroll
            for (uint32_t c = 0; c < kStPerLane; ++c) out8[pbase + t + kStThreads * c] = st_strip(st_pad());
        }
        return;
    }
#pragma unroll
    for (uint32_t c = 0; c < kStPerLane; ++c) {
        const uint32_t e = t + kStThreads * c;
        tile[st_slot(e)] = data[(size_t)(pbase + e)];
    }
    __syncthreads();
    st_tile_steps(tile, kStLog, t, pos_base + pbase, stage);
    st_tile_out(tile, t, pbase, m, data, out8);
}

// The step j = |pos_mine - pos_theirs| >= m of a stage between a range and a copy of its
// partner's: mine[x] keeps the smaller (take_small) or the larger of (mine[x], theirs[x]) by
// key — a select of the whole record.  take_small is one value for the range: (this range
// is the lower one) == (bit `stage` of its position is 0).  Equal keys (two pads) stay.
__global__ __launch_bounds__(256) void stable_exchange_kernel(uint4 *__restrict__ mine,
                                                              const uint4 *__restrict__ theirs,
                                                              int take_small) {
    const size_t x = (size_t)blockIdx.x * kStThreads + threadIdx.x;
    const uint4 a = mine[x], b = theirs[x];
    const uint64_t ka = ((uint64_t)a.y << 32) | a.x, kb = ((uint64_t)b.y << 32) | b.x;
    const bool sw = take_small ? kb < ka : kb > ka;
    st_store(mine + x, make_uint4(sw ? b.x : a.x, sw ? b.y : a.y, sw ? b.z : a.z, sw ? b.w : a.w));
}

// The entries of global positions [pos_base, pos_base + m) as 16-byte records (st_init).
__global__ __launch_bounds__(256) void stable_init_kernel(uint4 *__restrict__ data,
                                                          const uint64_t *__restrict__ rec,
                                                          uint32_t nrec, uint32_t d, uint32_t pos_base) {
    const uint32_t x = blockIdx.x * kStThreads + threadIdx.x;
    st_store(data + x, st_init(rec, nrec, d, pos_base + x, x));
}

// 16-byte records -> the fold's 8-byte records.
__global__ __launch_bounds__(256) void stable_strip_kernel(const uint4 *__restrict__ data,
                                                           uint64_t *__restrict__ out8) {
    const size_t x = (size_t)blockIdx.x * kStThreads + threadIdx.x;
    out8[x] = st_strip(data[x]);
}

size_t stable_sort_max_records() { return kMaxNetRecords; }

// live records of a pass over stage blocks of 2^stage: the blocks that start below valid
static uint64_t st_live(size_t m, size_t valid, uint32_t stage) {
    if (!valid || valid >= m) return m;
    const uint64_t bs = (uint64_t)1 << stage;
    const uint64_t live = (valid + bs - 1) / bs * bs;
    return live < m ? live : m;
}

// The steps j < m of stage `stage` on the range (every tile; the register passes first when
// m > tile).  valid: the range's live prefix (0: all of it).
static void st_merge_launch(uint4 *data, size_t m, uint32_t stage, uint32_t top, size_t valid,
                            uint32_t v32, uint32_t pos_base, uint64_t *out8, hipStream_t s) {
    const uint32_t tiles = (uint32_t)(m / kStTile);
    const uint64_t live = st_live(m, valid, stage);
    uint32_t hi = top;
    while (hi > kStLog) {
        const uint32_t r = hi - kStLog < 4 ? hi - kStLog : 4, lo = hi - r;
        const dim3 grid((uint32_t)((m >> r) / kStThreads));
        net_account(live * 32, "stable_global", s);
        switch (r) {
        case 1: FLTEE_LAUNCH(stable_global_kernel<1>, grid, dim3(kStThreads), 0, s, data, lo, stage, v32, pos_base); break;
        case 2: FLTEE_LAUNCH(stable_global_kernel<2>, grid, dim3(kStThreads), 0, s, data, lo, stage, v32, pos_base); break;
        case 3: FLTEE_LAUNCH(stable_global_kernel<3>, grid, dim3(kStThreads), 0, s, data, lo, stage, v32, pos_base); break;
        default: FLTEE_LAUNCH(stable_global_kernel<4>, grid, dim3(kStThreads), 0, s, data, lo, stage, v32, pos_base); break;
        }
        hi = lo;
    }
    net_account(live * 16 + (out8 ? (uint64_t)m * 8 : live * 16), "stable_tile_merge", s);
    FLTEE_LAUNCH(stable_tile_merge_kernel, dim3(tiles), dim3(kStThreads), 0, s, data, (uint32_t)m, stage,
                 v32, out8, pos_base);
}

// Stages 1..log2 m of the network in place on data[0, m) = the global positions [pos_base,
// pos_base + m), m = 2^j <= 2^29 (pos_base a multiple of m, pos_base + m <= 2^31).  valid
// (0: unknown): local positions >= valid hold pads.  init: data's entries are made from
// rec (the record of position pos_base first; nrec, d of the whole array) on the way in.
// out8: the sorted range leaves as 8-byte records there instead (data is scratch then).
hipError_t stable_sort_range(void *data16, size_t m, size_t pos_base, hipStream_t s, size_t valid,
                             bool init, const void *rec, size_t nrec, size_t d, uint64_t *out8) {
    if (m == 0 || (m & (m - 1)) || m > stable_sort_max_records()) return hipErrorInvalidValue;
    if (nrec + d >= ((size_t)1 << 31) || pos_base % m || pos_base + m > ((size_t)1 << 31))
        return hipErrorInvalidValue;
    uint4 *data = (uint4 *)data16;
    const uint32_t mlog = log2_pow2(m), pb = (uint32_t)pos_base;
    const uint32_t v32 = valid >= m ? 0u : (uint32_t)valid;
    const uint32_t tiles = m > kStTile ? (uint32_t)(m / kStTile) : 1u;
    const bool one = mlog <= kStLog;
    const size_t nloc = nrec <= pos_base ? 0 : (nrec - pos_base < m ? nrec - pos_base : m);
    net_account((init ? nloc * 8 : st_live(m, valid, kStLog) * 16) +
                    (one && out8 ? m * 8 : st_live(m, valid, kStLog) * 16),
                "stable_tile_sort", s);
    FLTEE_LAUNCH(stable_tile_sort_kernel, dim3(tiles), dim3(kStThreads), 0, s, data, (uint32_t)m, v32,
                 init ? 1 : 0, (const uint64_t *)rec, (uint32_t)nrec, (uint32_t)d,
                 one ? out8 : (uint64_t *)nullptr, pb);
    for (uint32_t stage = kStLog + 1; stage <= mlog; ++stage)
        st_merge_launch(data, m, stage, stage, valid, v32, pb, stage == mlog ? out8 : nullptr, s);
    return hipGetLastError();
}

// the whole array on one GPU
hipError_t stable_sort(void *data16, size_t m, hipStream_t s, size_t valid, bool init, const void *rec,
                       size_t nrec, size_t d, uint64_t *out8) {
    return stable_sort_range(data16, m, 0, s, valid, init, rec, nrec, d, out8);
}

static bool st_range_ok(size_t m, size_t pos_base) {
    return m >= kStTile && !(m & (m - 1)) && m <= stable_sort_max_records() && pos_base % m == 0 &&
           pos_base + m <= ((size_t)1 << 31);
}

// The steps j = m/2 .. 1 of stage 2^stage (> m) on one range: one direction throughout.
hipError_t stable_merge_range(void *data16, size_t m, size_t pos_base, uint32_t stage, hipStream_t s,
                              uint64_t *out8) {
    if (!st_range_ok(m, pos_base) || stage > 31 || ((size_t)1 << stage) <= m) return hipErrorInvalidValue;
    st_merge_launch((uint4 *)data16, m, stage, log2_pow2(m), 0, 0u, (uint32_t)pos_base, out8, s);
    return hipGetLastError();
}

// The step |pos_mine - pos_theirs| of stage 2^stage between a range and a copy of its partner's.
hipError_t stable_exchange(void *mine16, const void *theirs16, size_t m, size_t pos_mine,
                           size_t pos_theirs, uint32_t stage, hipStream_t s) {
    if (!st_range_ok(m, pos_mine) || !st_range_ok(m, pos_theirs) || stage > 31) return hipErrorInvalidValue;
    const size_t j = pos_mine ^ pos_theirs;
    if (j < m || (j & (j - 1)) || j >= ((size_t)1 << stage)) return hipErrorInvalidValue;
    const bool lower = pos_mine < pos_theirs, up = !((pos_mine >> stage) & 1);
    net_account((uint64_t)m * 48, "stable_exchange", s);
    FLTEE_LAUNCH(stable_exchange_kernel, dim3((uint32_t)(m / kStThreads)), dim3(kStThreads), 0, s,
                 (uint4 *)mine16, (const uint4 *)theirs16, lower == up ? 1 : 0);
    return hipGetLastError();
}

hipError_t stable_init_range(const void *rec, size_t nrec, size_t d, size_t pos_base, size_t m,
                             void *dst16, hipStream_t s) {
    if (!st_range_ok(m, pos_base) || nrec + d >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    FLTEE_LAUNCH(stable_init_kernel, dim3((uint32_t)(m / kStThreads)), dim3(kStThreads), 0, s,
                 (uint4 *)dst16, (const uint64_t *)rec, (uint32_t)nrec, (uint32_t)d, (uint32_t)pos_base);
    return hipGetLastError();
}

hipError_t stable_strip_range(const void *data16, size_t m, uint64_t *dst8, hipStream_t s) {
    if (m == 0 || m % kStThreads || m > stable_sort_max_records()) return hipErrorInvalidValue;
    FLTEE_LAUNCH(stable_strip_kernel, dim3((uint32_t)(m / kStThreads)), dim3(kStThreads), 0, s,
                 (const uint4 *)data16, dst8);
    return hipGetLastError();
}

}  // namespace fltee
