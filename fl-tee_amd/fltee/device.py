"""Device-resident entry points of libfltee_agg.so on torch tensors.

PyTorch only supplies HBM allocations, the stream and torch.distributed; all
arithmetic runs in the library's HIP kernels.  Records are int64 tensors whose
bytes are the enclave's Weight layout (parameters.rs:9): low 32 bits u32 idx,
high 32 bits f32 val (little-endian), client-major in upload order.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L


def _stream(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def pack_records(idx, val):
    """(u32 idx, f32 val) arrays -> int64 numpy array of Weight records."""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    val = np.ascontiguousarray(val, dtype=np.float32)
    rec = np.empty(len(idx), dtype=np.uint64)
    rec[:] = idx.astype(np.uint64) | (val.view(np.uint32).astype(np.uint64) << np.uint64(32))
    return rec.view(np.int64)


def unpack_records(rec):
    r = np.ascontiguousarray(rec).view(np.uint64)
    return (r & np.uint64(0xFFFFFFFF)).astype(np.uint32), (r >> np.uint64(32)).astype(np.uint32).view(np.float32)


def opts(*, dense=False, dp=False, clip=False, accumulate=False, no_average=False, sigma=1.12,
         clipping=1.0, seed=0, k_req=None, batch=0, n_avg=0, fold_halo=0, status=None,
         oram_tree=False, oram_lazy=False, packed=False, trim=None, bf16=False, trim_select=False,
         fp8=False, krum=None, gmed=None):
    if krum is not None and gmed is not None:  # (two structs, one pointer; the plan refuses the pair anyway)
        raise ValueError("krum= and gmed= are alternatives")
    o = L.DeviceOptsKrum() if krum is not None else L.DeviceOptsGmed() if gmed is not None else L.DeviceOpts()
    o.flags = ((L.OPT_DENSE if dense else 0) | (L.OPT_DP if dp else 0) | (L.OPT_CLIP if clip else 0)
               | (L.OPT_ACCUMULATE if accumulate else 0) | (L.OPT_NO_AVERAGE if no_average else 0)
               | (L.OPT_ORAM_TREE if oram_tree else 0) | (L.OPT_ORAM_LAZY if oram_lazy else 0)
               | (L.OPT_PACKED if packed else 0) | (L.OPT_BF16 if bf16 else 0) | (L.OPT_FP8 if fp8 else 0))
    o.sigma, o.clipping, o.seed = sigma, clipping, seed
    if k_req is not None:
        o.flags |= L.OPT_K_REQ
        o.k_req = k_req
    o.batch, o.n_avg, o.fold_halo = batch, n_avg, fold_halo
    if trim is not None:  # the trimmed mean of a dense call: trim clients removed on each side
        o.flags |= L.OPT_TRIM
        o.trim = trim
    if trim_select:  # ... by selection: any trim with 2 * trim < n, n <= TRIM_SELECT_MAX_N
        o.flags |= L.OPT_TRIM_SELECT
    if krum is not None:  # Multi-Krum of a dense call: (f assumed Byzantine clients, m clients kept)
        o.flags |= L.OPT_KRUM
        o.krum_f, o.krum_m = krum
    if gmed is not None:  # the geometric median of a dense call: (Weiszfeld iterations R, smoothing floor nu)
        o.flags |= L.OPT_GMED
        o.gmed_iters, o.gmed_nu = gmed
    o.d_status = status.data_ptr() if status is not None else None
    return o


def _check(st, what):
    if st != L.SUCCESS:
        raise RuntimeError(f"{what} failed with status {st:#x}")


def aggregate(alg, records, n, k, d, out=None, stream=None, **kw):
    """fltee_aggregate_device: aggregate n x k records (int64 cuda tensor) into out[d] (f32).
    packed=True: records is n packed slices instead (any cuda tensor of n * packed_row(d)
    f32's worth of bytes: client c's d values, then one ignored f32 when d is odd; k == d).
    bf16=True: n bf16 slices (n * bf16_row(d) halves' worth of bytes, 2-byte aligned).
    fp8=True: n fp8 slices (n * fp8_row(d) bytes, 4-byte aligned).
    krum=(f, m): Multi-Krum of a dense call on algs 3, 4, 5 — the m clients with the smallest sums
    of squared distances to their n - f - 2 nearest neighbours, averaged whole.
    gmed=(R, nu): the geometric median of a dense call on algs 3, 4, 5 — R smoothed Weiszfeld
    iterations with the floor nu, every valid client kept with a weight 1 / max(nu, distance)."""
    if kw.get("fp8"):
        assert records.is_cuda and records.numel() * records.element_size() >= n * fp8_row(d)
    elif kw.get("bf16"):
        assert records.is_cuda and records.numel() * records.element_size() >= n * bf16_row(d) * 2
    elif kw.get("packed"):
        assert records.is_cuda and records.numel() * records.element_size() >= n * packed_row(d) * 4
    else:
        assert records.is_cuda and records.dtype == torch.int64 and records.numel() >= n * k
    if out is None:
        out = torch.empty(d, dtype=torch.float32, device=records.device)
    o = opts(**kw)
    st = L.lib().fltee_aggregate_device(alg, _ptr(records), n, k, d, _ptr(out), ctypes.byref(o),
                                        _stream(stream))
    _check(st, "fltee_aggregate_device")
    return out


def krum_select(records, n, d, f, m, stream=None, **kw):
    """fltee_krum_select_device: Multi-Krum's scores and selection alone, on n dense uploads of
    d parameters (records, or packed= / bf16= / fp8= rows; clip= with clipping=) ->
    (scores float64 [n], keep int32 [n]: 0 or -1), cuda tensors."""
    assert records.is_cuda
    o = opts(krum=(f, m), **kw)
    scores = torch.empty(n, dtype=torch.float64, device=records.device)
    keep = torch.empty(n, dtype=torch.int32, device=records.device)
    _check(L.lib().fltee_krum_select_device(_ptr(records), n, d, ctypes.byref(o), _ptr(scores), _ptr(keep),
                                            _stream(stream)), "fltee_krum_select_device")
    return scores, keep


def krum_gram_ranges(records, n, d, ranks, packed=False):
    """fltee_krum_gram_ranges_device: the Gram matrix of n dense uploads of d parameters (records,
    or packed=True f32 rows) computed over `ranks` column ranges cut on the Gram pass's chunk
    boundaries and combined by the carry chain, as an eid over `ranks` GPUs does -> G float64
    [NP, NP], NP = 16 * ceil(n / 16), a cuda tensor: the one-GPU pass's bits for any ranks.  Runs
    on the current device's null stream.  What the library refuses by host arithmetic (ranks
    outside 1 .. 64, n outside 1 .. KRUM_MAX_N, d >= 2^31) raises ValueError here, before any
    allocation."""
    if not 1 <= ranks <= 64 or not 1 <= n <= L.KRUM_MAX_N or not 0 <= d < 1 << 31:
        raise ValueError(f"fltee_krum_gram_ranges_device refuses n={n}, d={d}, ranks={ranks}")
    assert records.is_cuda
    npad = (n + 15) // 16 * 16
    G = torch.empty((npad, npad), dtype=torch.float64, device=records.device)
    _check(L.lib().fltee_krum_gram_ranges_device(_ptr(records), 1 if packed else 0, n, d, ranks, _ptr(G)),
           "fltee_krum_gram_ranges_device")
    return G


def gmed_weights(records, n, d, iters, nu, stream=None, **kw):
    """fltee_gmed_weights_device: the geometric median's weights alone, on n dense uploads of d
    parameters (records, or packed= / bf16= / fp8= rows; clip= with clipping=) ->
    (alpha float32 [n], rho float64 [n]: the last iteration's distances), cuda tensors."""
    assert records.is_cuda
    o = opts(gmed=(iters, nu), **kw)
    alpha = torch.empty(n, dtype=torch.float32, device=records.device)
    rho = torch.empty(n, dtype=torch.float64, device=records.device)
    _check(L.lib().fltee_gmed_weights_device(_ptr(records), n, d, ctypes.byref(o), _ptr(alpha), _ptr(rho),
                                             _stream(stream)), "fltee_gmed_weights_device")
    return alpha, rho


def packed_row(d):
    """f32 slots of one packed slice of d parameters: 2 * ceil(d / 2)."""
    return (d + 1) // 2 * 2


def bf16_row(d):
    """bf16 slots of one bf16 slice of d parameters: 4 * ceil(d / 4)."""
    return (d + 3) // 4 * 4


def fp8_row(d):
    """bytes of one fp8 slice of d parameters: 8 * (ceil(d / 8) + 1) — the codes, padding up
    to the unit, then the unit that holds the f32 scale."""
    return ((d + 7) // 8 + 1) * 8


def _unpack_rows(what, rows, row_bytes, n, d, records, stream):
    assert rows.is_cuda and rows.is_contiguous()
    assert rows.numel() * rows.element_size() >= n * row_bytes
    if records is None:
        records = torch.empty(n * d, dtype=torch.int64, device=rows.device)
    _check(getattr(L.lib(), what)(_ptr(rows), n, d, _ptr(records), _stream(stream)), what)
    return records


def unpack_dense(packed, n, d, records=None, stream=None):
    """fltee_unpack_dense_device: n packed slices ([n, packed_row(d)] f32) -> int64 records
    [n * d]: (j, v[j]) per client."""
    return _unpack_rows("fltee_unpack_dense_device", packed, packed_row(d) * 4, n, d, records, stream)


def unpack_bf16(rows, n, d, records=None, stream=None):
    """fltee_unpack_bf16_device: n bf16 slices ([n, bf16_row(d)] halves) -> int64 records
    [n * d]: (j, widen(h[j])) per client."""
    return _unpack_rows("fltee_unpack_bf16_device", rows, bf16_row(d) * 2, n, d, records, stream)


def unpack_fp8(rows, n, d, records=None, stream=None):
    """fltee_unpack_fp8_device: n fp8 slices ([n, fp8_row(d)] bytes) -> int64 records
    [n * d]: (j, w(q[j]) * s) per client."""
    return _unpack_rows("fltee_unpack_fp8_device", rows, fp8_row(d), n, d, records, stream)


def reserve(alg, n, k, d, **kw):
    o = opts(**kw)
    _check(L.lib().fltee_reserve(alg, n, k, d, ctypes.byref(o)), "fltee_reserve")


def workspace_bytes(alg, n, k, d, **kw):
    o = opts(**kw)
    return L.lib().fltee_workspace_bytes(alg, n, k, d, ctypes.byref(o))


def status(stream=None):
    """Synchronise and return (and clear) the library-owned device status word."""
    v = ctypes.c_uint32(0)
    _check(L.lib().fltee_device_status(_stream(stream), ctypes.byref(v)), "fltee_device_status")
    return v.value


def bitonic(records, mode, seed=0, stream=None):
    m = records.numel()
    _check(L.lib().fltee_bitonic_device(_ptr(records), m, mode, seed, _stream(stream)),
           "fltee_bitonic_device")
    return records


def stable_sort(records16, stream=None):
    """fltee_stable_sort_device: alg 7's network in place on 16-byte records {u64 key; f32
    val; u32 pad} (any tensor whose bytes are m = 2^j such records), ascending by key."""
    nbytes = records16.numel() * records16.element_size()
    assert records16.is_cuda and records16.is_contiguous() and nbytes % 16 == 0
    _check(L.lib().fltee_stable_sort_device(_ptr(records16), nbytes // 16, _stream(stream)),
           "fltee_stable_sort_device")
    return records16


def fold(src, dst, fold_len, halo, status_word, stream=None):
    _check(L.lib().fltee_fold_device(_ptr(src), _ptr(dst), src.numel(), fold_len, halo,
                                     _ptr(status_word), _stream(stream)), "fltee_fold_device")
    return dst


def decrypt(client_ids, cipher, bytes_per_client, records, stream=None):
    ids = np.ascontiguousarray(client_ids, dtype=np.uint32)
    _check(L.lib().fltee_decrypt_device(ids.ctypes.data_as(ctypes.c_void_p), len(ids),
                                        _ptr(cipher), bytes_per_client, _ptr(records),
                                        _stream(stream)), "fltee_decrypt_device")
    return records


def decrypt_auth(client_ids, cipher, ct_bytes, iv, aad=b"", records=None, stream=None):
    """AES-128-GCM decrypt of n slices of (ct_bytes || 16-byte tag): (records, fail) with
    fail[c] = 1 where client c's tag did not verify (FLTEE_DEV_ERR_AUTH is then set in the
    status word)."""
    ids = np.ascontiguousarray(client_ids, dtype=np.uint32)
    n = len(ids)
    assert len(iv) == 12 and len(aad) % max(n, 1) == 0
    if records is None:
        records = torch.empty(max(n * (ct_bytes // 8), 1), dtype=torch.int64, device=cipher.device)
    fail = torch.full((max(n, 1),), 0x7fffffff, dtype=torch.int32, device=cipher.device)
    ivb = (ctypes.c_uint8 * 12)(*iv)
    aadb = (ctypes.c_uint8 * max(len(aad), 1))(*aad)
    _check(L.lib().fltee_decrypt_auth_device(ids.ctypes.data_as(ctypes.c_void_p), n, _ptr(cipher),
                                             ct_bytes, ivb, aadb, len(aad) // max(n, 1),
                                             _ptr(records), _ptr(fail), _stream(stream)),
           "fltee_decrypt_auth_device")
    return records[:n * (ct_bytes // 8)], fail[:n]


def gather_clients(records, keep, out=None, stream=None):
    """fltee_gather_clients_device: the slices keep[0], keep[1], ... (ascending client
    positions) of records, an (n, k) int64 cuda tensor of client-major records, compacted into
    out (len(keep), k) — a second buffer, never records itself.  keep: a cuda int32 tensor, or
    host integers (uploaded here)."""
    assert records.is_cuda and records.dtype == torch.int64 and records.dim() == 2
    n, k = records.shape
    assert records.stride(1) == 1 and records.stride(0) == k, "client-major, slices back to back"
    if not torch.is_tensor(keep):
        keep = torch.from_numpy(np.ascontiguousarray(keep, dtype=np.int32))
    keep = keep.to(device=records.device, dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty((keep.numel(), k), dtype=torch.int64, device=records.device)
    assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= keep.numel() * k
    # an empty tensor may have a null data pointer: the library refuses those before it looks at n_keep
    anchor = records if keep.numel() == 0 else keep
    _check(L.lib().fltee_gather_clients_device(_ptr(records), n, k, _ptr(anchor), keep.numel(),
                                               _ptr(out if out.numel() else records), _stream(stream)),
           "fltee_gather_clients_device")
    return out


def gcm_segments(ct_bytes, aad_len):
    """fltee_gcm_segments: GHASH partials per client of a slice of ct_bytes with aad_len of AAD."""
    return L.lib().fltee_gcm_segments(ct_bytes, aad_len)


def ghash_window(client_ids, window, row_stride, ct_bytes, first_block, win_bytes, aad=b"",
                 aad_len=None, with_aad=False, part=None, stream=None):
    """fltee_ghash_window_device: the GHASH partials (uint8 [n, P, 16]) of one window of n
    slices — ciphertext blocks [first_block, first_block + ceil(win_bytes / 16)) of each, rows
    of `window` at row_stride bytes.  aad_len is the slices' AAD length (it shapes the segment
    layout); aad (n x aad_len bytes) is hashed by the one window that passes with_aad."""
    ids = np.ascontiguousarray(client_ids, dtype=np.uint32)
    n = len(ids)
    if aad_len is None:
        aad_len = len(aad) // max(n, 1)
    P = gcm_segments(ct_bytes, aad_len)
    if part is None:
        part = torch.empty((n, P, 16), dtype=torch.uint8, device=window.device)
    aadb = (ctypes.c_uint8 * max(len(aad), 1))(*aad)
    _check(L.lib().fltee_ghash_window_device(ids.ctypes.data_as(ctypes.c_void_p), n, _ptr(window),
                                             row_stride, ct_bytes, first_block, win_bytes, aadb, aad_len,
                                             1 if with_aad else 0, _ptr(part), _stream(stream)),
           "fltee_ghash_window_device")
    return part


def ghash_merge(acc, part, stream=None):
    """fltee_ghash_merge_device: acc ^= part (two [n, P, 16] partial vectors)."""
    assert acc.shape == part.shape and acc.is_contiguous() and part.is_contiguous()
    n, P = acc.shape[0], acc.shape[1]
    _check(L.lib().fltee_ghash_merge_device(_ptr(acc), _ptr(part), n, P, _stream(stream)),
           "fltee_ghash_merge_device")
    return acc


def gcm_finish(client_ids, part, ct_bytes, iv, aad_len, tags, stream=None):
    """fltee_gcm_finish_device: the merged partials against the n received tags (uint8 [n, 16])
    -> fail (int32 [n], 1 where a tag did not verify; FLTEE_DEV_ERR_AUTH then in the status)."""
    ids = np.ascontiguousarray(client_ids, dtype=np.uint32)
    n = len(ids)
    assert len(iv) == 12 and tags.is_contiguous()
    fail = torch.full((max(n, 1),), 0x7fffffff, dtype=torch.int32, device=part.device)
    ivb = (ctypes.c_uint8 * 12)(*iv)
    _check(L.lib().fltee_gcm_finish_device(ids.ctypes.data_as(ctypes.c_void_p), n, _ptr(part), ct_bytes,
                                           ivb, aad_len, _ptr(tags), _ptr(fail), _stream(stream)),
           "fltee_gcm_finish_device")
    return fail[:n]


def decrypt_slice_auth(client_ids, window, row_stride, first_block, win_bytes, iv, records=None,
                       stream=None):
    """fltee_decrypt_slice_auth_device: the CTR half of GCM on one window of n slices ->
    int64 [n, win_bytes // 8] records (nothing is verified here)."""
    ids = np.ascontiguousarray(client_ids, dtype=np.uint32)
    n = len(ids)
    assert len(iv) == 12
    if records is None:
        records = torch.empty((n, win_bytes // 8), dtype=torch.int64, device=window.device)
    ivb = (ctypes.c_uint8 * 12)(*iv)
    _check(L.lib().fltee_decrypt_slice_auth_device(ids.ctypes.data_as(ctypes.c_void_p), n, _ptr(window),
                                                   row_stride, first_block, win_bytes, ivb,
                                                   _ptr(records), _stream(stream)),
           "fltee_decrypt_slice_auth_device")
    return records


def laplace_r(d, k, n, seed, device="cuda", stream=None):
    r = torch.empty(d, dtype=torch.int32, device=device)
    T = ctypes.c_float(0)
    _check(L.lib().fltee_laplace_r_device(d, k, n, seed, _ptr(r), ctypes.byref(T),
                                          _stream(stream)), "fltee_laplace_r_device")
    return r, T.value


def sum_rows(rows, coef=1.0, out=None, stream=None):
    """fltee_sum_rows_device: out = coef * (rows[0] + rows[1] + ...), added in row order."""
    assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2
    nrows, d = rows.shape
    rows = rows.contiguous()
    if out is None:
        out = torch.empty(d, dtype=torch.float32, device=rows.device)
    _check(L.lib().fltee_sum_rows_device(_ptr(rows), nrows, d, coef, _ptr(out), _stream(stream)),
           "fltee_sum_rows_device")
    return out


def dp_noise(out, sigma, clipping, n, seed=0, stream=None):
    """fltee_dp_noise_device: out += (N(0, clipping*sigma) / n) as f32 (common.rs:56-72)."""
    _check(L.lib().fltee_dp_noise_device(_ptr(out), out.numel(), sigma, clipping, n, seed,
                                         _stream(stream)), "fltee_dp_noise_device")
    return out


# ---- position-range pieces of `advanced` (multi-GPU Option B, fltee/parallel.py) ----
def advanced_init_range(records, nrec, d, pos_base, m, out=None, stream=None):
    """Entries pos_base..pos_base+m-1 of advanced's padded array (advanced.rs:116-142);
    records[x] is the record at position pos_base + x (read where < nrec)."""
    if out is None:
        out = torch.empty(m, dtype=torch.int64, device=records.device)
    _check(L.lib().fltee_advanced_init_range_device(_ptr(records), nrec, d, pos_base, m, _ptr(out),
                                                    _stream(stream)),
           "fltee_advanced_init_range_device")
    return out


def bitonic_range_sort(records, pos_base, mode=0, seed=0, stream=None, valid=None):
    """valid: entries valid.. of this range are identical pads (None: unknown)."""
    if valid is not None:
        _check(L.lib().fltee_bitonic_range_sort_padded_device(_ptr(records), records.numel(),
                                                              pos_base, valid, mode, seed,
                                                              _stream(stream)),
               "fltee_bitonic_range_sort_padded_device")
        return records
    _check(L.lib().fltee_bitonic_range_sort_device(_ptr(records), records.numel(), pos_base, mode,
                                                   seed, _stream(stream)),
           "fltee_bitonic_range_sort_device")
    return records


def bitonic_range_merge(records, pos_base, stage_log, mode=0, seed=0, stream=None):
    _check(L.lib().fltee_bitonic_range_merge_device(_ptr(records), records.numel(), pos_base, mode,
                                                    seed, stage_log, _stream(stream)),
           "fltee_bitonic_range_merge_device")
    return records


def bitonic_range_exchange(mine, theirs, pos_mine, pos_theirs, stage_log, mode=0, seed=0,
                           stream=None):
    assert theirs.numel() == mine.numel()
    _check(L.lib().fltee_bitonic_range_exchange_device(_ptr(mine), _ptr(theirs), mine.numel(),
                                                       pos_mine, pos_theirs, mode, seed, stage_log,
                                                       _stream(stream)),
           "fltee_bitonic_range_exchange_device")
    return mine


def bitonic_range_steps(records, pos_base, stage_log, step_top, step_bot, mode=0, seed=0,
                        stream=None):
    _check(L.lib().fltee_bitonic_range_steps_device(_ptr(records), records.numel(), pos_base, mode,
                                                    seed, stage_log, step_top, step_bot,
                                                    _stream(stream)),
           "fltee_bitonic_range_steps_device")
    return records


def fold_context(halo):
    return L.lib().fltee_fold_context(halo)


def fold_side_bytes(span, halo):
    return L.lib().fltee_fold_side_bytes(span, halo)


def fold_range(src, dst, origin, end, pos_base, fold_len, halo, side, stream=None):
    """fltee_fold_range_device: [0, origin) of src holds >= fold_context(halo) + 1 records
    of context; side: a byte buffer of >= fold_side_bytes(end - origin, halo)."""
    assert side.numel() * side.element_size() >= fold_side_bytes(end - origin, halo)
    _check(L.lib().fltee_fold_range_device(_ptr(src), _ptr(dst), src.numel(), origin, end, pos_base,
                                           fold_len, halo, _ptr(side), _stream(stream)),
           "fltee_fold_range_device")
    return dst


def fold_range_total(side, span, halo, total, stream=None):
    """the range's segmented total (16 bytes into `total`) for the ranges after it"""
    assert total.numel() * total.element_size() >= 16
    _check(L.lib().fltee_fold_range_total_device(_ptr(side), span, halo, _ptr(total), _stream(stream)),
           "fltee_fold_range_total_device")
    return total


def fold_range_patch(dst, origin, end, pos_base, fold_len, halo, side, prev_totals, stream=None):
    """the long-run patch of one range's fold output; prev_totals: the totals of the ranges
    before it, in order (a contiguous tensor of n * 16 bytes, or None)"""
    n_prev = 0 if prev_totals is None else prev_totals.numel() * prev_totals.element_size() // 16
    _check(L.lib().fltee_fold_range_patch_device(_ptr(dst), origin, end, pos_base, fold_len, halo,
                                                 _ptr(side), _ptr(prev_totals) if n_prev else None,
                                                 n_prev, _stream(stream)),
           "fltee_fold_range_patch_device")
    return dst


def compact_range(chunk, d, coef, buf, tmp, out=None, stream=None):
    if out is None:
        out = torch.empty(d, dtype=torch.float32, device=chunk.device)
    c = chunk.numel()
    assert buf.numel() >= d + c and tmp.numel() >= d + c
    _check(L.lib().fltee_compact_range_device(_ptr(chunk), c, d, _ptr(buf), _ptr(tmp), coef,
                                              _ptr(out), _stream(stream)),
           "fltee_compact_range_device")
    return out


# ---- position-range pieces of alg 7's stable network (fltee/parallel.py) ----
def _records16(t):
    """m of a tensor whose bytes are m 16-byte records (e.g. int64 [m, 2])"""
    nbytes = t.numel() * t.element_size()
    assert t.is_cuda and t.is_contiguous() and nbytes % 16 == 0
    return nbytes // 16


def stable_init_range(records, nrec, d, pos_base, m, out=None, stream=None):
    """Entries pos_base..pos_base+m-1 of alg 7's padded array as 16-byte records (int64
    [m, 2]: key = idx << 32 | global position; val bits); records[x] is the record at
    position pos_base + x (read where < nrec)."""
    if out is None:
        out = torch.empty((m, 2), dtype=torch.int64, device=records.device)
    _check(L.lib().fltee_stable_init_range_device(_ptr(records), nrec, d, pos_base, m, _ptr(out),
                                                  _stream(stream)),
           "fltee_stable_init_range_device")
    return out


def stable_range_sort(rec16, pos_base, valid=None, stream=None):
    """Stages 1..log2 m on one range; valid: entries valid.. of it are pads (None: none)."""
    m = _records16(rec16)
    _check(L.lib().fltee_stable_range_sort_device(_ptr(rec16), m, pos_base,
                                                  m if valid is None else valid, _stream(stream)),
           "fltee_stable_range_sort_device")
    return rec16


def stable_range_exchange(mine16, theirs16, pos_mine, pos_theirs, stage_log, stream=None):
    m = _records16(mine16)
    assert _records16(theirs16) == m
    _check(L.lib().fltee_stable_range_exchange_device(_ptr(mine16), _ptr(theirs16), m, pos_mine,
                                                      pos_theirs, stage_log, _stream(stream)),
           "fltee_stable_range_exchange_device")
    return mine16


def stable_range_merge(rec16, pos_base, stage_log, stream=None):
    _check(L.lib().fltee_stable_range_merge_device(_ptr(rec16), _records16(rec16), pos_base,
                                                   stage_log, _stream(stream)),
           "fltee_stable_range_merge_device")
    return rec16


def stable_range_strip(rec16, out=None, stream=None):
    """The range as the fold's 8-byte (idx, val) records (int64 [m])."""
    m = _records16(rec16)
    if out is None:
        out = torch.empty(m, dtype=torch.int64, device=rec16.device)
    _check(L.lib().fltee_stable_range_strip_device(_ptr(rec16), m, _ptr(out), _stream(stream)),
           "fltee_stable_range_strip_device")
    return out


def nips19_build_range(records, nrec, r, d, tf, pos_base, m, out=None, stream=None):
    """Entries pos_base..pos_base+m-1 of nips19's padded array (records ++ Laplace dummies
    ++ pads, common.rs:164-197); r = laplace_r(...)[0], tf = int(T)."""
    if out is None:
        out = torch.empty(m, dtype=torch.int64, device=records.device)
    _check(L.lib().fltee_nips19_build_range_device(_ptr(records), nrec, _ptr(r), d, tf, pos_base, m,
                                                   _ptr(out), _stream(stream)),
           "fltee_nips19_build_range_device")
    return out


def safe_aggregate(entries, d, out=None, stream=None):
    """common.rs:25-35 on a range of shuffled entries: un-averaged f32[d] partial sums."""
    if out is None:
        out = torch.empty(d, dtype=torch.float32, device=entries.device)
    _check(L.lib().fltee_safe_aggregate_device(_ptr(entries), entries.numel(), d, _ptr(out),
                                               _stream(stream)),
           "fltee_safe_aggregate_device")
    return out


def select(entries, d, stream=None):
    """The entries of one range with idx < d, in position order (fltee_select_device):
    the piece of nips19's safe_aggregate a range contributes, as an int64 tensor."""
    count = ctypes.c_size_t(0)
    lst = torch.empty(max(1, entries.numel()), dtype=torch.int64, device=entries.device)
    _check(L.lib().fltee_select_device(_ptr(entries), entries.numel(), d, _ptr(lst), lst.numel(),
                                       ctypes.byref(count), _stream(stream)),
           "fltee_select_device")
    return lst[: count.value]


def ordered_list(lst, d, coef, out=None, stream=None):
    """out[i] = coef * (+0 + v1 + v2 ...) over the list's entries with idx i, in list
    order (fltee_ordered_list_device)."""
    if out is None:
        out = torch.empty(d, dtype=torch.float32, device=lst.device)
    _check(L.lib().fltee_ordered_list_device(_ptr(lst), lst.numel(), d, coef, _ptr(out),
                                             _stream(stream)),
           "fltee_ordered_list_device")
    return out


def debug_sort_records(records, d, out=None, stream=None):
    """The ordered fold's stable sort alone (fltee_debug_sort_records_device): the records in
    order of min(idx, d), upload order within an index, as a new int64 tensor."""
    if out is None:
        out = torch.empty_like(records)
    _check(L.lib().fltee_debug_sort_records_device(_ptr(records), records.numel(), d, _ptr(out),
                                                   _stream(stream)),
           "fltee_debug_sort_records_device")
    return out
