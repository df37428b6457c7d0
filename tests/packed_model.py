"""Packed dense uploads in numpy (include/fltee_agg.h: FLTEE_OPT_PACKED), independent of the
library: a slice of d parameters is U = ceil(d / 2) units of 8 bytes — the d f32 values in
position order, then one f32 of padding (+0.0 from the client, ignored by the server) when d
is odd.

pack / unpack    values [n, d] <-> rows [n, 2 U];  records: rows -> (idx, val) of the n * d
                 records (j, v[j]) the same upload would have carried.
inorder_mean     the enclave's dense result: ((+0.0 + v_0) + v_1) + ... in f32, client by
                 client, times f32(1) / f32(n_avg) (common.rs:14-19)."""
import struct

import numpy as np

AAD_PACKED_BIT = 0x80000000


def units(d):
    return (d + 1) // 2


def row(d):
    return 2 * units(d)


def slice_bytes(d):
    return 8 * units(d)


def pack(values, pad=0.0):
    v = np.ascontiguousarray(values, np.float32)
    n, d = v.shape
    out = np.full((n, row(d)), pad, np.float32)
    out[:, :d] = v
    return out


def unpack(rows, d):
    r = np.ascontiguousarray(rows, np.float32)
    assert r.shape[1] == row(d)
    return r[:, :d].copy()


def records(rows, d):
    """(idx u32 [n * d], val f32 [n * d]) of the unpacked upload"""
    v = unpack(rows, d)
    return np.tile(np.arange(d, dtype=np.uint32), v.shape[0]), v.reshape(-1)


def inorder_sum(values):
    v = np.ascontiguousarray(values, np.float32)
    acc = np.zeros(v.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for c in range(v.shape[0]):
            acc = acc + v[c]
    return acc


def inorder_mean(values, n_avg=None):
    n = values.shape[0] if n_avg is None else n_avg
    with np.errstate(all="ignore"):
        return inorder_sum(values) * (np.float32(1) / np.float32(n))


def is_packed(on, d, k_req, ct_bytes):
    """the packed-call rule of ecall_secure_aggregation on one client's ciphertext bytes"""
    return bool(on) and d >= 2 and k_req in (0, d) and ct_bytes == slice_bytes(d)


def aad(fl_id, round_, client_id, alg, packed):
    return struct.pack(">IIII", fl_id, round_, client_id, alg | (AAD_PACKED_BIT if packed else 0))


def values(rng, n, d):
    """N(0, 1) with -0.0, denormals and +-large magnitudes sprinkled in"""
    v = rng.normal(0, 1, (n, d)).astype(np.float32)
    flat = v.reshape(-1)
    m = flat.size
    for special in (-0.0, 1e-41, -3e-39, 3e37, -3e37, 1e30, 0.0):
        flat[rng.integers(0, m, max(1, m // 97))] = np.float32(special)
    return v
