"""bf16 dense uploads in numpy (include/fltee_agg.h: FLTEE_OPT_BF16), independent of the
library: a slice of d parameters is Q = ceil(d / 4) units of 8 bytes — the d bf16 values in
position order, then 4 Q - d bf16 of padding (+0.0 from the client, ignored by the server).

narrow / widen   f32 <-> bf16 bits (uint16).  widen is exact: bits << 16.  narrow is round to
                 nearest even in integer ops; a NaN keeps its sign and is quieted.
pack / unpack    values [n, d] (f32) -> rows [n, 4 Q] (uint16);  rows -> the widened f32 [n, d];
                 records: rows -> (idx, val) of the n * d records (j, widen(h[j])).
inorder_mean     packed_model's: the enclave's dense result on the widened values."""
import struct

import numpy as np

import packed_model as PM

AAD_BF16_BIT = 0x40000000


def units(d):
    return (d + 3) // 4


def row(d):
    return 4 * units(d)


def slice_bytes(d):
    return 8 * units(d)


def narrow(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    rne = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x0040, rne).astype(np.uint16)


def widen(h):
    return (np.ascontiguousarray(h, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def pack(values, pad=0):
    """pad: the bf16 bit pattern of the padding (0x7FC0: a NaN)"""
    h = narrow(values)
    n, d = h.shape
    out = np.full((n, row(d)), pad, np.uint16)
    out[:, :d] = h
    return out


def unpack(rows, d):
    r = np.ascontiguousarray(rows, np.uint16)
    assert r.shape[1] == row(d)
    return widen(r[:, :d])


def records(rows, d):
    """(idx u32 [n * d], val f32 [n * d]) of the unpacked upload"""
    v = unpack(rows, d)
    return np.tile(np.arange(d, dtype=np.uint32), v.shape[0]), v.reshape(-1)


def inorder_mean(rows, d, n_avg=None):
    return PM.inorder_mean(unpack(rows, d), n_avg)


def is_bf16(on, d, k_req, ct_bytes):
    """the bf16-call rule of ecall_secure_aggregation on one client's ciphertext bytes"""
    return bool(on) and d >= 3 and k_req in (0, d) and ct_bytes == slice_bytes(d)


def aad(fl_id, round_, client_id, alg, bf16):
    return struct.pack(">IIII", fl_id, round_, client_id, alg | (AAD_BF16_BIT if bf16 else 0))


# f32 bit patterns every narrow has to get right: exact ties (mantissa low half = 0x8000) with
# an even and an odd upper bit, just above and below a tie, the largest finite values (round up
# to inf), denormals, NaNs of both signs (quiet, signalling, payload only in the low half)
SPECIAL_BITS = np.array([
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000,
    0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00000000, 0x80000000,
    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FA00000, 0xFFFFFFFF, 0x7F80FFFF, 0xFF808000,
], np.uint32)


def same_bits(a, b):
    """bit for bit, except that a NaN only has to meet a NaN: which NaN an add returns (inf - inf,
    or a NaN operand's payload) is the adder's choice, not the format's"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def values(rng, n, d, nans=False):
    """N(0, 1) with -0.0, denormals, +-3e37, values that round up to inf and exact ties
    sprinkled in (nans: NaNs of both signs too).  f32: narrow() is the client's step."""
    v = PM.values(rng, n, d).copy()
    flat = v.reshape(-1).view(np.uint32)
    m = flat.size
    pool = SPECIAL_BITS if nans else SPECIAL_BITS[(SPECIAL_BITS & 0x7FFFFFFF) <= 0x7F800000]
    for b in pool:
        flat[rng.integers(0, m, max(1, m // 1009))] = b
    return v
