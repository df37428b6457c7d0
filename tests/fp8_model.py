"""fp8 dense uploads in numpy (include/fltee_agg.h: FLTEE_OPT_FP8), independent of the library:
with P = ceil(d / 8) a slice of d parameters is P + 1 units of 8 bytes — the d OCP e4m3fn codes
in position order, 0x00 padding up to 8 P, then the trailer: the client's scale s as a
little-endian f32 and 4 ignored bytes.

TABLE            the 256 codes' exact f32 values, built from the bit fields (1 sign, 4 exponent
                 bits with bias 7, 3 mantissa bits; no infinities; S.1111.111 is NaN and widens
                 to sign << 31 | 0x7FC00000).
dequant          x = TABLE[q] * s in f32 (round to nearest even): the value the server sums.
quantise         values [n, d] -> (codes, s): per row a = the largest finite |v|, s = a / 448
                 (f32) when that is a normal nonzero f32, else 1; y = v / s (f32); NaN ->
                 sign | 0x7F, |y| > 448 -> sign | 0x7E, else the nearest of the 127 finite
                 magnitudes (searchsorted over the midpoints, a tie to the even code).
pack / unpack    (codes, s) -> rows [n, 8 (P + 1)] uint8;  rows -> the f32 values x [n, d];
                 records: rows -> (idx, val) of the n * d records (j, x_j).
inorder_mean     packed_model's: the enclave's dense result on the x values."""
import struct

import numpy as np

import packed_model as PM

AAD_FP8_BIT = 0x20000000
MIN_D = 13


def units(d):
    return (d + 7) // 8 + 1


def row(d):
    return 8 * units(d)


def slice_bytes(d):
    return 8 * units(d)


def _table():
    bits = np.zeros(256, np.uint32)
    for q in range(256):
        sign, e, m = q >> 7, (q >> 3) & 15, q & 7
        if e == 15 and m == 7:
            b = 0x7FC00000
        elif e == 0:
            b = int(np.float32(m * 2.0 ** -9).view(np.uint32))  # subnormal: m * 2^-9, exact
        else:
            b = int(np.float32((1 + m / 8) * 2.0 ** (e - 7)).view(np.uint32))
        bits[q] = b | (sign << 31)
    return bits.view(np.float32)


TABLE = _table()
MAGS = TABLE[:0x7F].astype(np.float64)  # the 127 finite magnitudes, ascending: MAGS[q] is code q
MIDS = (MAGS[:-1] + MAGS[1:]) / 2       # exact in f64
MAX = np.float32(448.0)


def widen(codes):
    return TABLE[np.ascontiguousarray(codes, np.uint8)]


def dequant(codes, s):
    """codes [n, d] (or [d]), s [n] (or a scalar): x = w(q) * s, one f32 rounding"""
    w = widen(codes)
    s = np.asarray(s, np.float32)
    with np.errstate(all="ignore"):
        return (w * (s[:, None] if w.ndim == 2 and s.ndim == 1 else s)).astype(np.float32)


def narrow(y):
    """f32 y (already divided by the scale) -> codes"""
    y = np.ascontiguousarray(y, np.float32)
    sign = (y.view(np.uint32) >> 31).astype(np.uint8) << 7
    nan = np.isnan(y)
    a = np.abs(np.where(nan, np.float32(0), y)).astype(np.float64)
    lo = np.searchsorted(MIDS, a, side="left")      # MIDS[lo - 1] < a <= MIDS[lo]
    tie = (lo < len(MIDS)) & (a == MIDS[np.minimum(lo, len(MIDS) - 1)])
    q = np.where(tie & (lo % 2 == 1), lo + 1, lo)   # a tie between lo and lo + 1: the even code
    q = np.where(a > 448.0, 0x7E, q)
    q = np.where(nan, 0x7F, q)
    return (q.astype(np.uint8) | sign).astype(np.uint8)


def scales(values):
    v = np.ascontiguousarray(values, np.float32)
    a = np.where(np.isfinite(v), np.abs(v), np.float32(0)).max(axis=1).astype(np.float32)
    with np.errstate(all="ignore"):
        s = (a / MAX).astype(np.float32)
    normal = s.view(np.uint32) >= 0x00800000  # (a is finite and >= 0: so is s)
    return np.where(normal, s, np.float32(1.0)).astype(np.float32)


def quantise(values):
    """values [n, d] f32 -> (codes uint8 [n, d], s f32 [n])"""
    v = np.ascontiguousarray(values, np.float32)
    s = scales(v)
    with np.errstate(all="ignore"):
        y = (v / s[:, None]).astype(np.float32)
    return narrow(y), s


def pack_codes(codes, s, pad=0x00, tail=0x00):
    """pad: the padding byte; tail: the byte of the trailer's 4 ignored bytes"""
    codes = np.ascontiguousarray(codes, np.uint8)
    n, d = codes.shape
    out = np.full((n, row(d)), pad, np.uint8)
    out[:, :d] = codes
    out[:, row(d) - 8:row(d) - 4] = np.ascontiguousarray(s, np.float32).astype("<f4").view(np.uint8).reshape(n, 4)
    out[:, row(d) - 4:] = tail
    return out


def pack(values, pad=0x00, tail=0x00):
    return pack_codes(*quantise(values), pad=pad, tail=tail)


def split(rows, d):
    """rows -> (codes [n, d], s [n])"""
    r = np.ascontiguousarray(rows, np.uint8)
    assert r.shape[1] == row(d)
    return r[:, :d], np.ascontiguousarray(r[:, row(d) - 8:row(d) - 4]).view("<f4").reshape(-1).astype(np.float32)


def unpack(rows, d):
    return dequant(*split(rows, d))


def records(rows, d):
    """(idx u32 [n * d], val f32 [n * d]) of the unpacked upload"""
    v = unpack(rows, d)
    return np.tile(np.arange(d, dtype=np.uint32), v.shape[0]), v.reshape(-1)


def inorder_mean(rows, d, n_avg=None):
    return PM.inorder_mean(unpack(rows, d), n_avg)


def is_fp8(on, d, k_req, ct_bytes):
    """the fp8-call rule of ecall_secure_aggregation on one client's ciphertext bytes"""
    return bool(on) and d >= MIN_D and k_req in (0, d) and ct_bytes == slice_bytes(d)


def aad(fl_id, round_, client_id, alg, fp8):
    return struct.pack(">IIII", fl_id, round_, client_id, alg | (AAD_FP8_BIT if fp8 else 0))


def same_bits(a, b):
    """bit for bit, except that a NaN only has to meet a NaN: which NaN an add returns (inf - inf,
    or a NaN operand's payload) is the adder's choice, not the format's"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def random_rows(rng, n, d, nans=False):
    """n slices of uniformly random codes (every finite code; nans: the NaN codes too) under
    random positive scales around 1e-3 — what a compressing client sends"""
    codes = rng.integers(0, 256, (n, d), dtype=np.uint16).astype(np.uint8)
    if not nans:
        codes[(codes & 0x7F) == 0x7F] = 0x3A
    s = np.exp(rng.normal(np.log(1e-3), 1.0, n)).astype(np.float32)
    return pack_codes(codes, s)
