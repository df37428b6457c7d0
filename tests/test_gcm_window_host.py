"""GHASH by windows on the host (no GPU): fltee_debug_ghash_window_host is the host twin of the
windowed GHASH kernel (k_ghash.hip) that a multi-GPU eid's column shard runs.  A slice cut into
1, 2 and 4 windows where group_dense_ecall cuts it (records p_i = (d i / W) & ~3, blocks p_i / 2)
gives partial vectors whose XOR is the single window's, and that vector, put through
sum_s part_s G^(P - 1 - s), the length block and E_K(J0) with the plain-Python model's gf_mul,
is the model's tag.  Every refusal of the windowed entry points is host arithmetic."""
import ctypes

import pytest

import gcm_model as M

CID = 260
# (B, aad_len): two segments; five segments (the W = 4 cuts two blocks before three segment
# boundaries, the last block partial); three whole blocks without AAD; one partial block
SHAPES = [(8808, 16), (32792, 16), (48, 0), (8, 16)]
REV8 = bytes(int(f"{b:08b}"[::-1], 2) for b in range(256))


@pytest.fixture(scope="module")
def lib():
    from fltee import _lib as L
    return L.lib()


def _u8(b):
    return (ctypes.c_uint8 * max(len(b), 1))(*b)


def window_part(lib, cid, aad, with_aad, ct, first_block, win_bytes, aad_len=None):
    """(status, P partials as GCM blocks) of the window [16 first_block, + win_bytes) of ct"""
    aad_len = len(aad) if aad_len is None else aad_len
    P = lib.fltee_gcm_segments(len(ct), aad_len)
    out = (ctypes.c_uint8 * max(16 * P, 1))()
    lo = 16 * first_block
    st = lib.fltee_debug_ghash_window_host(cid, _u8(aad), aad_len, 1 if with_aad else 0,
                                           _u8(ct[lo:lo + win_bytes]), len(ct), first_block, win_bytes, out)
    # a partial is stored as the kernels hold it: every byte of the GCM block bit-reversed
    return st, bytes(out)[:16 * P].translate(REV8)


def cuts(d, W):
    p = [(d * i // W) & ~3 for i in range(W)] + [d]
    return [(p[i] // 2, (p[i + 1] - p[i]) * 8) for i in range(W)]


def xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def tag_from_parts(cid, iv, aad_len, ct_len, parts):
    rk = M.expand_key(M.session_key(cid))
    h = int.from_bytes(M.encrypt_block(rk, bytes(16)), "big")
    g = h
    for _ in range(9):  # G = H^512
        g = M.gf_mul(g, g)
    y = 0
    for s in range(len(parts) // 16):  # Horner: sum_s part_s G^(P - 1 - s)
        y = M.gf_mul(y, g) ^ int.from_bytes(parts[16 * s:16 * s + 16], "big")
    lens = (8 * aad_len << 64) | (8 * ct_len)
    ej0 = int.from_bytes(M.encrypt_block(rk, iv + b"\0\0\0\1"), "big")
    return (M.gf_mul(y ^ lens, h) ^ ej0).to_bytes(16, "big")


@pytest.mark.parametrize("B,aad_len", SHAPES)
def test_windows_xor_to_the_slice_and_the_slice_to_the_tag(lib, B, aad_len):
    assert M.S == 512
    ct = M.plaintext(B, B % 251)
    aad = M.aad_of(CID, aad_len)
    P = lib.fltee_gcm_segments(B, aad_len)
    assert P == -(-((B + 15) // 16 + (aad_len + 15) // 16) // M.S)
    st, whole = window_part(lib, CID, aad, True, ct, 0, B)
    assert st == 0 and len(whole) == 16 * P
    for W in (1, 2, 4):
        acc = bytes(16 * P)
        for i, (fb, wb) in enumerate(cuts(B // 8, W)):
            st, part = window_part(lib, CID, aad, i == 0, ct, fb, wb, aad_len)
            assert st == 0
            if wb == 0 and i:
                assert not any(part), "an empty window without the AAD contributes nothing"
            acc = xor(acc, part)
        assert acc == whole, f"W = {W}"
    assert tag_from_parts(CID, M.IV, aad_len, B, whole) == M.tag(M.session_key(CID), M.IV, aad, ct)


def test_the_w4_cuts_of_the_five_segment_shape_straddle_segments(lib):
    """what the shape is for: pad + AAD block + cut lands two blocks before a segment boundary"""
    B, aad_len = 32792, 16
    blocks = (B + 15) // 16 + 1
    P = lib.fltee_gcm_segments(B, aad_len)
    assert P == 5 and B % 16 == 8
    pad = P * M.S - blocks
    at = [(pad + 1 + fb) % M.S for fb, _ in cuts(B // 8, 4)[1:]]
    assert at == [M.S - 2] * 3


def test_aad_may_ride_on_any_one_window(lib):
    B, aad_len = 8808, 16
    ct, aad = M.plaintext(B, 3), M.aad_of(CID, aad_len)
    _, whole = window_part(lib, CID, aad, True, ct, 0, B)
    (f0, w0), (f1, w1) = cuts(B // 8, 2)
    _, a = window_part(lib, CID, aad, False, ct, f0, w0, aad_len)
    _, b = window_part(lib, CID, aad, True, ct, f1, w1, aad_len)
    assert xor(a, b) == whole


def _device_window(lib, ct_bytes, first_block, win_bytes, aad_len, row_stride):
    """the device entry point with pointers it must not get to read"""
    ids = (ctypes.c_uint32 * 1)(CID)
    return lib.fltee_ghash_window_device(ids, 1, None, row_stride, ct_bytes, first_block, win_bytes,
                                         _u8(bytes(64)), aad_len, 0, None, None)


REFUSED = [
    # ct_bytes, first_block, win_bytes, aad_len
    (8808, 0, 8808, 65),             # aad_len > 64
    ((1 << 36) - 31, 0, 16, 16),     # ct_bytes > 2^36 - 32
    (8808, 552, 0, 16),              # starts past the slice (551 blocks, the last one partial)
    (48, 4, 0, 0),                   # starts past a slice of whole blocks
    (8808, 548, 48, 16),             # reaches past ct_bytes
    (8808, 0, 8816, 16),
    (8808, 0, 4392, 16),             # ends off a 16-byte boundary inside the slice
    (8808, 1 << 60, 16, 16),         # 16 first_block overflows
]


@pytest.mark.parametrize("ct_bytes,first_block,win_bytes,aad_len", REFUSED)
def test_refusals_are_host_arithmetic(lib, ct_bytes, first_block, win_bytes, aad_len):
    out = (ctypes.c_uint8 * 64)()
    st = lib.fltee_debug_ghash_window_host(CID, _u8(bytes(64)), aad_len, 1, _u8(bytes(16)), ct_bytes,
                                           first_block, win_bytes, out)
    assert st == 2
    assert _device_window(lib, ct_bytes, first_block, win_bytes, aad_len, max(win_bytes, 16)) == 2


def test_more_refusals_of_the_device_pieces(lib):
    ids = (ctypes.c_uint32 * 1)(CID)
    iv = (ctypes.c_uint8 * 12)()
    # a row shorter than its window
    assert _device_window(lib, 8808, 0, 4400, 16, 4392) == 2
    assert lib.fltee_decrypt_slice_auth_device(ids, 1, None, 4392, 0, 4400, iv, None, None) == 2
    # the slice's counters would pass 32 bits
    assert lib.fltee_decrypt_slice_auth_device(ids, 1, None, 1 << 40, (1 << 32) - 2, 32, iv, None, None) == 2
    # the finish: the whole-slice bounds
    assert lib.fltee_gcm_finish_device(ids, 1, None, 8808, iv, 65, None, None, None) == 2
    assert lib.fltee_gcm_finish_device(ids, 1, None, (1 << 36) - 31, iv, 16, None, None, None) == 2
    # accepted windows at the edges: the partial last block alone, an empty window at the end
    out = (ctypes.c_uint8 * 64)()
    for fb, wb in ((550, 8), (550, 0), (0, 0)):
        assert lib.fltee_debug_ghash_window_host(CID, _u8(bytes(16)), 16, 0, _u8(bytes(16)), 8808, fb, wb,
                                                 out) == 0
