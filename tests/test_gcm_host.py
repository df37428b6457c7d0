"""AES-128-GCM on the host (no GPU): fltee_debug_gcm_tag_host runs the one GF(2^128)
multiply of the library (csrc/ghash.h, the function the kernels of k_ghash.hip run) and must
agree with OpenSSL's known answers (tests/golden/gcm_kat.npz) and with the plain-Python model
(tests/gcm_model.py).  Also: identities of the multiply, the AES-NI and the portable subkeys,
the host-arithmetic refusals, and the constants the Python layer mirrors."""
import ctypes
import os

import numpy as np
import pytest

import gcm_model as M
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def lib():
    from fltee import _lib as L
    return L.lib()


@pytest.fixture(scope="module")
def kat():
    z = np.load(os.path.join(GOLDEN, "gcm_kat.npz"))
    idx = {k: i for i, k in enumerate(z["keys"].tolist())}
    return z, idx


def host_tag(lib, cid, iv, aad, ct):
    tag = (ctypes.c_uint8 * 16)()
    st = lib.fltee_debug_gcm_tag_host(cid, (ctypes.c_uint8 * 12)(*iv),
                                      (ctypes.c_uint8 * max(len(aad), 1))(*aad), len(aad),
                                      (ctypes.c_uint8 * max(len(ct), 1))(*ct), len(ct), tag)
    return st, bytes(tag)


def test_segment_constant_is_the_kernels(lib):
    from fltee import _lib as L
    assert lib.fltee_debug_gcm_segment_blocks() == L.GCM_SEGMENT_BLOCKS == M.S
    hdr = open(os.path.join(ROOT, "include", "fltee_agg.h")).read()
    assert f"#define FLTEE_GCM_SEGMENT_BLOCKS {M.S}\n" in hdr
    assert "#define FLTEE_ERROR_MAC_MISMATCH 0x3001u" in hdr and "#define FLTEE_DEV_ERR_AUTH 0x10u" in hdr
    assert (L.ERROR_MAC_MISMATCH, L.DEV_ERR_AUTH) == (0x3001, 0x10)


def test_sp800_38d_cases_1_and_2(lib, kat):
    z, _ = kat
    assert host_tag(lib, 0, bytes(12), b"", b"") == (0, bytes.fromhex("58e2fccefa7e3061367f1d57a4e7455a"))
    assert bytes(z["kat1_tag"]) == bytes.fromhex("58e2fccefa7e3061367f1d57a4e7455a")
    ct = bytes.fromhex("0388dace60b6a392f328c2b971b2fe78")
    assert bytes(z["kat2_ct"]) == ct
    assert host_tag(lib, 0, bytes(12), b"", ct) == (0, bytes.fromhex("ab6e47d42cec13bdf53a67b21257bddf"))
    assert M.encrypt(bytes(16), bytes(12), b"", bytes(16)) == (ct, bytes(z["kat2_tag"]))


@pytest.mark.parametrize("cid", [0, 1, 258, 65535])
def test_host_tag_equals_fixture_and_model(lib, kat, cid):
    z, idx = kat
    key = M.session_key(cid)
    for length in M.SMALL_LENS:
        ct_model = None
        for al in M.AAD_LENS:
            aad = M.aad_of(cid, al)
            if ct_model is None:
                ct_model = M.encrypt(key, M.IV, aad, M.plaintext(length, cid))[0]
            i = idx[M.case_key(cid, length, al)]
            if length <= 64:
                assert bytes(z["cts"][i][:length]) == ct_model
            want = bytes(z["tags"][i])
            assert M.tag(key, M.IV, aad, ct_model) == want, (cid, length, al)
            assert host_tag(lib, cid, M.IV, aad, ct_model) == (0, want), (cid, length, al)


def gf(lib, a, b):
    out = (ctypes.c_uint8 * 16)()
    lib.fltee_debug_gf128_mul((ctypes.c_uint8 * 16)(*a), (ctypes.c_uint8 * 16)(*b), out)
    return bytes(out)


def test_multiply_identities_and_model(lib):
    rng = np.random.default_rng(38)
    one = bytes([0x80]) + bytes(15)  # GCM's reflected bit order: x^0 is the MSB of byte 0
    xor = lambda p, q: bytes(a ^ b for a, b in zip(p, q))  # noqa: E731
    edge = [bytes(16), one, bytes(15) + b"\x01", b"\xff" * 16, bytes([0xE1]) + bytes(15)]
    elems = edge + [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(40)]
    for i, x in enumerate(elems):
        y, w = elems[(i * 7 + 3) % len(elems)], elems[(i * 11 + 5) % len(elems)]
        assert gf(lib, x, one) == x and gf(lib, one, x) == x
        assert gf(lib, x, bytes(16)) == bytes(16)
        assert gf(lib, x, y) == gf(lib, y, x)
        assert gf(lib, x, xor(y, w)) == xor(gf(lib, x, y), gf(lib, x, w))
        assert gf(lib, x, y) == M.gf_mul(int.from_bytes(x, "big"), int.from_bytes(y, "big")).to_bytes(16, "big")
        assert gf(lib, gf(lib, x, y), w) == gf(lib, x, gf(lib, y, w))


def test_subkeys_aesni_equals_portable_and_model(lib):
    for cid in (0, 1, 258, 65535, 0xFFFFFFFF):
        a, b = (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 32)()
        iv = (ctypes.c_uint8 * 12)(*M.IV)
        lib.fltee_debug_gcm_subkeys(cid, iv, a, 0)
        lib.fltee_debug_gcm_subkeys(cid, iv, b, 1)
        rk = M.expand_key(M.session_key(cid))
        want = M.encrypt_block(rk, bytes(16)) + M.encrypt_block(rk, M.IV + b"\0\0\0\1")
        assert bytes(a) == bytes(b) == want


def test_host_arithmetic_refusals(lib):
    iv = (ctypes.c_uint8 * 12)()
    tag = (ctypes.c_uint8 * 16)()
    buf = (ctypes.c_uint8 * 80)()
    assert lib.fltee_debug_gcm_tag_host(1, iv, buf, 64, buf, 16, tag) == 0
    assert lib.fltee_debug_gcm_tag_host(1, iv, buf, 65, buf, 16, tag) == 2
    # the 32-bit counter bound, refused before anything is read
    assert lib.fltee_debug_gcm_tag_host(1, iv, buf, 0, buf, (1 << 36) - 31, tag) == 2
    ids = (ctypes.c_uint32 * 1)(1)
    fail = (ctypes.c_uint32 * 1)(7)
    for fn, extra in ((lib.fltee_decrypt_auth_device, (fail, None)), (lib.fltee_encrypt_auth_device, (None,))):
        assert fn(ids, 1, buf, 16, iv, buf, 65, buf, *extra) == 2
        assert fn(ids, 1, buf, (1 << 36) - 24, iv, buf, 16, buf, *extra) == 2
    assert lib.fltee_encrypt_auth_device(ids, 1, buf, 12, iv, buf, 16, buf, None) == 2  # whole records
    assert fail[0] == 7
