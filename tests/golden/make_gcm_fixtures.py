"""Writes tests/golden/gcm_kat.npz: AES-128-GCM known answers from OpenSSL's EVP_aes_128_gcm
(ctypes on libcrypto.so.3) for the inputs of tests/gcm_model.py.  Per case (client id,
ciphertext length, AAD length; the IV of gcm_model.IV): the tag, and the ciphertext itself up
to 64 bytes or its SHA-256 beyond, so the file stays a few KB.  Run from the repository root:
    python tests/golden/make_gcm_fixtures.py
The generator first reproduces SP 800-38D test cases 1 and 2 (client 0 has the all-zero key)
and writes nothing unless both match."""
import ctypes
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gcm_model as M  # noqa: E402

C = ctypes.CDLL("libcrypto.so.3")
C.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
C.EVP_aes_128_gcm.restype = ctypes.c_void_p
C.EVP_EncryptInit_ex.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_char_p, ctypes.c_char_p]
C.EVP_EncryptUpdate.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int),
                                ctypes.c_char_p, ctypes.c_int]
C.EVP_EncryptFinal_ex.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
C.EVP_CIPHER_CTX_ctrl.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
C.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
EVP_CTRL_GCM_SET_IVLEN, EVP_CTRL_GCM_GET_TAG = 0x9, 0x10


def openssl_gcm(key, iv, aad, pt):
    ctx = C.EVP_CIPHER_CTX_new()
    n = ctypes.c_int(0)
    try:
        assert C.EVP_EncryptInit_ex(ctx, C.EVP_aes_128_gcm(), None, None, None) == 1
        assert C.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_SET_IVLEN, len(iv), None) == 1
        assert C.EVP_EncryptInit_ex(ctx, None, None, key, iv) == 1
        if aad:
            assert C.EVP_EncryptUpdate(ctx, None, ctypes.byref(n), aad, len(aad)) == 1
        out = ctypes.create_string_buffer(len(pt) + 16)
        if pt:
            assert C.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), pt, len(pt)) == 1
        assert n.value == len(pt) or not pt
        assert C.EVP_EncryptFinal_ex(ctx, None, ctypes.byref(n)) == 1
        tag = ctypes.create_string_buffer(16)
        assert C.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_GET_TAG, 16, tag) == 1
        return out.raw[:len(pt)], tag.raw
    finally:
        C.EVP_CIPHER_CTX_free(ctx)


def main():
    z = M.session_key(0)
    assert z == bytes(16)
    ct, tag = openssl_gcm(z, bytes(12), b"", b"")
    assert ct == b"" and tag.hex() == "58e2fccefa7e3061367f1d57a4e7455a"
    ct, tag = openssl_gcm(z, bytes(12), b"", bytes(16))
    assert ct.hex() == "0388dace60b6a392f328c2b971b2fe78" and tag.hex() == "ab6e47d42cec13bdf53a67b21257bddf"
    out = {"kat1_tag": np.frombuffer(bytes.fromhex("58e2fccefa7e3061367f1d57a4e7455a"), np.uint8),
           "kat2_ct": np.frombuffer(ct, np.uint8), "kat2_tag": np.frombuffer(tag, np.uint8)}
    keys, tags, cts = [], [], []
    for cid in M.IDS:
        for lens, aads in ((M.SMALL_LENS + M.SEGMENT_LENS, M.AAD_LENS), (M.SWITCH_LENS, (16,))):
            for length in lens:
                pt = M.plaintext(length, cid)
                for al in aads:
                    ct, tag = openssl_gcm(M.session_key(cid), M.IV, M.aad_of(cid, al), pt)
                    keys.append(M.case_key(cid, length, al))
                    tags.append(np.frombuffer(tag, np.uint8))
                    body = ct if length <= 64 else hashlib.sha256(ct).digest()
                    cts.append(np.frombuffer(body.ljust(64, b"\0"), np.uint8))
    out["keys"] = np.array(keys)
    out["tags"] = np.stack(tags)
    out["cts"] = np.stack(cts)  # the ciphertext (length <= 64) or its SHA-256, zero padded
    path = os.path.join(HERE, "gcm_kat.npz")
    np.savez_compressed(path, **out)
    print(path, len(keys), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
