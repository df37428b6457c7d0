"""AES-128-GCM on the GPU (k_ghash.hip + k_aes.hip's IV planes) against OpenSSL's known
answers (tests/golden/gcm_kat.npz): the producer fltee_encrypt_auth_device byte for byte,
fltee_decrypt_auth_device back to the plaintext with every tag verified, one-bit tampers
failing exactly the clients they touch, and the plain CTR path left as it was.  The lengths
cross every boundary of the layout: empty, a partial block, one block, the segment size
S = 512 blocks on either side, two and three segments with a ragged tail, and n = 5 on each
side of the CTR kernels' switch."""
import hashlib
import os

import numpy as np
import pytest

import gcm_model as M
from conftest import GOLDEN, gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

IDS_FOR = {1: (0,), 3: (1, 258, 65535), 5: M.IDS}
DEV_ERR_AUTH = 0x10


@pytest.fixture(scope="module")
def kat():
    z = np.load(os.path.join(GOLDEN, "gcm_kat.npz"))
    return z, {k: i for i, k in enumerate(z["keys"].tolist())}


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


def produce(ids, length, aad_len, iv=M.IV):
    """(plaintext [n, length] u8 on the GPU, slices [n, length + 16] from the producer, aad)"""
    import torch

    from fltee import client as C
    pt = np.stack([np.frombuffer(M.plaintext(length, c), np.uint8) for c in ids]) if length else \
        np.zeros((len(ids), 0), np.uint8)
    aad = b"".join(M.aad_of(c, aad_len) for c in ids)
    d_pt = torch.from_numpy(pt.copy()).cuda()
    return d_pt, C.encrypt_parameters_gcm(d_pt, ids, iv, aad), aad


def check_against_fixture(kat, ids, length, aad_len, slices):
    z, idx = kat
    host = slices.cpu().numpy()
    for j, c in enumerate(ids):
        i = idx[M.case_key(c, length, aad_len)]
        ct, tag = host[j, :length].tobytes(), host[j, length:].tobytes()
        want = ct if length <= 64 else hashlib.sha256(ct).digest()
        assert want == bytes(z["cts"][i][:len(want)]), f"ciphertext of client {c}, {length} bytes"
        assert tag == bytes(z["tags"][i]), f"tag of client {c}, {length} bytes, aad {aad_len}"


def round_trip(dev, kat, n, length, aad_len):
    ids = IDS_FOR[n]
    d_pt, slices, aad = produce(ids, length, aad_len)
    check_against_fixture(kat, ids, length, aad_len, slices)
    rec, fail = dev.decrypt_auth(ids, slices, length, M.IV, aad)
    assert dev.status() == 0
    assert not fail.cpu().numpy().any()
    if length >= 8:
        import torch
        got = rec.view(torch.uint8).cpu().numpy().reshape(n, -1)
        assert np.array_equal(got, d_pt.cpu().numpy()[:, :length // 8 * 8])


@pytest.mark.parametrize("length", M.SMALL_LENS + M.SEGMENT_LENS)
@pytest.mark.parametrize("n,aad_len", [(1, 0), (3, 20), (5, 16)])
def test_round_trip_and_kat(dev, kat, n, aad_len, length):
    round_trip(dev, kat, n, length, aad_len)


@pytest.mark.parametrize("length", M.SWITCH_LENS)
def test_round_trip_on_each_side_of_the_ctr_kernel_switch(dev, kat, length):
    round_trip(dev, kat, 5, length, 16)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("length", [40, 16 * M.S + 8])
def test_round_trip_on_either_ctr_kernel(dev, kat, variant, length):
    from fltee import _lib as L
    L.lib().fltee_debug_set_aes_variant(variant)
    try:
        round_trip(dev, kat, 3, length, 20)
    finally:
        L.lib().fltee_debug_set_aes_variant(0)


def test_empty_aad_pointer_and_zero_iv_vectors(dev):
    """SP 800-38D test cases 1 and 2 on the device (client 0: the all-zero key)."""
    import torch
    z = torch.zeros(16, dtype=torch.uint8, device="cuda")
    from fltee import client as C
    out = C.encrypt_parameters_gcm(z, (0,), bytes(12)).cpu().numpy().tobytes()
    assert out.hex() == "0388dace60b6a392f328c2b971b2fe78" "ab6e47d42cec13bdf53a67b21257bddf"
    out = C.encrypt_parameters_gcm(z[:0], (0,), bytes(12)).cpu().numpy().tobytes()
    assert out.hex() == "58e2fccefa7e3061367f1d57a4e7455a"


def test_plain_ctr_is_untouched(dev, oracle):
    """fltee_decrypt_device gives the bytes of the oracle's CTR, and its launch trace after the
    authenticated path has run (and the ECALL switch been flipped) is the one from before."""
    import torch

    from fltee.ecalls import set_upload_aead
    from test_gpu_oblivious import traced
    ids = np.array(IDS_FOR[3], np.uint32)
    length = 16 * M.S + 8
    pt = [M.plaintext(length, int(c)) for c in ids]
    enc = torch.from_numpy(np.frombuffer(oracle.encrypt_clients(ids, pt), np.uint8).copy()).cuda()
    rec = torch.empty(3 * length // 8, dtype=torch.int64, device="cuda")

    def run():
        dev.decrypt(ids, enc, length, rec)
        return rec.view(torch.uint8).cpu().numpy().tobytes()

    assert run() == b"".join(pt)
    before = traced(run)
    _, slices, aad = produce(IDS_FOR[3], length, 16)
    assert not dev.decrypt_auth(IDS_FOR[3], slices, length, M.IV, aad)[1].cpu().numpy().any()
    set_upload_aead(True)
    set_upload_aead(False)
    after = traced(run)
    assert before and before == after
    assert not any("ghash" in line or "true, true" in line or "false, true" in line for line in after)
    assert run() == b"".join(pt)


TAMPER_LEN = 16 * (2 * M.S + 1) + 8  # three segments, a partial last block
TAMPERS = [
    ("ciphertext first byte", lambda s, aad, iv: s[1].__setitem__(0, s[1, 0] ^ 1), (0, 1, 0)),
    ("last byte of the partial block", lambda s, aad, iv: s[2].__setitem__(TAMPER_LEN - 1, s[2, TAMPER_LEN - 1] ^ 0x80), (0, 0, 1)),
    ("a byte in the second segment", lambda s, aad, iv: s[0].__setitem__(16 * M.S + 5, s[0, 16 * M.S + 5] ^ 4), (1, 0, 0)),
    ("tag byte 0", lambda s, aad, iv: s[1].__setitem__(TAMPER_LEN, s[1, TAMPER_LEN] ^ 1), (0, 1, 0)),
    ("tag byte 15", lambda s, aad, iv: s[1].__setitem__(TAMPER_LEN + 15, s[1, TAMPER_LEN + 15] ^ 0x80), (0, 1, 0)),
    ("one AAD byte", lambda s, aad, iv: aad.__setitem__(2 * 16 + 9, aad[2 * 16 + 9] ^ 1), (0, 0, 1)),
    ("the IV's round word", lambda s, aad, iv: iv.__setitem__(7, iv[7] ^ 1), (1, 1, 1)),
    ("two clients' slices swapped", lambda s, aad, iv: s.__setitem__([0, 1], s[[1, 0]]), (1, 1, 0)),
]


@pytest.fixture(scope="module")
def tamper_base(dev):
    """the untampered slices (host copy) and AAD, built once and never modified"""
    ids = IDS_FOR[3]
    d_pt, slices, aad = produce(ids, TAMPER_LEN, 16)
    return ids, d_pt.cpu().numpy(), slices.cpu().numpy(), aad


@pytest.mark.parametrize("what,change,expect", TAMPERS, ids=[t[0] for t in TAMPERS])
def test_tamper_fails_exactly_the_clients_it_touches(dev, tamper_base, what, change, expect):
    import torch
    ids, pt, slices, aad = tamper_base
    s, a, iv = slices.copy(), bytearray(aad), bytearray(M.IV)
    change(s, a, iv)
    rec, fail = dev.decrypt_auth(ids, torch.from_numpy(s).cuda(), TAMPER_LEN, bytes(iv), bytes(a))
    assert tuple(fail.cpu().numpy().tolist()) == expect, what
    assert dev.status() == DEV_ERR_AUTH
    assert dev.status() == 0
    # and the untampered slices still verify
    rec, fail = dev.decrypt_auth(ids, torch.from_numpy(slices.copy()).cuda(), TAMPER_LEN, M.IV, aad)
    assert not fail.cpu().numpy().any() and dev.status() == 0
    assert np.array_equal(rec.view(torch.uint8).cpu().numpy().reshape(3, -1), pt)
