"""A plain-Python AES-128-GCM (NIST SP 800-38D), independent of OpenSSL and of the library:
AES from FIPS-197 with an S-box computed from its definition, GHASH as the bit-serial
multiply of SP 800-38D algorithm 1 on Python integers.  Slow and obvious on purpose."""
import struct


def _xtime(a):
    a <<= 1
    return (a ^ 0x11B) & 0xFF if a & 0x100 else a


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a, b = _xtime(a), b >> 1
    return r


def _make_sbox():
    inv = [0] * 256
    for a in range(1, 256):
        for b in range(1, 256):
            if _gmul(a, b) == 1:
                inv[a] = b
                break
    sbox = []
    for a in range(256):
        x = inv[a]
        y = x
        for s in range(1, 5):
            y ^= ((x << s) | (x >> (8 - s))) & 0xFF
        sbox.append(y ^ 0x63)
    return sbox


SBOX = _make_sbox()


def expand_key(key):
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rc = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rc
            rc = _xtime(rc)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(11)]


def encrypt_block(rk, block):
    s = [a ^ b for a, b in zip(block, rk[0])]
    for r in range(1, 11):
        s = [SBOX[b] for b in s]
        s = [s[(4 * c + r_ + 4 * r_) % 16] for c in range(4) for r_ in range(4)]  # ShiftRows
        if r < 10:
            t = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                for i in range(4):
                    t.append(_gmul(a[i], 2) ^ _gmul(a[(i + 1) % 4], 3) ^ a[(i + 2) % 4] ^ a[(i + 3) % 4])
            s = t
        s = [a ^ b for a, b in zip(s, rk[r])]
    return bytes(s)


def session_key(client_id):
    """session_key_store.rs:17-32: 16 zero bytes with bytes[4..8] = client_id big-endian"""
    return bytes(4) + struct.pack(">I", client_id) + bytes(8)


R = 0xE1 << 120


def gf_mul(x, y):
    """SP 800-38D algorithm 1 on blocks as big-endian integers (bit 0 = the MSB)"""
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ R if v & 1 else v >> 1
    return z


def ghash(h, aad, ct):
    y = 0
    for data in (aad, ct):
        for o in range(0, len(data), 16):
            blk = data[o:o + 16].ljust(16, b"\0")
            y = gf_mul(y ^ int.from_bytes(blk, "big"), h)
    lens = struct.pack(">QQ", 8 * len(aad), 8 * len(ct))
    return gf_mul(y ^ int.from_bytes(lens, "big"), h)


def tag(key, iv, aad, ct):
    rk = expand_key(key)
    h = int.from_bytes(encrypt_block(rk, bytes(16)), "big")
    ej0 = int.from_bytes(encrypt_block(rk, iv + b"\0\0\0\1"), "big")
    return (ghash(h, aad, ct) ^ ej0).to_bytes(16, "big")


def encrypt(key, iv, aad, pt):
    """-> (ciphertext, tag)"""
    rk = expand_key(key)
    ct = bytearray()
    for i in range(0, len(pt), 16):
        ks = encrypt_block(rk, iv + struct.pack(">I", 2 + i // 16))
        ct += bytes(a ^ b for a, b in zip(pt[i:i + 16], ks))
    ct = bytes(ct)
    return ct, tag(key, iv, aad, ct)


# ---- the shared test inputs (tests/golden/make_gcm_fixtures.py, test_gcm_host.py, test_gpu_gcm.py)
S = 512  # FLTEE_GCM_SEGMENT_BLOCKS
IV = bytes(range(1, 13))
IDS = (0, 1, 258, 65535, 4242)
AAD_LENS = (0, 16, 20)
SMALL_LENS = (0, 8, 16, 24, 40, 16 * S - 8, 16 * S, 16 * S + 8)
SEGMENT_LENS = (16 * (2 * S + 1) + 8, 16 * 3 * S)  # two and three segments, a ragged tail
# n = 5 clients on each side of the CTR kernels' switch (k_aes.hip: the byte-per-lane kernel
# below 1024 quad-kernel waves of 512 counter blocks, the counters starting at 2)
SWITCH_LENS = (16 * (204 * 512 - 2), 16 * (204 * 512 - 1))


def plaintext(length, seed):
    import numpy as np
    i = np.arange(length, dtype=np.int64)
    return ((7 * i + 13 * seed + (i * i >> 5) + (i >> 9)) & 0xFF).astype(np.uint8).tobytes()


def aad_of(client_id, aad_len):
    return bytes((3 * i + client_id) & 0xFF for i in range(aad_len))


def case_key(client_id, length, aad_len):
    return f"{client_id}_{length}_{aad_len}"
