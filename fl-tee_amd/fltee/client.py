"""Client-side producers on the GPU, named after the reference's
client functions in src/utils.py / src/update.py.

fl_main.py:221-238 turns each sampled client's update into its upload:

    top, idxs = zero_except_top_k_weights(diff, buffer_names, k)   # utils.py:327-354
    if dp: top = l2clipping(top, buffer_names, clipping)            # update.py:187-204
    b = serialize_sparse(top, buffer_names, idxs)                   # utils.py:193-209
    (dense: l2clipping + serialize_dense, utils.py:171-190)
    enc = encrypt_parameters(b, client_id)                          # utils.py:268-290

and concatenates the clients' ciphertexts in sampling order.  Here the n clients'
flattened learnable parameters are one [n, d] f32 CUDA tensor and every step is a
kernel of libfltee_agg (no CPU path):

    payload = produce_payloads(values, client_ids, k=k, clipping=C)   # uint8 CUDA tensor

The payload can go into an Aggregate request as is, or straight to the device-side
aggregation (fltee_decrypt_device + fltee_aggregate_device) for a GPU-resident round.
"""
import ctypes
import struct

import numpy as np
import torch

from . import _lib as L
from .device import _check, _ptr, _stream


def _values(values):
    assert values.is_cuda and values.dtype == torch.float32 and values.dim() == 2
    return values.contiguous()


def zero_except_top_k_weights(values, k, stream=None):
    """[n, d] -> int64 records [n*k]: (idx, val) of the k largest |val| per client in the
    reference's order (|val| descending, ties by ascending idx)."""
    v = _values(values)
    n, d = v.shape
    rec = torch.empty(n * k, dtype=torch.int64, device=v.device)
    _check(L.lib().fltee_client_topk_device(_ptr(v), n, d, k, _ptr(rec), _stream(stream)),
           "fltee_client_topk_device")
    return rec


def serialize_dense(values, stream=None):
    """[n, d] -> int64 records [n*d]: (i, v[i])."""
    v = _values(values)
    n, d = v.shape
    rec = torch.empty(n * d, dtype=torch.int64, device=v.device)
    _check(L.lib().fltee_client_serialize_dense_device(_ptr(v), n, d, _ptr(rec), _stream(stream)),
           "fltee_client_serialize_dense_device")
    return rec


def _pack_rows(what, values, per_unit, dtype, stream):
    v = _values(values)
    n, d = v.shape
    out = torch.empty((n, -(-d // per_unit) * per_unit), dtype=dtype, device=v.device)
    _check(getattr(L.lib(), what)(_ptr(v), n, d, _ptr(out), _stream(stream)), what)
    return out


def pack_dense(values, stream=None):
    """[n, d] -> f32 [n, 2 * ceil(d / 2)]: the packed dense slices (fltee.ecalls.
    set_upload_packed) — each client's d values in position order, then one +0.0 when d is odd;
    half the bytes of serialize_dense."""
    return _pack_rows("fltee_client_pack_dense_device", values, 2, torch.float32, stream)


def pack_dense_bf16(values, stream=None):
    """[n, d] f32 -> int16 [n, 4 * ceil(d / 4)]: the bf16 dense slices (fltee.ecalls.
    set_upload_bf16) — each client's d values narrowed to bf16 (round to nearest even; a NaN
    keeps its sign and is quieted) in position order, then +0.0 up to a whole 8-byte unit; a
    quarter of the bytes of serialize_dense.  The server widens exactly: quantisation is the
    client's choice and the client's error."""
    return _pack_rows("fltee_client_pack_bf16_device", values, 4, torch.int16, stream)


def pack_dense_fp8(values, stream=None):
    """[n, d] f32 -> uint8 [n, 8 * (ceil(d / 8) + 1)]: the fp8 dense slices (fltee.ecalls.
    set_upload_fp8) — each client's d values as OCP e4m3fn codes of v / s (s = the row's largest
    finite |v| / 448, or 1 where that is no normal f32; nearest code, ties to even, saturating at
    448) in position order, 0x00 up to a whole 8-byte unit, then one unit more: s as a
    little-endian f32 and 4 zero bytes.  An eighth of the bytes of serialize_dense, plus the
    trailer.  The server widens exactly and multiplies by s once: quantisation is the client's
    choice and the client's error."""
    v = _values(values)
    n, d = v.shape
    out = torch.empty((n, 8 * (-(-d // 8) + 1)), dtype=torch.uint8, device=v.device)
    _check(L.lib().fltee_client_pack_fp8_device(_ptr(v), n, d, _ptr(out), _stream(stream)),
           "fltee_client_pack_fp8_device")
    return out


def l2clipping(records, n, k, clipping, stream=None):
    """In place on n clients x k records: val *= min(1, clipping / ||values||_2)."""
    assert records.is_cuda and records.dtype == torch.int64 and records.numel() >= n * k
    _check(L.lib().fltee_client_clip_device(_ptr(records), n, k, float(clipping), _stream(stream)),
           "fltee_client_clip_device")
    return records


def encrypt_parameters(records, client_ids, stream=None):
    """Records of n clients (equal counts) -> uint8 ciphertext, client-major."""
    ids = np.ascontiguousarray(client_ids, dtype=np.uint32)
    n = len(ids)
    plain = records.contiguous().view(torch.uint8)
    assert plain.numel() % n == 0
    out = torch.empty_like(plain)
    _check(L.lib().fltee_encrypt_device(ids.ctypes.data_as(ctypes.c_void_p), n, _ptr(plain),
                                        plain.numel() // n, _ptr(out), _stream(stream)),
           "fltee_encrypt_device")
    return out


def ecall_iv(fl_id, round_):
    """The 12-byte IV the ECALLs use with authenticated uploads: BE32(fl_id) || BE32(round) ||
    BE32(0)."""
    return struct.pack(">III", fl_id, round_, 0)


def ecall_aad(fl_id, round_, client_ids, aggregation_alg, packed=False, bf16=False, fp8=False):
    """The ECALLs' AAD, 16 bytes per client: BE32(fl_id) || BE32(round) || BE32(client_id) ||
    BE32(aggregation_alg) — a slice cannot be replayed in another round, moved to another
    client or submitted under another algorithm.  packed: the slices are packed dense values
    (pack_dense); the last word is BE32(aggregation_alg | 0x80000000), so a slice sealed as
    records never verifies as packed values, nor the other way round.  bf16: the slices are
    bf16 values (pack_dense_bf16); the last word is BE32(aggregation_alg | 0x40000000).  fp8: the
    slices are fp8 codes with their scale (pack_dense_fp8); BE32(aggregation_alg | 0x20000000)."""
    assert bool(packed) + bool(bf16) + bool(fp8) <= 1
    word = (aggregation_alg | (L.AAD_PACKED_BIT if packed else 0) | (L.AAD_BF16_BIT if bf16 else 0)
            | (L.AAD_FP8_BIT if fp8 else 0))
    return b"".join(struct.pack(">IIII", fl_id, round_, int(c), word) for c in client_ids)


def encrypt_parameters_gcm(records, client_ids, iv, aad=b"", stream=None):
    """AES-128-GCM of n clients' records (equal counts) -> uint8 [n, B + 16]: ciphertext ||
    tag per client, one 12-byte IV, aad = n equal parts of at most 64 bytes."""
    ids = np.ascontiguousarray(client_ids, dtype=np.uint32)
    n = len(ids)
    plain = records.contiguous().view(torch.uint8).reshape(-1)
    assert len(iv) == 12 and plain.numel() % n == 0 and len(aad) % n == 0
    B = plain.numel() // n
    out = torch.empty(n * (B + L.GCM_TAG_BYTES), dtype=torch.uint8, device=plain.device)
    ivb = (ctypes.c_uint8 * 12)(*iv)
    aadb = (ctypes.c_uint8 * max(len(aad), 1))(*aad)
    _check(L.lib().fltee_encrypt_auth_device(ids.ctypes.data_as(ctypes.c_void_p), n, _ptr(plain), B,
                                             ivb, aadb, len(aad) // n, _ptr(out), _stream(stream)),
           "fltee_encrypt_auth_device")
    return out.reshape(n, B + L.GCM_TAG_BYTES)


def encrypt_parameters_auth(records, client_ids, fl_id, round_, aggregation_alg, stream=None,
                            packed=False, bf16=False, fp8=False):
    """The authenticated upload of an ECALL (fltee.ecalls.set_upload_aead): the payload of
    ecall_secure_aggregation(fl_id, round_, client_ids, ..., aggregation_alg).  packed:
    `records` is pack_dense's tensor (any tensor is sealed by its bytes, n equal parts); bf16:
    pack_dense_bf16's; fp8: pack_dense_fp8's."""
    return encrypt_parameters_gcm(records, client_ids, ecall_iv(fl_id, round_),
                                  ecall_aad(fl_id, round_, client_ids, aggregation_alg, packed, bf16, fp8),
                                  stream).reshape(-1)


def produce_payloads(values, client_ids, k=None, clipping=None, stream=None, packed=False, bf16=False,
                     fp8=False):
    """fl_main.py:221-238 for every client at once: k=None -> dense uploads; packed (dense
    only): value-only slices of 8 * ceil(d / 2) bytes per client (pack_dense), for a server
    with fltee.ecalls.set_upload_packed(True); bf16 (dense only): bf16 slices of
    8 * ceil(d / 4) bytes per client (pack_dense_bf16), for a server with
    fltee.ecalls.set_upload_bf16(True); fp8 (dense only): fp8 slices of 8 * (ceil(d / 8) + 1)
    bytes per client (pack_dense_fp8), for a server with fltee.ecalls.set_upload_fp8(True)."""
    v = _values(values)
    n, d = v.shape
    assert len(client_ids) == n
    if packed or bf16 or fp8:
        assert bool(packed) + bool(bf16) + bool(fp8) == 1 and (k is None or k == d), \
            "packed, bf16 and fp8 uploads are dense"
        if clipping is not None:  # clipped as records (the reference's arithmetic), then packed
            rec = l2clipping(serialize_dense(v, stream), n, d, clipping, stream)
            v = rec.view(torch.float32).reshape(n, d, 2)[:, :, 1].contiguous()
        rows = pack_dense_fp8(v, stream) if fp8 else pack_dense_bf16(v, stream) if bf16 else pack_dense(v, stream)
        return encrypt_parameters(rows, client_ids, stream)
    if k is None:
        rec, kk = serialize_dense(v, stream), d
    else:
        rec, kk = zero_except_top_k_weights(v, k, stream), k
    if clipping is not None:
        l2clipping(rec, n, kk, clipping, stream)
    return encrypt_parameters(rec, client_ids, stream)
