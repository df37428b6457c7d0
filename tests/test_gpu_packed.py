"""FLTEE_OPT_PACKED on the device: the packed accumulate (k_rows.hip) against the dense route
on the same values serialized as records and against numpy's in-order f32 sum, bit for bit;
the options on the packed route against tests/options_model.py; every other alg on packed rows
against the same call on the unpacked records; the producer round trip; and a reserved packed
call growing no scratch.

Shapes: d % 4 in every class, U = ceil(d / 2) odd and even (8-byte and 16-byte rows), both
sides of the packed accumulate's small-d threshold (2^18) with U odd (2^18 + 6) and U even
(2^18 + 8, and the odd d = 2^18 + 7 whose last 16-byte group ends in the padding); n on both
sides of the batches of 16, 32 and 64 clients the kernel keeps in flight."""
import ctypes
import functools

import numpy as np
import pytest

import packed_model as PM
from conftest import gpu_available
from options_model import (GENERAL_CLIPPING, LATTICE_CLIPPING, bincount_sums, clip_coefs, general, lattice,
                           lattice_prev)
from stable_model import bits_equal
from test_packed_abi import R_PACKED
from test_plan import Plan

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SMALL_D = [2, 3, 4, 5, 7, 1023, 1024, 1026, 4097]
LARGE_D = [50890, (1 << 18) + 6, (1 << 18) + 7, (1 << 18) + 8]
ALL_N = [1, 2, 15, 16, 17, 33, 100]
SEED = 0x5EED0001F00D


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@functools.lru_cache(maxsize=None)
def host_values(d):
    """100 clients of d values (33 for the large d): built once, never modified"""
    v = PM.values(np.random.default_rng(d), 100 if d <= 4097 else 33, d)
    v.setflags(write=False)
    return v


def cuda_rows(values, pad=0.0, offset=0):
    """the packed rows on the device, their base `offset` floats into a 16-byte aligned buffer"""
    import torch
    rows = PM.pack(values, pad)
    buf = torch.zeros(rows.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:offset + rows.size]
    t.copy_(torch.from_numpy(rows.reshape(-1)))
    assert t.data_ptr() % 16 == (4 * offset) % 16
    return t


def records_of(values):
    import torch

    from fltee import client as C
    return C.serialize_dense(torch.from_numpy(np.ascontiguousarray(values)).cuda())


def packed(dev, alg, rows, n, d, prev=None, **kw):
    import torch
    out = None if prev is None else torch.from_numpy(prev.copy()).cuda()
    got = dev.aggregate(alg, rows, n, d, d, out=out, packed=True, **kw).cpu().numpy()
    assert dev.status() == 0
    return got


# ------------------------------------------------------------ the accumulate ----
@pytest.mark.parametrize("d", SMALL_D + LARGE_D)
def test_packed_accumulate_equals_the_dense_route_and_numpy(dev, d):
    allv = host_values(d)
    for n in [n for n in ALL_N if n <= allv.shape[0]]:
        v = allv[:n]
        assert Plan(3, n, d, d, packed=True).route == R_PACKED
        want = PM.inorder_mean(v)
        rec = records_of(v)
        ref = dev.aggregate(3, rec, n, d, d, dense=True).cpu().numpy()
        assert dev.status() == 0
        rows = cuda_rows(v)
        got = packed(dev, 3, rows, n, d)
        diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"d={d} n={n}: {diff} of {d} differ from numpy's in-order sum")
        assert bits_equal(ref, want)
        assert bits_equal(got, want)
        if n == 17:  # the other flat algs take the same route
            for alg in (4, 5):
                assert bits_equal(packed(dev, alg, rows, n, d), want)


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("n,d", [(5, 1028), (17, 1027), (3, (1 << 18) + 8), (3, (1 << 18) + 7)])
def test_packed_base_off_16_bytes(dev, n, d, offset):
    """the base at 8 mod 16 (8-byte loads where the rows would allow 16) and at 4 / 12 mod 16
    (4-byte loads)"""
    v = host_values(d)[:n]
    got = packed(dev, 3, cuda_rows(v, offset=offset), n, d)
    assert bits_equal(got, PM.inorder_mean(v))


@pytest.mark.parametrize("n,d", [(5, 3), (17, 1027), (3, 50891), (3, (1 << 18) + 7), (33, (1 << 18) + 5)])
def test_nan_in_the_padding_reaches_no_output(dev, n, d):
    import torch
    assert d % 2 == 1
    v = np.random.default_rng(d).normal(0, 1, (n, d)).astype(np.float32)  # (norms far below the 1e30 clip)
    want = PM.inorder_mean(v)
    assert np.isfinite(want).all()
    for offset in (0, 2):
        rows = cuda_rows(v, pad=np.nan, offset=offset)
        assert torch.isnan(rows.reshape(n, d + 1)[:, d]).all()
        for kw in ({}, dict(clip=True, clipping=1e30)):
            got = packed(dev, 3, rows, n, d, **kw)
            assert np.isfinite(got).all() and bits_equal(got, want)
        # and through the unpack, for a route that reads records
        if n <= 5:
            assert bits_equal(packed(dev, 7, rows, n, d), want)
        idx, val = dev.unpack_records(dev.unpack_dense(rows, n, d).cpu().numpy())
        assert np.array_equal(idx.reshape(n, d), np.tile(np.arange(d, dtype=np.uint32), (n, 1)))
        assert bits_equal(val, v.reshape(-1))


# ------------------------------------------------------------------- options ----
OPTION_SHAPES = [(6, 257), (6, 1026)]


@pytest.mark.parametrize("n,d", OPTION_SHAPES)
def test_clip_on_the_packed_route(dev, n, d):
    _, val, _ = general(n, d, d, True)
    coef, clipped = clip_coefs(val, n, d, GENERAL_CLIPPING)
    assert (coef < 1).all()
    want = PM.inorder_mean(clipped.reshape(n, d))
    rows = cuda_rows(val.reshape(n, d))
    got = packed(dev, 3, rows, n, d, clip=True, clipping=GENERAL_CLIPPING)
    assert bits_equal(got, want)
    assert not bits_equal(got, PM.inorder_mean(val.reshape(n, d)))
    # the rows were not written
    assert bits_equal(rows.cpu().numpy(), PM.pack(val.reshape(n, d)).reshape(-1))


@pytest.mark.parametrize("mode", ["accumulate", "no_average", "n_avg"])
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("n,d", OPTION_SHAPES)
def test_unaveraged_options_on_the_packed_route(dev, n, d, clip, mode):
    idx, val, coef = lattice(n, d, d, True)
    rows = cuda_rows(val.reshape(n, d))
    more = {}
    if clip:
        got_coef, val = clip_coefs(val, n, d, LATTICE_CLIPPING)
        assert np.array_equal(got_coef, coef)
        more = dict(clip=True, clipping=LATTICE_CLIPPING)
    sums = bincount_sums(idx, val, d)
    if mode == "accumulate":
        prev = lattice_prev(d)
        want = prev + sums
        got = packed(dev, 3, rows, n, d, prev=prev, accumulate=True, **more)
        assert bits_equal(packed(dev, 3, rows, n, d, prev=prev, accumulate=True, n_avg=7, **more), want)
    elif mode == "no_average":
        want = sums
        got = packed(dev, 3, rows, n, d, no_average=True, **more)
    else:
        want = sums * (np.float32(1) / np.float32(7))
        got = packed(dev, 3, rows, n, d, n_avg=7, **more)
    assert bits_equal(got, want)


@pytest.mark.parametrize("n,d", OPTION_SHAPES)
def test_dp_on_the_packed_route(dev, oracle, n, d):
    _, val, _ = general(n, d, d, True)
    rows = cuda_rows(val.reshape(n, d))
    kw = dict(seed=SEED, clip=True, clipping=GENERAL_CLIPPING, n_avg=7, sigma=1.12)
    base = packed(dev, 3, rows, n, d, **kw)
    got = packed(dev, 3, rows, n, d, dp=True, **kw)
    noise = oracle.dp_noise(np.zeros(d, np.float32), 1.12, GENERAL_CLIPPING, 7, seed=SEED)
    assert noise.any()
    assert bits_equal(got, base + noise)


# ------------------------------------------------------------------ every alg ----
EVERY = [(1, {}), (2, dict(seed=7)), (6, dict(batch=2)), (7, {}), (5, dict(oram_tree=True)),
         (5, dict(oram_tree=True, oram_lazy=True))]


@pytest.mark.parametrize("alg,kw", EVERY, ids=lambda x: str(x) if isinstance(x, int) else "-".join(x) or "plain")
@pytest.mark.parametrize("d", [257, 1026])
def test_every_other_alg_equals_the_call_on_unpacked_records(dev, alg, kw, d):
    n = 5
    v = host_values(1026)[:n, :d]
    rows = cuda_rows(v)
    rec = dev.unpack_dense(rows, n, d)
    assert np.array_equal(rec.cpu().numpy(), records_of(v).cpu().numpy())
    for more in ({}, dict(clip=True, clipping=GENERAL_CLIPPING)):
        want = dev.aggregate(alg, rec, n, d, d, **kw, **more).cpu().numpy()
        assert dev.status() == 0
        got = packed(dev, alg, rows, n, d, **kw, **more)
        assert bits_equal(got, want)
    assert bits_equal(rows.cpu().numpy(), PM.pack(v).reshape(-1))  # never written


def test_packed_refusals_on_the_device(dev):
    import torch

    from fltee import _lib as L
    rows = torch.zeros(64, dtype=torch.float32, device="cuda")
    out = torch.zeros(8, dtype=torch.float32, device="cuda")
    for alg, n, k, d in [(3, 4, 3, 4), (3, 4, 1, 1), (1, 4, 5, 4)]:
        o = dev.opts(packed=True)
        st = L.lib().fltee_aggregate_device(alg, ctypes.c_void_p(rows.data_ptr()), n, k, d,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.byref(o), None)
        assert st == L.ERROR_INVALID_PARAMETER


# ------------------------------------------------------------------- producer ----
@pytest.mark.parametrize("n,d", [(3, 2), (4, 257), (5, 1026)])
def test_pack_seal_decrypt_unpack_round_trip(dev, n, d):
    import torch

    from fltee import client as C
    v = host_values(1026)[:n, :d]
    ids = np.arange(40, 40 + n, dtype=np.uint32)
    rows = C.pack_dense(torch.from_numpy(np.ascontiguousarray(v)).cuda())
    assert bits_equal(rows.cpu().numpy(), PM.pack(v))
    enc = C.encrypt_parameters(rows, ids)
    assert enc.numel() == n * PM.slice_bytes(d)
    assert not np.array_equal(enc.cpu().numpy(), rows.view(torch.uint8).reshape(-1).cpu().numpy())
    plain = torch.empty(n * PM.row(d), dtype=torch.float32, device="cuda")
    dev.decrypt(ids, enc, PM.slice_bytes(d), plain)
    assert bits_equal(plain.cpu().numpy(), PM.pack(v).reshape(-1))
    idx, val = dev.unpack_records(dev.unpack_dense(plain, n, d).cpu().numpy())
    assert np.array_equal(idx, np.tile(np.arange(d, dtype=np.uint32), n)) and bits_equal(val, v.reshape(-1))
    # produce_payloads(packed=True) is that payload
    assert np.array_equal(C.produce_payloads(torch.from_numpy(np.ascontiguousarray(v)).cuda(), ids,
                                             packed=True).cpu().numpy(), enc.cpu().numpy())


@pytest.mark.parametrize("alg,kw", [(3, {}), (3, dict(clip=True, clipping=0.5)), (1, {}), (7, dict(clip=True, clipping=0.5))])
def test_a_reserved_packed_call_grows_no_scratch(dev, alg, kw):
    import torch

    from fltee import _lib as L
    n, d = 5, 1026
    rows = cuda_rows(host_values(1026)[:n])
    L.lib().fltee_debug_scratch_release()
    L.lib().fltee_debug_scratch_grown()
    dev.reserve(alg, n, d, d, packed=True, **kw)
    grown = L.lib().fltee_debug_scratch_grown()
    assert bool(grown) == bool(dev.workspace_bytes(alg, n, d, d, packed=True, **kw))
    packed(dev, alg, rows, n, d, **kw)
    torch.cuda.synchronize()
    assert L.lib().fltee_debug_scratch_grown() == 0
