"""FLTEE_OPT_BF16 on the device: the bf16 accumulate (k_rows.hip) against the dense route on the
widened values serialized as records and against numpy's in-order f32 sum, bit for bit; every
load width and the scalar path by the base's alignment; the options on the bf16 route against
tests/options_model.py; every other alg, the tree and the trim on bf16 rows against the same call
on the unpacked records; the producer against the model's narrow and torch.bfloat16; a reserved
bf16 call growing no scratch; and the launch trace of two inputs of one shape.

Shapes: d % 8 in every class around the 4- and 8-output groups, Q = ceil(d / 4) odd and even
(8-byte and 16-byte rows), both sides of the bf16 accumulate's small-d threshold (2^19) with Q
odd and even and d % 8 != 0; n on both sides of the batches of 16, 32 and 64 clients the kernel
keeps in flight."""
import ctypes
import functools

import numpy as np
import pytest

import bf16_model as BM
import packed_model as PM
import trim_model as TM
from conftest import gpu_available
from options_model import (GENERAL_CLIPPING, LATTICE_CLIPPING, bincount_sums, clip_coefs, general_ok,
                           general_values, lattice, lattice_prev)
from stable_model import bits_equal
from test_bf16_abi import R_BF16, R_TRIM_DENSE
from test_gpu_oblivious import assert_same_trace, traced
from test_plan import Plan

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SMALL_D = [3, 4, 5, 7, 8, 9, 15, 16, 17, 1023, 1025, 1028, 4097]
T = 1 << 19  # rows.h kBf16SmallD
LARGE_D = [50890, T - 8, T - 4, T, T + 4, T + 7]
ALL_N = [1, 2, 15, 16, 17, 33, 65, 100]
SEED = 0x5EED0001F00D


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@functools.lru_cache(maxsize=None)
def host_rows(d):
    """100 clients' bf16 rows of d values (33 for the large d): built once, never modified"""
    r = BM.pack(BM.values(np.random.default_rng(d), 100 if d <= 4097 else 33, d))
    r.setflags(write=False)
    return r


def cuda_rows(rows, offset=0):
    """the rows on the device, their base `offset` halves into a 16-byte aligned buffer"""
    import torch
    buf = torch.zeros(rows.size + 8, dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:offset + rows.size]
    t.copy_(torch.from_numpy(np.array(rows, np.uint16).reshape(-1).view(np.int16)))
    assert t.data_ptr() % 16 == (2 * offset) % 16
    return t


def lattice_rows(val, n, d):
    """options_model's lattice / general values as bf16 rows, and the values as widened"""
    rows = BM.pack(val.reshape(n, d))
    return rows, BM.unpack(rows, d).reshape(-1)


@functools.lru_cache(maxsize=None)
def general_rows(n, d):
    """options_model.general's values narrowed to bf16: the first seed whose every client norm
    keeps that model's margin after the narrowing (a condition on the input, not a tolerance)"""
    for seed in range(64):
        _, val = general_values(n, d, d, True, seed)
        rows, wide = lattice_rows(val, n, d)
        if general_ok(wide, n, d):
            return rows, wide
    raise AssertionError("no seed keeps the margin")


def records_of(values):
    import torch

    from fltee import client as C
    return C.serialize_dense(torch.from_numpy(np.ascontiguousarray(values)).cuda())


def bf16(dev, alg, rows, n, d, prev=None, **kw):
    import torch
    out = None if prev is None else torch.from_numpy(prev.copy()).cuda()
    got = dev.aggregate(alg, rows, n, d, d, out=out, bf16=True, **kw).cpu().numpy()
    assert dev.status() == 0
    return got


# ------------------------------------------------------------ the accumulate ----
@pytest.mark.parametrize("d", SMALL_D + LARGE_D)
def test_bf16_accumulate_equals_the_dense_route_and_numpy(dev, d):
    allr = host_rows(d)
    for n in [n for n in ALL_N if n <= allr.shape[0]]:
        r = allr[:n]
        assert Plan(3, n, d, d, bf16=True).route == R_BF16
        want = BM.inorder_mean(r, d)  # (infinities among the values: inf - inf is a NaN)
        assert np.isnan(want).sum() <= max(2, d // 10)
        ref = dev.aggregate(3, records_of(BM.unpack(r, d)), n, d, d, dense=True).cpu().numpy()
        assert dev.status() == 0
        rows = cuda_rows(r)
        got = bf16(dev, 3, rows, n, d)
        diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"d={d} n={n}: {diff} of {d} differ from numpy's in-order sum")
        assert BM.same_bits(ref, want)
        assert BM.same_bits(got, want)
        assert bits_equal(got, ref)
        if n == 17:  # the other flat algs take the same route
            for alg in (4, 5):
                assert bits_equal(bf16(dev, alg, rows, n, d), got)


@pytest.mark.parametrize("offset", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n,d", [(5, 1032), (17, 1027), (3, T + 8), (3, T - 9)])
def test_bf16_base_off_16_bytes(dev, n, d, offset):
    """the base at 8 mod 16 (8-byte loads where the rows would allow 16), at 4 / 12 mod 16
    (4-byte loads) and at an odd half (the scalar path)"""
    r = host_rows(d)[:n]
    got = bf16(dev, 3, cuda_rows(r, offset=offset), n, d)
    assert BM.same_bits(got, BM.inorder_mean(r, d))
    assert bits_equal(got, bf16(dev, 3, cuda_rows(r), n, d))


@pytest.mark.parametrize("n,d", [(5, 5), (17, 1026), (3, 50891), (33, T + 5), (3, T - 5)])
def test_nan_in_the_padding_reaches_no_output(dev, n, d):
    import torch
    assert d % 4 in (1, 2, 3)
    v = np.random.default_rng(d).normal(0, 1, (n, d)).astype(np.float32)  # (norms far below the 1e30 clip)
    r = BM.pack(v, pad=0x7FC0)
    want = BM.inorder_mean(r, d)
    assert np.isfinite(want).all()
    for offset in (0, 4, 2, 1):
        rows = cuda_rows(r, offset=offset)
        assert torch.isnan(rows.view(torch.bfloat16).reshape(n, BM.row(d))[:, d:]).all()
        for kw in ({}, dict(clip=True, clipping=1e30)):
            got = bf16(dev, 3, rows, n, d, **kw)
            assert np.isfinite(got).all() and bits_equal(got, want)
        # and through the unpack, for a route that reads records
        if n <= 5 and d < 60000:
            assert bits_equal(bf16(dev, 7, rows, n, d), want)
        idx, val = dev.unpack_records(dev.unpack_bf16(rows, n, d).cpu().numpy())
        assert np.array_equal(idx.reshape(n, d), np.tile(np.arange(d, dtype=np.uint32), (n, 1)))
        assert bits_equal(val, BM.unpack(r, d).reshape(-1))


@pytest.mark.parametrize("n,d", [(17, 1027), (33, 4097)])
def test_nan_and_inf_inputs_equal_the_dense_route(dev, n, d):
    """NaNs of both signs and infinities among the values: the same adds in the same order as
    the records route — the same bits wherever the sum is a number, a NaN wherever it is one"""
    r = BM.pack(BM.values(np.random.default_rng(d + 1), n, d, nans=True))
    assert np.isnan(BM.unpack(r, d)).any()
    ref = dev.aggregate(3, records_of(BM.unpack(r, d)), n, d, d, dense=True).cpu().numpy()
    assert dev.status() == 0
    assert np.isnan(ref).any()
    for offset in (0, 4, 2, 1):
        assert BM.same_bits(bf16(dev, 3, cuda_rows(r, offset=offset), n, d), ref)


# ------------------------------------------------------------------- options ----
OPTION_SHAPES = [(6, 257), (6, 1026)]


@pytest.mark.parametrize("n,d", OPTION_SHAPES)
def test_clip_on_the_bf16_route(dev, n, d):
    r, val = general_rows(n, d)
    coef, clipped = clip_coefs(val, n, d, GENERAL_CLIPPING)
    assert (coef < 1).all()
    want = PM.inorder_mean(clipped.reshape(n, d))
    rows = cuda_rows(r)
    got = bf16(dev, 3, rows, n, d, clip=True, clipping=GENERAL_CLIPPING)
    assert bits_equal(got, want)
    assert not bits_equal(got, BM.inorder_mean(r, d))
    # the coefficients are the records route's, bit for bit: the same call on the records
    rec = records_of(val.reshape(n, d))
    ref = dev.aggregate(3, rec, n, d, d, dense=True, clip=True, clipping=GENERAL_CLIPPING).cpu().numpy()
    assert bits_equal(got, ref)
    # the rows were not written
    assert np.array_equal(rows.cpu().numpy().view(np.uint16), r.reshape(-1))


@pytest.mark.parametrize("mode", ["accumulate", "no_average", "n_avg"])
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("n,d", OPTION_SHAPES)
def test_unaveraged_options_on_the_bf16_route(dev, n, d, clip, mode):
    idx, val, coef = lattice(n, d, d, True)
    r, wide = lattice_rows(val, n, d)
    assert bits_equal(wide, val)  # the lattice values are bf16 values: nothing is lost
    rows = cuda_rows(r)
    more = {}
    if clip:
        got_coef, val = clip_coefs(val, n, d, LATTICE_CLIPPING)
        assert np.array_equal(got_coef, coef)
        more = dict(clip=True, clipping=LATTICE_CLIPPING)
    sums = bincount_sums(idx, val, d)
    if mode == "accumulate":
        prev = lattice_prev(d)
        want = prev + sums
        got = bf16(dev, 3, rows, n, d, prev=prev, accumulate=True, **more)
        assert bits_equal(bf16(dev, 3, rows, n, d, prev=prev, accumulate=True, n_avg=7, **more), want)
    elif mode == "no_average":
        want = sums
        got = bf16(dev, 3, rows, n, d, no_average=True, **more)
    else:
        want = sums * (np.float32(1) / np.float32(7))
        got = bf16(dev, 3, rows, n, d, n_avg=7, **more)
    assert bits_equal(got, want)


@pytest.mark.parametrize("n,d", OPTION_SHAPES)
def test_dp_on_the_bf16_route(dev, oracle, n, d):
    r, _ = general_rows(n, d)
    rows = cuda_rows(r)
    kw = dict(seed=SEED, clip=True, clipping=GENERAL_CLIPPING, n_avg=7, sigma=1.12)
    base = bf16(dev, 3, rows, n, d, **kw)
    got = bf16(dev, 3, rows, n, d, dp=True, **kw)
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
    r = BM.pack(BM.unpack(host_rows(1028)[:n], 1028)[:, :d])
    rows = cuda_rows(r)
    rec = dev.unpack_bf16(rows, n, d)
    assert np.array_equal(rec.cpu().numpy(), records_of(BM.unpack(r, d)).cpu().numpy())
    for more in ({}, dict(clip=True, clipping=GENERAL_CLIPPING)):
        want = dev.aggregate(alg, rec, n, d, d, **kw, **more).cpu().numpy()
        assert dev.status() == 0
        got = bf16(dev, alg, rows, n, d, **kw, **more)
        assert bits_equal(got, want)
    assert np.array_equal(rows.cpu().numpy().view(np.uint16), r.reshape(-1))  # never written


@pytest.mark.parametrize("n,t", [(17, 1), (17, 8), (5, 2)], ids=["t1", "median", "n5"])
@pytest.mark.parametrize("d", [257, 1027])
def test_trim_on_bf16_rows_is_the_records_trim(dev, n, t, d):
    """a trimmed bf16 call is trimmed: the records trim route on the unpacked copy, equal to the
    same call on the records and to tests/trim_model.py"""
    r = BM.pack(BM.values(np.random.default_rng(d + n), n, d, nans=True))
    v = BM.unpack(r, d)
    rows = cuda_rows(r)
    assert Plan(3, n, d, d, bf16=True, trim=t).route == R_TRIM_DENSE
    for more in ({}, dict(clip=True, clipping=GENERAL_CLIPPING)):
        want = dev.aggregate(3, records_of(v), n, d, d, dense=True, trim=t, **more).cpu().numpy()
        assert dev.status() == 0
        got = bf16(dev, 3, rows, n, d, trim=t, **more)
        assert BM.same_bits(got, want)
    model = TM.trimmed(v, t)
    assert np.isnan(model).mean() < 0.2
    assert BM.same_bits(bf16(dev, 4, rows, n, d, trim=t), model)
    assert not BM.same_bits(model, BM.inorder_mean(r, d))  # (not the untrimmed mean)


def test_bf16_refusals_on_the_device(dev):
    import torch

    from fltee import _lib as L
    rows = torch.zeros(64, dtype=torch.int16, device="cuda")
    out = torch.zeros(8, dtype=torch.float32, device="cuda")
    for alg, n, k, d, kw, off in [(3, 4, 3, 4, {}, 0), (3, 4, 2, 2, {}, 0), (1, 4, 5, 4, {}, 0),
                                  (3, 4, 4, 4, dict(packed=True), 0), (3, 4, 4, 4, {}, 1)]:
        o = dev.opts(bf16=True, **kw)
        st = L.lib().fltee_aggregate_device(alg, ctypes.c_void_p(rows.data_ptr() + off), n, k, d,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.byref(o), None)
        assert st == L.ERROR_INVALID_PARAMETER
    o = dev.opts(bf16=True)
    assert L.lib().fltee_aggregate_device(3, ctypes.c_void_p(rows.data_ptr()), 4, 4, 4,
                                          ctypes.c_void_p(out.data_ptr()), ctypes.byref(o), None) == 0
    assert dev.status() == 0


# ------------------------------------------------------------------- producer ----
@pytest.mark.parametrize("n,d", [(3, 3), (4, 257), (5, 1026), (2, 70001)])
def test_producer_round_trip(dev, n, d):
    import torch

    from fltee import client as C
    v = BM.values(np.random.default_rng(7 * d + n), n, d, nans=True)
    if d == 257:  # every listed pattern, whatever the sprinkling hit
        v.reshape(-1).view(np.uint32)[:BM.SPECIAL_BITS.size] = BM.SPECIAL_BITS
    assert np.isnan(v).any()
    dv = torch.from_numpy(v).cuda()
    rows = C.pack_dense_bf16(dv)
    assert rows.dtype == torch.int16 and tuple(rows.shape) == (n, BM.row(d))
    got = rows.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, BM.pack(v))  # the model's narrow, NaNs included; padding +0.0
    ok = ~np.isnan(v)
    t = dv.to(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got[:, :d][ok], t[ok])  # torch.bfloat16 off the NaNs
    idx, val = dev.unpack_records(dev.unpack_bf16(rows, n, d).cpu().numpy())
    assert np.array_equal(idx, np.tile(np.arange(d, dtype=np.uint32), n))
    assert bits_equal(val, BM.unpack(BM.pack(v), d).reshape(-1))
    # sealed, decrypted: the same bytes; produce_payloads(bf16=True) is that payload
    ids = np.arange(40, 40 + n, dtype=np.uint32)
    enc = C.encrypt_parameters(rows, ids)
    assert enc.numel() == n * BM.slice_bytes(d)
    plain = torch.empty(n * BM.row(d), dtype=torch.int16, device="cuda")
    dev.decrypt(ids, enc, BM.slice_bytes(d), plain)
    assert np.array_equal(plain.cpu().numpy().view(np.uint16), BM.pack(v).reshape(-1))
    assert np.array_equal(C.produce_payloads(dv, ids, bf16=True).cpu().numpy(), enc.cpu().numpy())


@pytest.mark.parametrize("alg,kw", [(3, {}), (3, dict(clip=True, clipping=0.5)), (1, {}), (7, dict(clip=True, clipping=0.5)),
                                    (3, dict(trim=1))])
def test_a_reserved_bf16_call_grows_no_scratch(dev, alg, kw):
    import torch

    from fltee import _lib as L
    n, d = 5, 1028
    rows = cuda_rows(host_rows(1028)[:n])
    L.lib().fltee_debug_scratch_release()
    L.lib().fltee_debug_scratch_grown()
    dev.reserve(alg, n, d, d, bf16=True, **kw)
    grown = L.lib().fltee_debug_scratch_grown()
    assert bool(grown) == bool(dev.workspace_bytes(alg, n, d, d, bf16=True, **kw))
    bf16(dev, alg, rows, n, d, **kw)
    torch.cuda.synchronize()
    assert L.lib().fltee_debug_scratch_grown() == 0


# ---------------------------------------------------------------------- trace ----
@pytest.mark.parametrize("alg,n,d,kw", [(3, 17, 1027, {}), (3, 33, 4097, dict(clip=True, clipping=0.5)),
                                        (4, 5, T + 4, {}), (3, 17, 1027, dict(trim=1)), (1, 5, 257, {})])
def test_two_inputs_of_one_shape_give_one_trace(dev, alg, n, d, kw):
    """the launches of a bf16 call depend on (alg, n, d) and the options, never on the values:
    N(0, 1) against rows of zeros, infinities and NaNs"""
    import torch
    a = cuda_rows(BM.pack(np.random.default_rng(1).normal(0, 1, (n, d)).astype(np.float32)))
    adv = np.zeros((n, d), np.float32)
    adv[0, :] = np.inf
    adv[n - 1, ::3] = np.nan
    b = cuda_rows(BM.pack(adv))
    out = torch.empty(d, dtype=torch.float32, device="cuda")
    dev.reserve(alg, n, d, d, bf16=True, **kw)
    for rows in (a, b):  # warm: code objects loaded, scratch grown
        dev.aggregate(alg, rows, n, d, d, out=out, bf16=True, **kw)
    ta = traced(lambda: dev.aggregate(alg, a, n, d, d, out=out, bf16=True, **kw))
    tb = traced(lambda: dev.aggregate(alg, b, n, d, d, out=out, bf16=True, **kw))
    dev.status()
    assert any("dense_accumulate_h" in line for line in ta) == (alg != 1 and "trim" not in kw)
    assert_same_trace(ta, tb, f"alg {alg} n={n} d={d} {kw}")
