"""FLTEE_OPT_FP8 on the device: the decode of all 256 codes under eight scales against
tests/fp8_model.py; the fp8 accumulate (k_rows.hip) against the dense route on the dequantised
values serialized as records, bit for bit, at every load width the launcher ships; the options on
the fp8 route against the same records call; every other alg, the tree and the trims on fp8 rows
against the same call on the unpacked records; the producer against the model's quantise; and the
bytes a row does not own (padding, the trailer's last 4 bytes) reaching no output.

Shapes: d around the 8-code units (13, 15, 16, 17, 24, 25), P = ceil(d / 8) odd and even (rows of
16 n and 16 n + 8 bytes), 1031 for more than one block, both sides of the threshold (2^19) from
which a lane owns more than one output, with n = 3 and, above it, n = 17; n on both sides of the
batch of 16 clients in flight.  Below the threshold a lane owns one output whatever the
alignment; above it the width follows the alignment of the row base and the out base (rows.h
rows_width): the cases below reach 4, 2 and 1 outputs a lane."""
import ctypes
import functools

import numpy as np
import pytest

import fp8_model as FM
import trim_model as TM
from conftest import gpu_available
from stable_model import bits_equal
from test_fp8_abi import R_FP8, R_TRIM_DENSE, R_TRIM_SELECT_DENSE
from test_gpu_oblivious import assert_same_trace, traced
from test_plan import Plan

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SMALL_D = [13, 15, 16, 17, 24, 25, 1031]
T = 1 << 19  # rows.h kFp8SmallD
ALL_N = [1, 3, 17, 65]
# (row base offset in bytes, out base offset in floats) -> outputs a lane from T on: 4, 4, 4, 2, 1
# (below T: 1)
ALIGN = [(0, 0), (4, 0), (8, 0), (0, 2), (0, 1)]
SEED = 0x5EED0001F00D


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@functools.lru_cache(maxsize=None)
def host_rows(d, nans=False):
    """65 clients' fp8 rows of d codes (3 for the large d): built once, never modified"""
    r = FM.random_rows(np.random.default_rng(d), 65 if d <= 4096 else 3, d, nans=nans)
    r.setflags(write=False)
    return r


def cuda_rows(rows, offset=0):
    """the rows on the device, their base `offset` bytes into a 16-byte aligned buffer that ends
    with the last row"""
    import torch
    buf = torch.zeros(offset + rows.size, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:]
    t.copy_(torch.from_numpy(np.array(rows, np.uint8).reshape(-1)))
    assert t.data_ptr() % 16 == offset % 16
    return t


def records_of(values):
    import torch

    from fltee import client as C
    return C.serialize_dense(torch.from_numpy(np.ascontiguousarray(values)).cuda())


def fp8(dev, alg, rows, n, d, prev=None, out_offset=0, **kw):
    import torch
    buf = torch.zeros(d + 4, dtype=torch.float32, device="cuda")
    out = buf[out_offset:out_offset + d]
    if prev is not None:
        out.copy_(torch.from_numpy(prev))
    got = dev.aggregate(alg, rows, n, d, d, out=out, fp8=True, **kw).cpu().numpy()
    assert dev.status() == 0
    return got


def records_call(dev, alg, x, n, d, prev=None, **kw):
    import torch
    out = None if prev is None else torch.from_numpy(prev.copy()).cuda()
    ref = dev.aggregate(alg, records_of(x), n, d, d, out=out, **kw).cpu().numpy()
    assert dev.status() == 0
    return ref


# ----------------------------------------------------------------- the decode ----
SUBNORMAL_SCALE = np.float32(2.0 ** -140)  # every product is a subnormal f32 or rounds to zero
SCALES = np.array([1.0, 2.0 ** -20, 3.1e-4, SUBNORMAL_SCALE, -1.0, 0.0, np.inf, np.nan], np.float32)


def test_every_code_under_every_scale_decodes_to_the_models_bits(dev):
    """fltee_unpack_fp8_device on 8 clients x 256 codes: every one of the 2048 products has the
    model's bits, NaN payloads included — the operand, quieted, where one operand is a NaN (at
    s = 1 that is the widening itself: sign << 31 | 0x7FC00000), and for the four products IEEE
    754 leaves to the multiplier (inf * +-0, NaN * the NaN codes) the patterns the model's own
    multiplier gives, which are the device's (printed)."""
    n, d = len(SCALES), 256
    codes = np.tile(np.arange(256, dtype=np.uint8), (n, 1))
    r = FM.pack_codes(codes, SCALES)
    rec = dev.unpack_fp8(cuda_rows(r), n, d).cpu().numpy()
    idx, val = dev.unpack_records(rec)
    assert np.array_equal(idx.reshape(n, d), np.tile(np.arange(d, dtype=np.uint32), (n, 1)))
    got, want = val.reshape(n, d), FM.dequant(codes, SCALES)
    w = FM.widen(codes)
    exact = ~np.isnan(want) | (np.isnan(w) ^ np.isnan(SCALES)[:, None])
    assert exact[:6].all() and exact.sum() == 8 * 256 - 4  # inf * +-0, NaN * the two NaN codes
    assert np.array_equal(got.view(np.uint32)[exact], want.view(np.uint32)[exact])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the widening, spelled out: s = 1 changes nothing
    assert np.array_equal(got[0].view(np.uint32), FM.TABLE.view(np.uint32))
    assert got.view(np.uint32)[0, 0x7F] == 0x7FC00000 and got.view(np.uint32)[0, 0xFF] == 0xFFC00000
    assert (np.abs(got[3][np.isfinite(got[3])]) < 2.0 ** -126).all() and got[3].any()  # subnormal products
    print("inf * +-0, NaN * NaN codes:", [hex(b) for b in got.view(np.uint32)[~exact]],
          "model:", [hex(b) for b in want.view(np.uint32)[~exact]])


# ------------------------------------------------------------ the accumulate ----
@pytest.mark.parametrize("d", SMALL_D)
def test_fp8_accumulate_equals_the_records_call(dev, d):
    allr = host_rows(d)
    for n in ALL_N:
        r = allr[:n]
        assert Plan(3, n, d, d, fp8=True).route == R_FP8
        x = FM.unpack(r, d)
        want = FM.inorder_mean(r, d)
        assert np.isfinite(want).all()
        ref = records_call(dev, 3, x, n, d, dense=True)
        assert bits_equal(ref, want)
        for offset, out_offset in ALIGN:
            rows = cuda_rows(r, offset)
            got = fp8(dev, 3, rows, n, d, out_offset=out_offset)
            assert bits_equal(got, ref), (n, offset, out_offset)
            if n == 17:  # the other flat algs take the same route
                for alg in (4, 5):
                    assert bits_equal(fp8(dev, alg, rows, n, d, out_offset=out_offset), ref)


@pytest.mark.parametrize("n,d", [(3, T + 3), (3, T + 11), (3, T), (3, T - 1), (3, T - 5), (17, T + 3)])
def test_fp8_accumulate_at_the_width_threshold(dev, n, d):
    """from T outputs on a lane owns up to 4 (the last group of T + 3 and T + 11 reaching into
    the padding), 2 or 1 by the out base; below, one.  n = 17: a full batch of 16 clients and
    the guarded tail at the widths that exist only from T on"""
    r = FM.random_rows(np.random.default_rng(d), n, d) if n > 3 else host_rows(d)
    ref = records_call(dev, 3, FM.unpack(r, d), n, d, dense=True)
    assert bits_equal(ref, FM.inorder_mean(r, d))
    for offset, out_offset in ALIGN:
        assert bits_equal(fp8(dev, 3, cuda_rows(r, offset), n, d, out_offset=out_offset), ref)


@pytest.mark.parametrize("n,d", [(17, 1031), (3, 25)])
def test_nan_codes_and_hostile_scales_equal_the_records_call(dev, n, d):
    """NaN codes of both signs, and clients whose scale is NaN, inf, 0 and negative: the same adds
    in the same order as the records route — the same bits wherever the sum is a number"""
    codes, s = FM.split(host_rows(d, nans=True)[:n], d)
    s = s.copy()
    s[:3] = [np.inf, -2.5e-3, 0.0]
    if n > 3:
        s[n - 1] = np.nan
    r = FM.pack_codes(codes, s)
    x = FM.unpack(r, d)
    assert np.isnan(x).any() and np.isinf(x).any()
    ref = records_call(dev, 3, x, n, d, dense=True)
    assert np.isnan(ref).any()
    for offset, out_offset in ALIGN:
        assert FM.same_bits(fp8(dev, 3, cuda_rows(r, offset), n, d, out_offset=out_offset), ref)


# ------------------------------------------------------------------- options ----
OPTIONS = [dict(clip=True, clipping=0.05), dict(accumulate=True), dict(no_average=True), dict(n_avg=7),
           dict(accumulate=True, clip=True, clipping=0.05, n_avg=7),
           dict(dp=True, seed=SEED, clip=True, clipping=0.05, sigma=1.12),
           dict(dp=True, seed=SEED, sigma=1.12, n_avg=7, clipping=0.25)]


@pytest.mark.parametrize("kw", OPTIONS, ids=lambda kw: "-".join(k for k in kw if k not in ("clipping", "sigma", "seed")))
@pytest.mark.parametrize("n,d", [(6, 25), (17, 1031), (3, T + 3)])
def test_options_on_the_fp8_route_equal_the_records_call(dev, n, d, kw):
    """CLIP (the f64 norm over the x values; x * cc rounded before the add: two roundings, scale
    first), ACCUMULATE, NO_AVERAGE, n_avg and DP under a fixed seed: the dense route's bits on
    the records (j, x_j)"""
    r = host_rows(d)[:n]
    x = FM.unpack(r, d)
    prev = np.random.default_rng(d).normal(0, 1, d).astype(np.float32) if kw.get("accumulate") else None
    ref = records_call(dev, 3, x, n, d, prev=prev, dense=True, **kw)
    plain = records_call(dev, 3, x, n, d, dense=True)
    assert not bits_equal(ref, plain)  # the option did something
    if kw.get("clip") and d == 1031:   # (every norm is above the bound: the coefficients are not 1)
        assert (np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)) > 2 * kw["clipping"]).all()
    for offset, out_offset in ALIGN:
        rows = cuda_rows(r, offset)
        assert bits_equal(fp8(dev, 3, rows, n, d, prev=prev, out_offset=out_offset, **kw), ref)
        assert np.array_equal(rows.cpu().numpy(), r.reshape(-1))  # the rows were not written


# ------------------------------------------------------------------ every alg ----
EVERY = [(1, {}), (2, dict(seed=7)), (7, {}), (5, dict(oram_tree=True)), (5, dict(oram_tree=True, oram_lazy=True)),
         (3, dict(trim=1)), (4, dict(trim=2)), (3, dict(trim=2, trim_select=True))]


@pytest.mark.parametrize("alg,kw", EVERY, ids=lambda x: str(x) if isinstance(x, int) else "-".join(x) or "plain")
@pytest.mark.parametrize("d", [13, 257])
def test_every_other_route_equals_the_call_on_unpacked_records(dev, alg, kw, d):
    n = 5
    r = FM.pack_codes(*[a[:n] if a.ndim == 1 else a[:n, :d] for a in FM.split(host_rows(1031), 1031)])
    rows = cuda_rows(r)
    rec = dev.unpack_fp8(rows, n, d)
    assert np.array_equal(rec.cpu().numpy(), records_of(FM.unpack(r, d)).cpu().numpy())
    dense = dict(dense=True) if "trim" in kw else {}
    for more in ({}, dict(clip=True, clipping=0.05)):
        want = dev.aggregate(alg, rec, n, d, d, **dense, **kw, **more).cpu().numpy()
        assert dev.status() == 0
        assert bits_equal(fp8(dev, alg, rows, n, d, **kw, **more), want)
    assert np.array_equal(rows.cpu().numpy(), r.reshape(-1))  # never written


def test_trim_on_fp8_rows_is_the_records_trim(dev):
    """the median of 17 clients, one of them under a NaN scale and one under 1e30: trimmed away"""
    n, d, t = 17, 257, 8
    codes, s = FM.split(host_rows(1031)[:n], 1031)
    s = s.copy()
    s[4], s[9] = np.nan, 1e30
    r = FM.pack_codes(codes[:, :d], s)
    x = FM.unpack(r, d)
    assert np.isnan(x[4]).all()
    assert Plan(3, n, d, d, fp8=True, trim=t).route == R_TRIM_DENSE
    assert Plan(3, n, d, d, fp8=True, trim=t, trim_select=True).route == R_TRIM_SELECT_DENSE
    model = TM.trimmed(x, t)
    assert np.isfinite(model).all() and (np.abs(model) < 1).all()
    rows = cuda_rows(r)
    assert bits_equal(fp8(dev, 3, rows, n, d, trim=t), model)
    assert bits_equal(fp8(dev, 5, rows, n, d, trim=t, trim_select=True), model)
    assert not np.isfinite(fp8(dev, 3, rows, n, d)).any()  # (the untrimmed mean is theirs)


def test_fp8_refusals_on_the_device(dev):
    import torch

    from fltee import _lib as L
    rows = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.zeros(16, dtype=torch.float32, device="cuda")
    for alg, n, k, d, kw, off in [(3, 4, 13, 14, {}, 0), (3, 4, 12, 12, {}, 0), (1, 4, 15, 14, {}, 0),
                                  (3, 4, 14, 14, dict(packed=True), 0), (3, 4, 14, 14, dict(bf16=True), 0),
                                  (3, 4, 14, 14, {}, 1), (3, 4, 14, 14, {}, 2)]:
        o = dev.opts(fp8=True, **kw)
        st = L.lib().fltee_aggregate_device(alg, ctypes.c_void_p(rows.data_ptr() + off), n, k, d,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.byref(o), None)
        assert st == L.ERROR_INVALID_PARAMETER
    o = dev.opts(fp8=True)
    assert L.lib().fltee_aggregate_device(3, ctypes.c_void_p(rows.data_ptr()), 4, 14, 14,
                                          ctypes.c_void_p(out.data_ptr()), ctypes.byref(o), None) == 0
    assert dev.status() == 0


# ------------------------------------------------------------------- producer ----
def producer_values(d):
    """8 clients: exact midpoints under s = 1 and under s = 2^-10, N(0, 1), all zeros, a row with
    +-inf, a row with NaNs of both signs, a row whose absmax / 448 is subnormal (s = 1), +-0"""
    rng = np.random.default_rng(d)
    v = rng.normal(0, 1, (8, d)).astype(np.float32)
    mids = np.concatenate([FM.MIDS, -FM.MIDS]).astype(np.float32)
    m = min(d - 1, mids.size)
    v[0, :m], v[0, m] = mids[:m], 448.0
    v[1] *= np.float32(0.01)  # (below the row's 448 * 2^-10)
    v[1, :m], v[1, m] = mids[:m] * np.float32(2.0 ** -10), -448.0 * 2.0 ** -10
    v[3] = 0.0
    v[4, ::5], v[4, 1::7] = np.inf, -np.inf
    v[5, ::4], v[5, 2::9] = np.nan, -np.nan
    v[6] = (rng.normal(0, 1, d) * 1e-40).astype(np.float32)
    v[7, ::2], v[7, 1::4] = 0.0, -0.0
    return v


@pytest.mark.parametrize("d", [13, 24, 300, 1031])
def test_producer_equals_the_models_quantise(dev, d):
    import torch

    from fltee import client as C
    v = producer_values(d)
    n = v.shape[0]
    codes, s = FM.quantise(v)
    assert s[0] == 1.0 and s[1] == 2.0 ** -10 and s[3] == 1.0 and s[6] == 1.0 and np.isfinite(s).all()
    assert 0 < np.abs(v[6]).max() / np.float32(448) < 2.0 ** -126
    if d == 300:  # every midpoint is there, and ties to the even code
        assert np.array_equal(codes[0, :126] & 1, np.zeros(126, np.uint8)) and np.array_equal(codes[0, :126], codes[1, :126])
    dv = torch.from_numpy(v).cuda()
    traced_lines = traced(lambda: C.pack_dense_fp8(dv))
    rows = C.pack_dense_fp8(dv)
    assert rows.dtype == torch.uint8 and tuple(rows.shape) == (n, FM.row(d))
    got = rows.cpu().numpy()
    want = FM.pack(v)
    gc, gs = FM.split(got, d)
    assert np.array_equal(gs.view(np.uint32), s.view(np.uint32))
    assert np.array_equal(gc, codes)
    assert np.array_equal(got, want)  # padding 0x00, the trailer's last 4 bytes zero
    assert sum("fp8_scale_kernel" in line for line in traced_lines) == 1
    assert sum("fp8_quantise_kernel" in line for line in traced_lines) == 1
    # deterministic: the maximum does not depend on the order it is taken in
    assert np.array_equal(C.pack_dense_fp8(dv).cpu().numpy(), got)
    idx, val = dev.unpack_records(dev.unpack_fp8(rows, n, d).cpu().numpy())
    assert np.array_equal(idx, np.tile(np.arange(d, dtype=np.uint32), n))
    assert FM.same_bits(val, FM.unpack(want, d).reshape(-1))
    # sealed, decrypted: the same bytes; produce_payloads(fp8=True) is that payload
    ids = np.arange(40, 40 + n, dtype=np.uint32)
    enc = C.encrypt_parameters(rows, ids)
    assert enc.numel() == n * FM.slice_bytes(d)
    plain = torch.empty(n * FM.row(d), dtype=torch.uint8, device="cuda")
    dev.decrypt(ids, enc, FM.slice_bytes(d), plain)
    assert np.array_equal(plain.cpu().numpy(), want.reshape(-1))
    assert np.array_equal(C.produce_payloads(dv, ids, fp8=True).cpu().numpy(), enc.cpu().numpy())


# ------------------------------------------------------------ bytes not owned ----
@pytest.mark.parametrize("n,d", [(5, 13), (17, 1031), (3, 25), (3, T + 3)])
def test_padding_and_the_trailers_tail_reach_no_output(dev, n, d):
    """0xFF (the NaN code; as an f32 a NaN too) in bytes [d, 8 P) and in the trailer's last 4
    bytes: every output, through the accumulate at every width it ships, the norm and the unpack, is what
    the clean rows give.  The rows end with their buffer: nothing past the last row is read."""
    codes, s = FM.split(host_rows(d)[:n], d)
    clean, dirty = FM.pack_codes(codes, s), FM.pack_codes(codes, s, pad=0xFF, tail=0xFF)
    assert d % 8 and not np.array_equal(clean, dirty)
    want = FM.inorder_mean(clean, d)
    assert np.isfinite(want).all()
    for offset, out_offset in ALIGN:
        rows = cuda_rows(dirty, offset)
        assert rows.data_ptr() + rows.numel() == rows.untyped_storage().data_ptr() + rows.untyped_storage().nbytes()
        for kw in ({}, dict(clip=True, clipping=1e30)):
            assert bits_equal(fp8(dev, 3, rows, n, d, out_offset=out_offset, **kw), want)
    rows = cuda_rows(dirty)
    clipped = fp8(dev, 3, cuda_rows(clean), n, d, clip=True, clipping=0.05)
    assert bits_equal(fp8(dev, 3, rows, n, d, clip=True, clipping=0.05), clipped) and not bits_equal(clipped, want)
    idx, val = dev.unpack_records(dev.unpack_fp8(rows, n, d).cpu().numpy())
    assert bits_equal(val, FM.unpack(clean, d).reshape(-1))
    if d < 60000:
        assert bits_equal(fp8(dev, 7, rows, n, d), want)


@pytest.mark.parametrize("alg,kw", [(3, {}), (3, dict(clip=True, clipping=0.5)), (1, {}), (7, dict(clip=True, clipping=0.5)),
                                    (3, dict(trim=1))])
def test_a_reserved_fp8_call_grows_no_scratch(dev, alg, kw):
    import torch

    from fltee import _lib as L
    n, d = 5, 1031
    rows = cuda_rows(host_rows(d)[:n])
    L.lib().fltee_debug_scratch_release()
    L.lib().fltee_debug_scratch_grown()
    dev.reserve(alg, n, d, d, fp8=True, **kw)
    grown = L.lib().fltee_debug_scratch_grown()
    assert bool(grown) == bool(dev.workspace_bytes(alg, n, d, d, fp8=True, **kw))
    fp8(dev, alg, rows, n, d, **kw)
    torch.cuda.synchronize()
    assert L.lib().fltee_debug_scratch_grown() == 0


# ---------------------------------------------------------------------- trace ----
@pytest.mark.parametrize("alg,n,d,kw", [(3, 17, 1031, {}), (3, 17, 1031, dict(clip=True, clipping=0.5)),
                                        (4, 3, T + 3, {}), (3, 17, 257, dict(trim=1)), (1, 5, 257, {})])
def test_two_inputs_of_one_shape_give_one_trace(dev, alg, n, d, kw):
    """the launches of an fp8 call depend on (alg, n, d) and the options, never on the values:
    random codes against rows of zeros, NaN codes and hostile scales"""
    import torch
    a = cuda_rows(FM.random_rows(np.random.default_rng(1), n, d))
    codes = np.zeros((n, d), np.uint8)
    codes[0, :] = 0x7E
    codes[n - 1, ::3] = 0xFF
    s = np.ones(n, np.float32)
    s[0], s[1] = np.inf, np.nan
    b = cuda_rows(FM.pack_codes(codes, s))
    out = torch.empty(d, dtype=torch.float32, device="cuda")
    dev.reserve(alg, n, d, d, fp8=True, **kw)
    for rows in (a, b):  # warm: code objects loaded, scratch grown
        dev.aggregate(alg, rows, n, d, d, out=out, fp8=True, **kw)
    ta = traced(lambda: dev.aggregate(alg, a, n, d, d, out=out, fp8=True, **kw))
    tb = traced(lambda: dev.aggregate(alg, b, n, d, d, out=out, fp8=True, **kw))
    dev.status()
    assert any("dense_accumulate_q" in line for line in ta) == (alg != 1 and "trim" not in kw)
    assert any("unpack_fp8_kernel" in line for line in ta) == (alg == 1 or "trim" in kw)
    assert any("fp8_norm_kernel" in line for line in ta) == ("clip" in kw)
    assert_same_trace(ta, tb, f"alg {alg} n={n} d={d} {kw}")
