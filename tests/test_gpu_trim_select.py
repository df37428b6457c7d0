"""FLTEE_OPT_TRIM | FLTEE_OPT_TRIM_SELECT on the device (k_trim_select.hip) against
tests/trim_model.py, bit for bit.

The kernel's public switch points, all functions of n alone (a block of 256 lanes owns C
columns, G = 256 / C client groups, a lane counts ceil(n / G) clients a round):
  C = 32 up to n = 512, 16 up to 1024, 8 up to 2048, 4 up to 4096 (FLTEE_TRIM_SELECT_MAX_N):
      swept on both sides — 512 | 513, 1024 | 1025, 2048 | 2049 — and at 4096 (d = 65);
  the clients-per-lane count is a run-time loop bound, ceil(n / G), unrolled by 8 with a
      remainder; the tile is padded to a whole number of G-client rows.  n = 64 | 65 (G = 8:
      8 | 9 clients a lane, the unrolled body alone | body + remainder), 129 | 131, 257 (one
      client past 32 rows) and 1000 (G = 16: 62.5 rows, 8 pad clients) sit on both sides of a
      multiple of G and of 8 G; n = 3 and 5 leave most lanes nothing but pads;
  the staging keeps 4 clients a lane in flight: batches of 4 G clients, the last one guarded
      (n = 3, 5, 65, 131, 257, 513, 1025, 2049 all end inside a batch).
d sweeps the column-tile tail at every C (d % 32, % 16, % 8, % 4 in {0, 1, 2, 3, 7, ...}) and
odd d with the packed padding float a NaN."""
import ctypes
import functools

import numpy as np
import pytest

import bf16_model as BM
import trim_model as TM
from conftest import gpu_available
from options_model import GENERAL_CLIPPING, general
from stable_model import bits_equal
from test_gpu_trim import DENSE_ORDER, LAYOUTS, NEG_NAN, POS_NAN, SEED, constructed, on_device, run
from test_plan import Plan
from test_trim_select_abi import R_SELECT_DENSE, R_SELECT_PACKED

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

ALL_D = [2, 3, 7, 8, 9, 31, 32, 33, 65, 257, 1101]
ALL_N = [3, 5, 64, 65, 129, 131, 257, 512, 513, 1000, 1024, 1025, 2048, 2049]
SEL = dict(trim_select=True)


def trims(n):
    return sorted(t for t in {1, 2, 64, 65, n // 10, (n - 1) // 2} if t >= 1 and 2 * t < n)


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@functools.lru_cache(maxsize=None)
def host_values():
    """4096 clients x 1101 finite values, half of them on a coarse grid (ties in every column):
    built once, never modified"""
    rng = np.random.default_rng(4096)
    v = rng.integers(-4, 5, (4096, 1101)).astype(np.float32) * np.float32(0.5)
    v = np.where(rng.random(v.shape) < 0.5, rng.normal(0, 100, v.shape).astype(np.float32), v)
    v = np.ascontiguousarray(v, np.float32)
    v.setflags(write=False)
    return v


def check(dev, v, ts, layouts=LAYOUTS, what=""):
    """the selection route on v[n, d] at every t of ts, on every layout, against the model
    (computed once per t)"""
    n, d = v.shape
    bufs = {layout: on_device(layout, v) for layout in layouts}
    for t in ts:
        want = TM.trimmed(v, t)
        for layout in layouts:
            got = run(dev, layout, bufs[layout], n, d, trim=t, **SEL)
            diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            print(f"{what}{layout} d={d} n={n} t={t}: {diff} of {d} outputs differ from the model")
            assert bits_equal(got, want), (layout, n, d, t)


# ------------------------------------------------------------ layouts and shapes ----
@pytest.mark.parametrize("n", ALL_N)
@pytest.mark.parametrize("d", ALL_D)
def test_selection_equals_the_model(dev, d, n):
    assert Plan(3, n, d, d, dense=True, trim=1, **SEL).route == R_SELECT_DENSE
    assert Plan(3, n, d, d, packed=True, trim=1, **SEL).route == R_SELECT_PACKED
    check(dev, np.ascontiguousarray(host_values()[:n, :d]), trims(n))


def test_the_cap_on_n(dev):
    n, d = 4096, 65
    check(dev, np.ascontiguousarray(host_values()[:n, :d]), trims(n))


def test_the_other_flat_algs_take_the_same_route(dev):
    n, d, t = 131, 33, 65
    v = np.ascontiguousarray(host_values()[:n, :d])
    want = TM.trimmed(v, t)
    for layout in LAYOUTS:
        buf = on_device(layout, v)
        for alg in (4, 5):
            assert bits_equal(run(dev, layout, buf, n, d, alg=alg, trim=t, **SEL), want)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,d", [(129, 257), (200, 65), (1000, 33)])
def test_selection_equals_the_list_kernel(dev, layout, n, d):
    v = np.ascontiguousarray(host_values()[:n, :d])
    buf = on_device(layout, v)
    for t in (1, 4, 5, 16, 17, 64):
        lst = run(dev, layout, buf, n, d, trim=t)
        got = run(dev, layout, buf, n, d, trim=t, **SEL)
        assert bits_equal(got, lst), (n, d, t)


@pytest.mark.parametrize("offset", [1, 2])
@pytest.mark.parametrize("n,d,t", [(131, 1101, 65), (257, 257, 128), (5, 64, 1), (1000, 65, 100), (2049, 9, 1024)])
def test_packed_base_off_16_bytes(dev, n, d, t, offset):
    """the base at 4 mod 16 and at 8 mod 16: the kernel's 4-byte loads take any"""
    v = np.ascontiguousarray(host_values()[:n, :d])
    got = run(dev, "packed", on_device("packed", v, offset=offset), n, d, trim=t, **SEL)
    assert bits_equal(got, TM.trimmed(v, t))


def test_bf16_rows_trim_on_the_unpacked_records(dev):
    import torch
    n, d, t = 131, 257, 65
    r = BM.pack(BM.values(np.random.default_rng(d + n), n, d, nans=True))
    v = BM.unpack(r, d)
    rows = torch.from_numpy(np.array(r, np.uint16).reshape(-1).view(np.int16)).cuda()
    assert Plan(3, n, d, d, bf16=True, trim=t, **SEL).route == R_SELECT_DENSE
    got = dev.aggregate(3, rows, n, d, d, bf16=True, trim=t, **SEL).cpu().numpy()
    assert dev.status() == 0
    assert BM.same_bits(got, TM.trimmed(v, t))


# ------------------------------------------------------------ constructed columns ----
def from_keys(keys):
    """the f32 values whose ord keys are `keys`"""
    k = np.asarray(keys, np.uint32)
    b = k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))
    return b.view(np.float32)


def decisive(n, t, rng):
    """[n, *] columns that decide the descent and the tie rule at (n, t).  No column lets two
    DIFFERENT NaN bit patterns survive the trim: which payload NaN + NaN propagates is left open
    by IEEE 754, and numpy on the host and the device's f32 add choose differently (0x7FFFFFFF
    and 0xFFFFFFFF kept in one column: the model's sum is 0x7FFFFFFF, the device's 0xFFFFFFFF,
    with the same clients kept) — outside the definition, which fixes the adds and their order.
    One NaN pattern surviving, alone or next to finite values, is covered."""
    big, one = np.float32(2.0 ** 24), np.float32(1)
    cols = []

    def add(col, orders=3):
        col = np.asarray(col, np.float32)
        assert col.shape == (n,)
        for _ in range(orders):
            cols.append(rng.permutation(col))

    add([np.float32(0.75)] * n, orders=1)                                   # all clients equal
    # ties straddling lo and hi, multiplicity larger than t: which copies stay changes the sum
    m = min(t + 3, n // 2)
    add([-big] * m + [big] * m + [one] * (n - 2 * m))
    add([one] * m + [big] * m + [np.float32(3)] * (n - 2 * m))
    add([one] * (n - m) + [big] * m)                                        # ties under lo and hi, a block above
    add([np.float32(-5)] + [np.float32(2.5)] * (n - 2) + [np.float32(9)])   # lo == hi, others around
    add([np.float32(2.5)] * (n - 1) + [np.float32(9)])
    add(rng.choice(np.array([0.0, -0.0], np.float32), n))                   # +-0.0 mixes
    add(np.concatenate([rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), n - 1), [-0.0]]))
    add([np.inf] * t + [-np.inf] * t + list(rng.normal(0, 1, n - 2 * t)))   # +-inf, all trimmed
    add([np.inf] * (t + 1) + [-np.inf] * t + list(rng.normal(0, 1, n - 2 * t - 1)))  # one +inf stays
    add(rng.choice(np.array([np.inf, -np.inf, 0.0, -0.0], np.float32), n))
    # NaNs of both signs, the two extreme keys among them: 0xFFFFFFFF is key 0, 0x7FFFFFFF key 0xFFFFFFFF
    lo_nan, hi_nan = from_keys([0])[0], from_keys([0xFFFFFFFF])[0]
    assert lo_nan.view(np.uint32) == 0xFFFFFFFF and hi_nan.view(np.uint32) == 0x7FFFFFFF
    k = max(1, t // 2)
    add([POS_NAN] * k + [NEG_NAN] * (t - k) + list(rng.normal(0, 1, n - t)))
    add([hi_nan] * k + [lo_nan] * (t - k) + list(rng.normal(0, 1, n - t)))
    add([hi_nan] * t + [lo_nan] * t + list(rng.normal(0, 1, n - 2 * t)))    # both extremes, all trimmed
    add([hi_nan] * (t + 1) + [lo_nan] * t + list(rng.normal(0, 1, n - 2 * t - 1)))  # key 0xFFFFFFFF is hi
    add([hi_nan] * t + [lo_nan] * (t + 1) + list(rng.normal(0, 1, n - 2 * t - 1)))  # key 0 is lo
    add([lo_nan] * n, orders=1)
    add([hi_nan] * n, orders=1)
    add([lo_nan] * t + [hi_nan] * (n - t))                                  # both keys, one pattern survives
    # two keys that differ in exactly one bit, for each of the 32 positions: the descent's round
    # for that bit decides; the split puts either key at the thresholds
    for b in range(32):
        while True:
            base = np.uint32(rng.integers(0, 1 << 32, dtype=np.uint64)) & ~np.uint32(1 << b)
            if not np.isnan(from_keys([base, base | np.uint32(1 << b)])).all():
                break  # (two different NaNs would both survive: see the docstring)
        for na in (t - 1, t, t + 1, n - t - 1, n - t, n - t + 1, n // 2):
            na = min(max(na, 1), n - 1)
            keys = np.array([base] * na + [base | np.uint32(1 << b)] * (n - na), np.uint32)
            cols.append(rng.permutation(from_keys(keys)))
    # an outlier of 1e30 at every client position
    body = rng.normal(0, 1, (n, n)).astype(np.float32)
    body[np.arange(n), np.arange(n)] = np.float32(1e30)
    v = np.concatenate([np.stack(cols, axis=1), body], axis=1)
    return np.ascontiguousarray(v, np.float32)


@pytest.mark.parametrize("n", [131, 257])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_constructed_columns(dev, layout, n):
    for t in (1, 65, n // 10, (n - 1) // 2):
        rng = np.random.default_rng(n * 1000 + t)
        v = decisive(n, t, rng)
        if v.shape[1] % 2 == 0:  # odd d: the packed padding float is in play
            v = np.ascontiguousarray(v[:, :-1])
        want = TM.trimmed(v, t)
        got = run(dev, layout, on_device(layout, v), n, v.shape[1], trim=t, **SEL)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        for j in np.flatnonzero(got.view(np.uint32) != want.view(np.uint32)):
            print(f"{layout} n={n} t={t} column {j}: got {got.view(np.uint32)[j]:#010x}, model "
                  f"{want.view(np.uint32)[j]:#010x}; distinct bit patterns in the column: "
                  f"{[hex(b) for b in np.unique(v[:, j].view(np.uint32))][:6]}")
        assert bits_equal(got, want), (n, t)
        # the tie rule matters on these columns: keeping the last copies instead changes bits
        if n - 2 * t >= 3:
            assert not bits_equal(TM.trimmed(v[::-1], t), want)
        # the list route's own constructed columns too
        v2, nan_survives = constructed(n, t, rng)
        got2 = run(dev, layout, on_device(layout, v2), n, v2.shape[1], trim=t, **SEL)
        assert np.array_equal(np.isnan(got2), nan_survives)
        assert bits_equal(got2, TM.trimmed(v2, t))


# ---------------------------------------------------------------------- options ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,d", [(6, 257), (131, 1101)])
def test_both_flags_with_t_zero_are_the_call_without_them(dev, layout, n, d):
    v = np.ascontiguousarray(host_values()[:n, :d])
    buf = on_device(layout, v)
    plain = run(dev, layout, buf, n, d)
    assert bits_equal(run(dev, layout, buf, n, d, trim=0, **SEL), plain)
    assert bits_equal(plain, TM.trimmed(v, 0))
    assert not bits_equal(run(dev, layout, buf, n, d, trim=1, **SEL), plain)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,d,t", [(6, 257, 1), (6, 1026, 2), (140, 257, 66)])
def test_clip_is_applied_before_ranking(dev, layout, n, d, t):
    _, val, _ = general(n, d, d, True)
    v = val.reshape(n, d)
    want = TM.trimmed(v, t, clip=GENERAL_CLIPPING)
    got = run(dev, layout, on_device(layout, v), n, d, trim=t, clip=True, clipping=GENERAL_CLIPPING, **SEL)
    assert bits_equal(got, want)
    assert not bits_equal(want, TM.trimmed(v, t))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("n,t", [(7, 2), (133, 65)])
def test_unaveraged_options(dev, layout, clip, n, t):
    d = 257
    _, val, _ = general(n, d, d, True)
    v = val.reshape(n, d)
    buf = on_device(layout, v)
    more = dict(clip=True, clipping=GENERAL_CLIPPING, **SEL) if clip else dict(SEL)
    c = GENERAL_CLIPPING if clip else None
    prev = np.random.default_rng(3).normal(0, 1, d).astype(np.float32)
    assert bits_equal(run(dev, layout, buf, n, d, trim=t, prev=prev, accumulate=True, **more),
                      TM.trimmed(v, t, clip=c, prev=prev))
    assert bits_equal(run(dev, layout, buf, n, d, trim=t, prev=prev, accumulate=True, n_avg=9, no_average=True, **more),
                      TM.trimmed(v, t, clip=c, prev=prev))
    assert bits_equal(run(dev, layout, buf, n, d, trim=t, no_average=True, **more),
                      TM.trimmed(v, t, clip=c, no_average=True))
    assert bits_equal(run(dev, layout, buf, n, d, trim=t, n_avg=9, **more), TM.trimmed(v, t, clip=c, n_avg=9))
    assert bits_equal(run(dev, layout, buf, n, d, trim=t, **more), TM.trimmed(v, t, clip=c))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_avg", [0, 9])
def test_dp_noise_is_the_list_routes(dev, layout, n_avg):
    """the same seed: the same noise, the trimmed divisor — bit for bit the list route's call"""
    n, d, t = 131, 257, 64
    _, val, _ = general(n, d, d, True)
    v = val.reshape(n, d)
    buf = on_device(layout, v)
    kw = dict(seed=SEED, clip=True, clipping=GENERAL_CLIPPING, n_avg=n_avg, sigma=1.12, trim=t)
    base = run(dev, layout, buf, n, d, **kw, **SEL)
    assert bits_equal(base, TM.trimmed(v, t, clip=GENERAL_CLIPPING, n_avg=n_avg))
    lst = run(dev, layout, buf, n, d, dp=True, **kw)
    got = run(dev, layout, buf, n, d, dp=True, **kw, **SEL)
    assert bits_equal(got, lst) and not bits_equal(got, base)


# ------------------------------------------------------------- status, scratch ----
@pytest.mark.parametrize("n,d,t", [(5, 257, 1), (131, 65, 65), (1000, 33, 499)])
def test_a_record_out_of_position_sets_the_status(dev, n, d, t):
    import torch

    from fltee import device as D
    v = np.ascontiguousarray(host_values()[:n, :d])
    idx = np.tile(np.arange(d, dtype=np.uint32), n)
    assert run(dev, "records", torch.from_numpy(D.pack_records(idx, v.reshape(-1))).cuda(), n, d, trim=t, **SEL) is not None
    idx[(n - 1) * d + d // 2] += 1
    rec = torch.from_numpy(D.pack_records(idx, v.reshape(-1))).cuda()
    run(dev, "records", rec, n, d, trim=t, want_status=DENSE_ORDER, **SEL)  # ... and the call returned


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kw", [{}, dict(clip=True, clipping=0.5)], ids=["plain", "clip"])
def test_a_reserved_call_grows_no_scratch(dev, layout, kw):
    import torch

    from fltee import _lib as L
    n, d, t = 131, 1101, 65
    v = np.ascontiguousarray(host_values()[:n, :d])
    buf = on_device(layout, v)
    lay = dict(packed=True) if layout == "packed" else dict(dense=True)
    L.lib().fltee_debug_scratch_release()
    L.lib().fltee_debug_scratch_grown()
    dev.reserve(3, n, d, d, trim=t, **lay, **kw, **SEL)
    assert bool(L.lib().fltee_debug_scratch_grown()) == bool(dev.workspace_bytes(3, n, d, d, trim=t, **lay, **kw, **SEL))
    run(dev, layout, buf, n, d, trim=t, **kw, **SEL)
    torch.cuda.synchronize()
    assert L.lib().fltee_debug_scratch_grown() == 0


def test_refusals_launch_nothing_and_leave_out_alone(dev):
    import torch

    from fltee import _lib as L
    from test_gpu_oblivious import traced
    buf = torch.zeros(4097 * 8, dtype=torch.int64, device="cuda")
    out = torch.full((64,), 7.5, dtype=torch.float32, device="cuda")
    cases = [(3, 4097, 8, 8, dict(dense=True, trim=100, **SEL)), (3, 130, 8, 8, dict(dense=True, trim=65, **SEL)),
             (3, 200, 8, 8, dict(dense=True, trim=2 ** 63, **SEL)), (1, 200, 8, 8, dict(dense=True, trim=70, **SEL)),
             (4, 200, 8, 64, dict(trim=70, **SEL)), (5, 200, 8, 8, dict(dense=True, oram_tree=True, trim=70, **SEL)),
             (3, 200, 8, 8, dict(dense=True, **SEL)), (3, 200, 8, 8, dict(packed=True, **SEL)),
             (3, 200, 8, 8, dict(dense=True, trim=65))]

    def calls():
        for alg, n, k, d, kw in cases:
            o = dev.opts(**kw)
            st = L.lib().fltee_aggregate_device(alg, ctypes.c_void_p(buf.data_ptr()), n, k, d,
                                                ctypes.c_void_p(out.data_ptr()), ctypes.byref(o), None)
            assert st == L.ERROR_INVALID_PARAMETER, (alg, n, k, d, kw)

    tr = traced(calls)
    assert not any(line.startswith("launch") for line in tr), tr
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == np.float32(7.5)).all()
