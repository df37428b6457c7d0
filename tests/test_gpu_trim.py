"""FLTEE_OPT_TRIM on the device (k_trim.hip) against tests/trim_model.py, bit for bit: both
layouts over the W tails and odd d (the packed padding float a NaN), n on both sides of every
batch of 8 and 16 clients in flight, t in {0, 1, 2, the median} and FLTEE_TRIM_MAX — every
list capacity (4, 16, 64); packed bases off 16 bytes; constructed columns on which the tie rule,
signed zeros, infinities and NaNs decide; the options; the status word; and a reserved call
growing no scratch."""
import functools

import numpy as np
import pytest

import packed_model as PM
import trim_model as TM
from conftest import gpu_available
from options_model import GENERAL_CLIPPING, general
from stable_model import bits_equal

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

ALL_D = [2, 3, 63, 64, 65, 257, 1101]
ALL_N = [3, 16, 17, 33, 65, 100, 129]
LAYOUTS = ["records", "packed"]
SEED = 0x5EED0001F00D
DENSE_ORDER = 0x1
POS_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]


def trims(n):
    ts = {0, 1, 2, (n - 1) // 2}
    if n == 129:
        ts.add(64)
    return sorted(t for t in ts if 2 * t < n)


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@functools.lru_cache(maxsize=None)
def host_values():
    """129 clients x 1101 finite values, half of them on a coarse grid (ties in every column):
    built once, never modified"""
    rng = np.random.default_rng(1101)
    v = rng.integers(-4, 5, (129, 1101)).astype(np.float32) * np.float32(0.5)
    v = np.where(rng.random(v.shape) < 0.5, rng.normal(0, 100, v.shape).astype(np.float32), v)
    v = np.ascontiguousarray(v, np.float32)
    v.setflags(write=False)
    return v


def on_device(layout, values, offset=0):
    """the n uploads as the layout's device buffer; packed: the padding float is a NaN and the
    base sits `offset` floats into a 16-byte aligned buffer"""
    import torch

    from fltee import device as D
    n, d = values.shape
    if layout == "records":
        idx = np.tile(np.arange(d, dtype=np.uint32), n)
        return torch.from_numpy(D.pack_records(idx, values.reshape(-1))).cuda()
    rows = PM.pack(values, np.nan)
    buf = torch.zeros(rows.size + 4, dtype=torch.float32, device="cuda")
    t = buf[offset:offset + rows.size]
    t.copy_(torch.from_numpy(rows.reshape(-1)))
    assert t.data_ptr() % 16 == (4 * offset) % 16
    return t


def run(dev, layout, buf, n, d, alg=3, prev=None, want_status=0, **kw):
    import torch
    out = None if prev is None else torch.from_numpy(prev.copy()).cuda()
    kw.update(packed=True) if layout == "packed" else kw.update(dense=True)
    got = dev.aggregate(alg, buf, n, d, d, out=out, **kw).cpu().numpy()
    assert dev.status() == want_status
    return got


# ------------------------------------------------------------ layouts and shapes ----
@pytest.mark.parametrize("d", ALL_D)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_trimmed_mean_equals_the_model(dev, layout, d):
    for n in ALL_N:
        v = np.ascontiguousarray(host_values()[:n, :d])
        buf = on_device(layout, v)
        for t in trims(n):
            want = TM.trimmed(v, t)
            got = run(dev, layout, buf, n, d, trim=t)
            diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            print(f"{layout} d={d} n={n} t={t}: {diff} of {d} outputs differ from the model")
            assert bits_equal(got, want), (n, t)
            if n == 17 and t == 2:  # the other flat algs take the same route
                for alg in (4, 5):
                    assert bits_equal(run(dev, layout, buf, n, d, alg=alg, trim=t), want)


@pytest.mark.parametrize("offset", [1, 2])
@pytest.mark.parametrize("n,d,t", [(17, 1101, 2), (33, 257, 16), (5, 64, 1), (129, 65, 64)])
def test_packed_base_off_16_bytes(dev, n, d, t, offset):
    """the base at 4 mod 16 (4-byte loads) and at 8 mod 16 (8-byte loads)"""
    v = np.ascontiguousarray(host_values()[:n, :d])
    got = run(dev, "packed", on_device("packed", v, offset=offset), n, d, trim=t)
    assert bits_equal(got, TM.trimmed(v, t))


def test_the_large_d_launch_shape(dev):
    """past the small-d threshold (2^18): 256-lane blocks, 16-byte loads, a d tail"""
    n, d, t = 5, (1 << 18) + 7, 1
    v = np.random.default_rng(7).normal(0, 1, (n, d)).astype(np.float32)
    for layout in LAYOUTS:
        assert bits_equal(run(dev, layout, on_device(layout, v), n, d, trim=t), TM.trimmed(v, t))


# ------------------------------------------------------------ constructed columns ----
def constructed(n, t, rng):
    """[n, 11 * 6 + 1] columns on which the definition's corners decide, each construct under
    six random upload orders; and whether a NaN must survive in a column"""
    big, one = np.float32(2.0 ** 24), np.float32(1)
    free = n - 2 * (t + 1)
    cols, nan_survives = [], []

    def add(col, nan=False):
        for _ in range(6):
            cols.append(rng.permutation(np.asarray(col, np.float32)))
            nan_survives.append(nan)

    add([np.float32(0.75)] * n)                                           # all clients equal
    if free >= 1:  # exactly t + 1 copies of the minimum and of the maximum: which copy stays
        add([-big] * (t + 1) + [big] * (t + 1) + [one] * free)            # changes the in-order sum
        add([one] * (t + 1) + [big] * (t + 1) + [np.float32(3)] * free)
    else:
        add([one] * n), add([big] * n)
    add([np.float32(-5)] + [np.float32(2.5)] * (n - 2) + [np.float32(9)])  # lo == hi, others around
    add([np.float32(2.5)] * (n - 1) + [np.float32(9)])
    add(rng.choice(np.array([0.0, -0.0], np.float32), n))                 # +-0.0 mixes
    add(np.concatenate([rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), n - 1), [-0.0]]))
    add([np.inf] * t + [-np.inf] * t + list(rng.normal(0, 1, n - 2 * t)))  # +-inf, all trimmed
    add([np.inf] * (t + 1) + [-np.inf] * t + list(rng.normal(0, 1, n - 2 * t - 1)))  # one +inf stays
    # NaNs of both signs in up to t clients: every one is an extreme, the output NaN-free
    k = max(1, t // 2)
    add([POS_NAN] * k + [NEG_NAN] * (t - k) + list(rng.normal(0, 1, n - t)))
    # a NaN in t + 1 clients: one survives
    add([POS_NAN] * (t + 1) + list(rng.normal(0, 1, n - t - 1)), nan=True)
    cols.append(np.full(n, 0.5, np.float32))
    nan_survives.append(False)
    return np.ascontiguousarray(np.stack(cols, axis=1), np.float32), np.array(nan_survives)


@pytest.mark.parametrize("n,t", [(5, 1), (9, 2), (17, 1), (17, 4), (17, 8), (33, 5), (33, 16), (129, 17), (129, 64)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_constructed_columns(dev, layout, n, t):
    v, nan_survives = constructed(n, t, np.random.default_rng(n * 1000 + t))
    d = v.shape[1]
    assert d % 2 == 1
    want = TM.trimmed(v, t)
    assert np.array_equal(np.isnan(want), nan_survives)
    got = run(dev, layout, on_device(layout, v), n, d, trim=t)
    assert np.array_equal(np.isnan(got), nan_survives)
    assert bits_equal(got, want)
    # the tie rule matters on these columns: keeping the last copies instead changes bits
    flipped = TM.trimmed(v[::-1], t)
    if n - 2 * (t + 1) >= 2:
        assert not bits_equal(flipped, want)


# ---------------------------------------------------------------------- options ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,d", [(6, 257), (17, 1101)])
def test_the_flag_with_t_zero_is_the_call_without_it(dev, layout, n, d):
    v = np.ascontiguousarray(host_values()[:n, :d])
    buf = on_device(layout, v)
    plain = run(dev, layout, buf, n, d)
    assert bits_equal(run(dev, layout, buf, n, d, trim=0), plain)
    assert bits_equal(plain, TM.trimmed(v, 0)) and bits_equal(plain, PM.inorder_mean(v))
    assert not bits_equal(run(dev, layout, buf, n, d, trim=1), plain)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,d,t", [(6, 257, 1), (6, 1026, 2)])
def test_clip_is_applied_before_ranking(dev, layout, n, d, t):
    _, val, _ = general(n, d, d, True)
    v = val.reshape(n, d)
    want = TM.trimmed(v, t, clip=GENERAL_CLIPPING)
    got = run(dev, layout, on_device(layout, v), n, d, trim=t, clip=True, clipping=GENERAL_CLIPPING)
    assert bits_equal(got, want)
    # ranking the raw values and clipping afterwards keeps other clients: not the same result
    from options_model import clip_coefs
    clipped = clip_coefs(val, n, d, GENERAL_CLIPPING)[1].reshape(n, d)
    keep_raw = TM.kept(v, t)
    assert (keep_raw != TM.kept(clipped, t)).any()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
def test_unaveraged_options(dev, layout, clip):
    n, d, t = 7, 257, 2
    _, val, _ = general(n, d, d, True)
    v = val.reshape(n, d)
    buf = on_device(layout, v)
    more = dict(clip=True, clipping=GENERAL_CLIPPING) if clip else {}
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
def test_dp_noise_takes_the_trimmed_divisor(dev, oracle, layout, n_avg):
    n, d, t = 7, 257, 2
    _, val, _ = general(n, d, d, True)
    v = val.reshape(n, d)
    buf = on_device(layout, v)
    kw = dict(seed=SEED, clip=True, clipping=GENERAL_CLIPPING, n_avg=n_avg, sigma=1.12, trim=t)
    base = run(dev, layout, buf, n, d, **kw)
    assert bits_equal(base, TM.trimmed(v, t, clip=GENERAL_CLIPPING, n_avg=n_avg))
    got = run(dev, layout, buf, n, d, dp=True, **kw)
    div = n_avg if n_avg else n - 2 * t
    noise = oracle.dp_noise(np.zeros(d, np.float32), 1.12, GENERAL_CLIPPING, div, seed=SEED)
    assert noise.any()
    assert bits_equal(got, base + noise)


# ------------------------------------------------------------- status, scratch ----
@pytest.mark.parametrize("n,d,t", [(5, 257, 1), (33, 65, 16), (129, 64, 64)])
def test_a_record_out_of_position_sets_the_status(dev, n, d, t):
    import torch

    from fltee import device as D
    v = np.ascontiguousarray(host_values()[:n, :d])
    idx = np.tile(np.arange(d, dtype=np.uint32), n)
    assert run(dev, "records", torch.from_numpy(D.pack_records(idx, v.reshape(-1))).cuda(), n, d, trim=t) is not None
    idx[(n - 1) * d + d // 2] += 1
    rec = torch.from_numpy(D.pack_records(idx, v.reshape(-1))).cuda()
    run(dev, "records", rec, n, d, trim=t, want_status=DENSE_ORDER)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kw", [{}, dict(clip=True, clipping=0.5)], ids=["plain", "clip"])
def test_a_reserved_trimmed_call_grows_no_scratch(dev, layout, kw):
    import torch

    from fltee import _lib as L
    n, d, t = 17, 1101, 3
    v = np.ascontiguousarray(host_values()[:n, :d])
    buf = on_device(layout, v)
    lay = dict(packed=True) if layout == "packed" else dict(dense=True)
    L.lib().fltee_debug_scratch_release()
    L.lib().fltee_debug_scratch_grown()
    dev.reserve(3, n, d, d, trim=t, **lay, **kw)
    assert bool(L.lib().fltee_debug_scratch_grown()) == bool(dev.workspace_bytes(3, n, d, d, trim=t, **lay, **kw))
    run(dev, layout, buf, n, d, trim=t, **kw)
    torch.cuda.synchronize()
    assert L.lib().fltee_debug_scratch_grown() == 0


def test_refusals_on_the_device(dev):
    import ctypes

    import torch

    from fltee import _lib as L
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    out = torch.zeros(64, dtype=torch.float32, device="cuda")
    for alg, n, k, d, kw in [(3, 4, 64, 64, dict(dense=True, trim=2)), (3, 200, 8, 8, dict(dense=True, trim=65)),
                             (1, 5, 64, 64, dict(dense=True, trim=1)), (4, 5, 8, 64, dict(trim=1)),
                             (5, 5, 64, 64, dict(dense=True, oram_tree=True, trim=1))]:
        o = dev.opts(**kw)
        st = L.lib().fltee_aggregate_device(alg, ctypes.c_void_p(buf.data_ptr()), n, k, d,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.byref(o), None)
        assert st == L.ERROR_INVALID_PARAMETER
