"""The stable oblivious network of aggregation_alg 7 alone (k_stable.hip through
fltee_stable_sort_device): 16-byte records {u64 key; f32 val; u32 pad} in place, ascending
by key, payloads attached, bit for bit against np.sort — for every m = 2^1 .. 2^21 (every
boundary between the LDS tile kernel, the register passes of 1..4 steps and the LDS merge
kernel), keys that differ only in the position word, the extreme keys, and a tail of
identical pads."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

REC = np.dtype([("key", "<u8"), ("val", "<u4"), ("pad", "<u4")])
PAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


def gpu_sort(dev, rec):
    import torch
    t = torch.from_numpy(rec.view(np.int64).copy()).cuda()
    dev.stable_sort(t)
    torch.cuda.synchronize()
    return t.cpu().numpy().view(REC)


def expect(rec):
    return rec[np.argsort(rec["key"], kind="stable")]


def distinct_keys(rng, m):
    # distinct with certainty: a random high part over a permutation in the low 21 bits
    hi = rng.integers(0, 2 ** 42, m, dtype=np.uint64) << np.uint64(21)
    return hi | rng.permutation(m).astype(np.uint64)


def payload(rng, rec):
    rec["val"] = rng.integers(0, 2 ** 32, len(rec), dtype=np.uint64).astype(np.uint32)
    rec["pad"] = rng.integers(0, 2 ** 32, len(rec), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("mlog", range(1, 22))
def test_sorts_random_distinct_keys(dev, mlog):
    m = 1 << mlog
    rng = np.random.default_rng(mlog)
    rec = np.zeros(m, REC)
    rec["key"] = distinct_keys(rng, m)
    payload(rng, rec)
    got = gpu_sort(dev, rec)
    assert got.tobytes() == expect(rec).tobytes()


@pytest.mark.parametrize("mlog", [12, 17])
def test_keys_differing_only_in_position(dev, mlog):
    m = 1 << mlog
    rng = np.random.default_rng(100 + mlog)
    rec = np.zeros(m, REC)
    rec["key"] = (np.uint64(77) << np.uint64(32)) | rng.permutation(m).astype(np.uint64)
    payload(rng, rec)
    got = gpu_sort(dev, rec)
    assert got.tobytes() == expect(rec).tobytes()
    assert np.array_equal(got["key"] & np.uint64(0xFFFFFFFF), np.arange(m, dtype=np.uint64))


@pytest.mark.parametrize("mlog", [3, 12, 14])
def test_extreme_keys_and_a_tail_of_pads(dev, mlog):
    m = 1 << mlog
    rng = np.random.default_rng(200 + mlog)
    live = m - m // 3 - 1                       # the rest: identical pads (key ~0, +0.0)
    rec = np.zeros(m, REC)
    rec["key"][:live] = distinct_keys(rng, live)
    payload(rng, rec[:live])
    rec["key"][0] = 0
    rec["key"][live - 1] = PAD_KEY - np.uint64(1)
    rec["key"][live:] = PAD_KEY
    rec[:live] = rec[:live][rng.permutation(live)]
    got = gpu_sort(dev, rec)
    assert got.tobytes() == expect(rec).tobytes()
    assert got["key"][0] == 0 and got["key"][live - 1] == PAD_KEY - np.uint64(1)
    assert (got["key"][live:] == PAD_KEY).all() and (got["val"][live:] == 0).all()


def test_pads_may_start_anywhere(dev):
    # pads mixed among the records on the way in: all of them leave at the end
    m = 1 << 13
    rng = np.random.default_rng(300)
    rec = np.zeros(m, REC)
    rec["key"] = distinct_keys(rng, m)
    payload(rng, rec)
    where = rng.permutation(m)[: m // 2]
    rec["key"][where] = PAD_KEY
    rec["val"][where] = 0
    rec["pad"][where] = 0
    got = gpu_sort(dev, rec)
    assert got.tobytes() == expect(rec).tobytes()


@pytest.mark.parametrize("m", [3, 6, 4097, 3 << 12])
def test_rejects_a_length_that_is_no_power_of_two(dev, m):
    import torch

    from fltee import _lib as L
    t = torch.zeros(2 * m, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match=hex(L.ERROR_INVALID_PARAMETER)):
        dev.stable_sort(t)
