"""aggregation_alg 7 through the device API against its model (tests/stable_model.py),
bit for bit: records ++ (i, 0.0) in stable order by idx, each run left-folded in float32
with the zero entry last — the in-order client sum out of the oblivious stable network
(k_stable.hip) and advanced's fold / compaction / extract.

Shapes: the smallest, a non-power-of-two one, advanced's fused fold-compaction, its
streaming fold and patch, and configs[0]'s.  Each shape's uploads and models are built
once (module cache) and left unchanged."""
import functools
import zlib

import numpy as np
import pytest

from conftest import gpu_available
from stable_model import bits_equal, distinct_indices, model, order_sensitive, run_sums

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SHAPES = [(1, 1, 1), (3, 5, 17), (30, 500, 5000), (400, 1000, 20000), (30, 5089, 50890)]
ALG_ADVANCED, ALG_BUBBLE = 1, 7


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


def cuda_records(dev, idx, val):
    import torch
    return torch.from_numpy(dev.pack_records(idx, val)).cuda()


@functools.lru_cache(maxsize=None)
def upload(kind, n, k, d):
    rng = np.random.default_rng(zlib.crc32(repr((kind, n, k, d)).encode()))
    if kind == "random":
        idx = distinct_indices(rng, n, k, d)
        val = rng.normal(0, 0.01, n * k).astype(np.float32)
    elif kind == "order":
        idx, val = order_sensitive(n, k, d)
    elif kind == "same_indices":            # every client sends the same k indices
        idx = np.tile(rng.choice(d, k, replace=False).astype(np.uint32), n)
        val = rng.normal(0, 0.01, n * k).astype(np.float32)
    elif kind == "out_of_range":            # some records with idx in [d, 2^31): ignored
        idx = distinct_indices(rng, n, k, d)
        val = rng.normal(0, 0.01, n * k).astype(np.float32)
        far = rng.random(n * k) < 0.25
        idx[far] = rng.integers(d, 2 ** 31, int(far.sum())).astype(np.uint32)
        idx[-1] = 2 ** 31 - 1
        idx[0] = d
    elif kind == "repeat_int":              # client 0 repeats one index k times: small
        idx = distinct_indices(rng, n, k, d)   # integers are exact under any association
        idx[:k] = idx[0]
        val = rng.integers(-8, 9, n * k).astype(np.float32)
    elif kind == "repeat_normal":           # the same with N(0, 0.01) values
        idx = distinct_indices(rng, n, k, d)
        idx[:k] = idx[0]
        val = rng.normal(0, 0.01, n * k).astype(np.float32)
    else:
        raise AssertionError(kind)
    idx.setflags(write=False)
    val.setflags(write=False)
    return idx, val, model(idx, val, n, d)


def run7(dev, idx, val, n, k, d, **kw):
    out = dev.aggregate(ALG_BUBBLE, cuda_records(dev, idx, val), n, k, d, **kw).cpu().numpy()
    assert dev.status() == 0
    return out


@pytest.mark.parametrize("n,k,d", SHAPES)
@pytest.mark.parametrize("kind", ["random", "same_indices", "out_of_range", "repeat_int"])
def test_alg7_equals_the_model(dev, kind, n, k, d):
    idx, val, ref = upload(kind, n, k, d)
    assert bits_equal(run7(dev, idx, val, n, k, d), ref)


@pytest.mark.parametrize("n,k,d", SHAPES)
def test_alg7_repeated_index_exact_with_a_full_halo(dev, n, k, d):
    # one walk of the whole array: every run bit for bit, whatever its length
    idx, val, ref = upload("repeat_normal", n, k, d)
    assert bits_equal(run7(dev, idx, val, n, k, d, fold_halo=n * k + d), ref)


@pytest.mark.parametrize("n,k,d", SHAPES)
def test_alg7_keeps_the_upload_order_where_advanced_does_not(dev, n, k, d):
    """On the order-sensitive input alg 7 is the in-order sum; advanced (the bitonic
    network's tie order) is another float32 value in at least one parameter — wherever an
    index has more than one record (with n = 1 a run is one value and its zero entry, one
    sum whatever the order: nothing to tell apart)."""
    idx, val, ref = upload("order", n, k, d)
    out = run7(dev, idx, val, n, k, d)
    adv = dev.aggregate(ALG_ADVANCED, cuda_records(dev, idx, val), n, k, d).cpu().numpy()
    assert dev.status() == 0
    diff = int((out.view(np.uint32) != adv.view(np.uint32)).sum())
    print(f"alg 7 vs advanced on the order-sensitive input ({n}, {k}, {d}): {diff} of {d} differ")
    assert bits_equal(out, ref)
    if n > 1:
        assert diff > 0, "the input does not show the order: fix the input"


@pytest.mark.parametrize("n,k,d", [(3, 5, 17), (30, 500, 5000)])
def test_alg7_accumulate_and_no_average(dev, n, k, d):
    import torch
    idx, val, _ = upload("random", n, k, d)
    sums = run_sums(idx, val, d)
    assert bits_equal(run7(dev, idx, val, n, k, d, no_average=True), sums)
    assert bits_equal(run7(dev, idx, val, n, k, d, n_avg=7),
                      sums * (np.float32(1) / np.float32(7)))
    prev = np.random.default_rng(9).normal(0, 1, d).astype(np.float32)
    acc = torch.from_numpy(prev.copy()).cuda()
    dev.aggregate(ALG_BUBBLE, cuda_records(dev, idx, val), n, k, d, out=acc, accumulate=True)
    assert dev.status() == 0
    assert bits_equal(acc.cpu().numpy(), prev + sums)


def test_alg7_refuses_another_k_req(dev):
    from fltee import _lib as L
    n, k, d = 3, 5, 17
    idx, val, ref = upload("random", n, k, d)
    rec = cuda_records(dev, idx, val)
    for k_req in (0, 4, 6):
        with pytest.raises(RuntimeError, match=hex(L.ERROR_INVALID_PARAMETER)):
            dev.aggregate(ALG_BUBBLE, rec, n, k, d, k_req=k_req)
    assert bits_equal(dev.aggregate(ALG_BUBBLE, rec, n, k, d, k_req=k).cpu().numpy(), ref)
    assert dev.status() == 0


def test_alg7_refuses_a_shape_past_the_size_limit_before_reserving(dev):
    """next_pow2(n * k + d) > 2^29: INVALID_PARAMETER before any scratch is reserved.  The
    scratch of this shape would be >= 2^30 x (16 + 8 + 8) bytes = 32 GiB; the device's free
    memory must not move by anything near that (1 GiB allowed for other users of a
    shared device)."""
    import torch

    from fltee import _lib as L
    n, k, d = 1, 1, (1 << 29) + 1
    assert dev.workspace_bytes(ALG_BUBBLE, n, k, d) >= (1 << 30) * 32
    rec = torch.zeros(n * k, dtype=torch.int64, device="cuda")
    out = torch.zeros(16, dtype=torch.float32, device="cuda")  # never written: refused first
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    with pytest.raises(RuntimeError, match=hex(L.ERROR_INVALID_PARAMETER)):
        dev.aggregate(ALG_BUBBLE, rec, n, k, d, out=out)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (1 << 30)
    assert dev.status() == 0 and not out.cpu().numpy().any()
