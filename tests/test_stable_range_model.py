"""aggregation_alg 7 by position range on the CPU: fltee.parallel.index_sharded_bubble — its
order of steps, its pairwise exchanges, its pad rule — with the numpy pieces of
tests/stable_range_np.py (the network from its definition) and tests/range_ops_np.py (the
fold and compaction) standing in for the HIP range pieces.

  * the network: for W in {1, 2, 4, 8} ranges of M in {2^13, 2^15} positions and a live
    length (records + zero entries) of M, M - 1, M/2 + 1 and M/2 + C/2 + 3, the ranges
    concatenated equal np.sort by key, and stripped they are bubble_sort_based's order
    (tests/stable_model.py: records ++ (i, 0.0), stable by idx), pads behind;
  * the aggregate: n = 64, k = 512, d = 600 with N(0, 0.01^2) values (every index has tens
    of entries, so runs cross the range boundaries) equals the in-order sum bit for bit;
  * two gloo processes (DistRanks: the ranges really travel) give the VirtualRanks result.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from stable_model import bits_equal, distinct_indices, model
from stable_range_np import PAD_KEY, NumpyStableRangeOps, init_range16, rec16
from test_parallel_gloo import free_port

from fltee import parallel as P


def network_case(M, valid):
    """nrec records and d zero entries, nrec + d = valid; some records with idx >= d"""
    rng = np.random.default_rng(M + valid)
    d = valid // 4
    nrec = valid - d
    idx = rng.integers(0, d + d // 8 + 1, nrec).astype(np.uint32)
    val = rng.normal(0, 0.01, nrec).astype(np.float32)
    return idx, val, d


@pytest.mark.parametrize("vkind", ["M", "M-1", "M/2+1", "M/2+C/2+3"])
@pytest.mark.parametrize("M", [1 << 13, 1 << 15])
@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_distributed_stable_network_sorts_by_key(W, M, vkind):
    C = M // W
    valid = {"M": M, "M-1": M - 1, "M/2+1": M // 2 + 1, "M/2+C/2+3": M // 2 + C // 2 + 3}[vkind]
    valid = min(valid, M)  # (W = 1: M/2 + C/2 + 3 is past the array)
    idx, val, d = network_case(M, valid)
    ops = NumpyStableRangeOps()
    chunks = {r: init_range16(idx, val, d, r * C, C) for r in range(W)}
    before = np.concatenate([rec16(chunks[r]) for r in range(W)])
    assert (before["key"] != PAD_KEY).sum() == valid
    out = P.distributed_stable_network(chunks, W, M, ops, P.VirtualRanks(W), valid=valid)
    got = np.concatenate([rec16(out[r]) for r in range(W)])
    want = before[np.argsort(before["key"], kind="stable")]
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    # stripped: bubble_sort_based's order, then the pads as (u32::MAX, +0.0)
    stripped = np.concatenate([ops.stable_strip(out[r]).numpy() for r in range(W)]).view(np.uint64)
    all_idx = np.concatenate([idx, np.arange(d, dtype=np.uint32)])
    all_val = np.concatenate([val, np.zeros(d, np.float32)])
    o = np.argsort(all_idx, kind="stable")
    ref = all_idx[o].astype(np.uint64) | (all_val[o].view(np.uint32).astype(np.uint64) << np.uint64(32))
    assert np.array_equal(stripped[:valid], ref)
    assert np.all(stripped[valid:] == np.uint64(0xFFFFFFFF))


N, K, D = 64, 512, 600


def aggregate_case():
    rng = np.random.default_rng(64512600)
    idx = distinct_indices(rng, N, K, D)
    val = rng.normal(0, 0.01, N * K).astype(np.float32)
    return idx, val


def sharded(idx, val, W, comm=None, ranks=None):
    M = 1 << (N * K + D - 1).bit_length()
    C = M // W
    chunks = {r: init_range16(idx, val, D, r * C, C) for r in (range(W) if ranks is None else ranks)}
    return P.index_sharded_bubble(chunks, W, M, N, K, D, ops=NumpyStableRangeOps(), comm=comm)


@pytest.fixture(scope="module")
def reference():
    idx, val = aggregate_case()
    ref = model(idx, val, N, D)
    ref.setflags(write=False)
    return idx, val, ref


@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_index_sharded_bubble_is_the_in_order_sum(reference, W):
    idx, val, ref = reference
    counts = np.bincount(idx, minlength=D)
    assert counts.min() >= 20                       # tens of entries per index
    M = 1 << (N * K + D - 1).bit_length()
    if W > 1:                                       # runs cross the range boundaries
        order = np.sort(np.concatenate([idx, np.arange(D, dtype=np.uint32)]), kind="stable")
        assert all(order[b - 1] == order[b] for b in range(M // W, N * K + D, M // W))
    out = sharded(idx, val, W)
    assert bits_equal(out.numpy(), ref)


def worker(rank, world, port, outdir):
    import sys
    for p in (ROOT, os.path.join(ROOT, "fl-tee_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    idx, val = aggregate_case()
    out = sharded(idx, val, world, comm=P.DistRanks(rank, world), ranks=[rank])
    if rank == 0:
        np.save(os.path.join(outdir, "bubble.npy"), out.numpy())
    else:
        assert out is None
    dist.barrier()
    dist.destroy_process_group()


def test_index_sharded_bubble_gloo_equals_virtual_ranks(reference, tmp_path):
    idx, val, ref = reference
    mp.spawn(worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    got = np.load(tmp_path / "bubble.npy")
    assert bits_equal(got, sharded(idx, val, 2).numpy())
    assert bits_equal(got, ref)
