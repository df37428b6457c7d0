"""Obliviousness of aggregation_alg 7's launch trace (the approach and helpers of
tests/test_gpu_oblivious.py): for uploads of the same public sizes — random, one client
repeating one index k times, every record on one index — every launch (site, grid, block,
LDS), copy, memset, sync and accounted byte count of the stable network (k_stable.hip) and
of the shared fold / compaction tail is the same, line for line."""
import pytest

from conftest import gpu_available
from test_gpu_oblivious import KINDS, _device_traces, assert_same_trace

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

ALG_BUBBLE = 7


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@pytest.mark.parametrize("n,d,k", [(30, 5000, 500),      # fused fold + compaction
                                   (400, 20000, 1000)])  # streaming fold + patch
def test_alg7_trace_is_data_independent(dev, n, d, k):
    tr = _device_traces(dev, ALG_BUBBLE, n, d, k, KINDS)
    assert any("stable_tile_sort_kernel" in line for line in tr[0]), "the stable network did not run"
    for t, kind in zip(tr[1:], KINDS[1:]):
        assert_same_trace(tr[0], t, f"alg 7 n={n} d={d} k={k} {kind}")
