"""Steady-state calls allocate nothing: for the smallest shape that reaches each
route of aggregate() (tests/test_plan.py ROUTES, whose routes and tails the CPU test pins),
the engine scratch is released, fltee_reserve sizes it from the shape plan, and two
aggregates then grow no scratch buffer (fltee_debug_scratch_grown stays 0) — the plan covers
every buffer the route touches.  The first result is checked against the alg's reference.
nips19 alone may grow ws_sel / ws_keys / ws_radix: its selected list is sized from a count
read back from the device."""
import ctypes

import numpy as np
import pytest

from conftest import gpu_available
from options_model import reference
from stable_model import bits_equal, distinct_indices
from test_plan import CLIPPED, ROUTES, WS

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

DATA_SIZED = sum(1 << WS.index(w) for w in ("sel", "keys", "radix"))


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


def upload(alg, n, k, d, dense):
    rng = np.random.default_rng(alg * 1000003 + n * 1009 + k * 31 + d)
    if dense:
        idx = np.tile(np.arange(d, dtype=np.uint32), n)
    else:
        idx = distinct_indices(rng, n, k, d)
    return idx, rng.normal(0, 0.01, n * k).astype(np.float32)


def reserved_run(dev, alg, rec, n, k, d, kw):
    """release -> reserve -> two aggregates; returns the first result and the growth mask"""
    import torch

    from fltee import _lib as L
    lib = L.lib()
    out = [torch.empty(d, dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    lib.fltee_debug_scratch_release()
    dev.reserve(alg, n, k, d, **kw)
    lib.fltee_debug_scratch_grown()
    for o in out:
        dev.aggregate(alg, rec, n, k, d, out=o, **kw)
    assert dev.status() == 0
    grown = lib.fltee_debug_scratch_grown()
    return out[0].cpu().numpy(), out[1].cpu().numpy(), grown


@pytest.mark.parametrize("case", ROUTES, ids=lambda c: c[0])
def test_reserved_shape_allocates_nothing(dev, oracle, case):
    import torch
    _, alg, n, k, d, kw, _, _ = case
    idx, val = upload(alg, n, k, d, kw.get("dense", False))
    rec = torch.from_numpy(dev.pack_records(idx, val)).cuda()
    first, second, grown = reserved_run(dev, alg, rec, n, k, d, kw)
    assert bits_equal(first, reference(oracle, alg, idx, val, n, k, d, kw))
    assert bits_equal(first, second)
    allowed = DATA_SIZED if alg == 2 else 0
    assert grown & ~allowed == 0, [w for i, w in enumerate(WS) if grown >> i & 1]


@pytest.mark.parametrize("case", CLIPPED, ids=lambda c: c[0])
def test_reserved_clipped_shape_allocates_nothing(dev, case):
    """FLTEE_OPT_CLIP: the coefficients and the clipped copy of the records are planned too.
    Reference: the clipped ordered sweep (baseline), the same in-order sum of the same clipped
    records (as tests/test_gpu_oram.py compares the clipped tree)."""
    import torch
    _, alg, n, k, d, kw, _, _ = case
    idx, val = upload(alg, n, k, d, False)
    val *= 100  # norms well past the clip bound
    rec = torch.from_numpy(dev.pack_records(idx, val)).cuda()
    want = dev.aggregate(3, rec, n, k, d, clip=True, clipping=kw["clipping"]).cpu().numpy()
    plain = dev.aggregate(3, rec, n, k, d).cpu().numpy()
    assert dev.status() == 0 and not bits_equal(want, plain)
    first, second, grown = reserved_run(dev, alg, rec, n, k, d, kw)
    assert bits_equal(first, want) and bits_equal(first, second)
    assert grown == 0, [w for i, w in enumerate(WS) if grown >> i & 1]


def test_unknown_alg_is_refused_before_anything_is_launched(dev):
    """An unknown alg with FLTEE_OPT_CLIP: 0x2 from the plan, before the clip kernels — the
    launch trace stays empty.  (The call brings its own status word: fltee_aggregate_device
    clears the library's word, one memset, before it hands over to the engine.)"""
    import torch

    from fltee import _lib as L
    lib = L.lib()
    lib.fltee_debug_trace.argtypes = [ctypes.c_int]
    lib.fltee_debug_trace.restype = None
    lib.fltee_debug_trace_text.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    lib.fltee_debug_trace_text.restype = ctypes.c_size_t
    n, k, d = 4, 8, 100
    idx, val = upload(4, n, k, d, False)
    rec = torch.from_numpy(dev.pack_records(idx, val)).cuda()
    out = torch.zeros(d, dtype=torch.float32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    dev.aggregate(4, rec, n, k, d, out=out, clip=True, status=status)  # the device context exists
    out.zero_()
    torch.cuda.synchronize()
    lib.fltee_debug_trace(1)
    try:
        for alg in (0, 8):
            with pytest.raises(RuntimeError, match=hex(L.ERROR_INVALID_PARAMETER)):
                dev.aggregate(alg, rec, n, k, d, out=out, clip=True, status=status)
    finally:
        lib.fltee_debug_trace(0)
    assert lib.fltee_debug_trace_text(None, 0) == 0
    assert not out.cpu().numpy().any() and int(status.item()) == 0
