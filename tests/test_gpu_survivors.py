"""The survivors gather (k_survivors.hip, fltee_gather_clients_device) against numpy indexing:
out[s] = records[keep[s]] on n = 5 clients of k records.  k = 1 (8-byte records at odd
multiples of 8), 2, 129 (odd: slices whose addresses agree modulo 16 move as 16-byte vectors
with an 8-byte record in front or behind, the others as 8-byte records) and 4096 (several
16 KB chunks per slice); every keep set of the issue — all, the first dropped (every slice
shifts by one), the last dropped, every other, one, none (writes nothing, returns 0) — plus
a source view 8 bytes off a 16-byte boundary, and an index past n (clamped, reported with
FLTEE_DEV_ERR_LAUNCH, nothing read or written out of bounds)."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

N = 5
KS = [1, 2, 129, 4096]
KEEPS = [[0, 1, 2, 3, 4], [1, 2, 3, 4], [0, 1, 2, 3], [0, 2, 4], [3], []]
GUARD = 64  # records of sentinel on either side of the output
SENTINEL = -0x0123456789ABCDEF
DEV_ERR_LAUNCH = 0x80000000


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@pytest.fixture(scope="module")
def sources():
    """k -> the (N, k) records, every 8-byte record distinct; built once, never modified"""
    rng = np.random.default_rng(1234)
    return {k: rng.integers(-2 ** 62, 2 ** 62, (N, k), dtype=np.int64) for k in KS}


def run(dev, src_t, keep, k):
    """gather into the middle of a sentinel-filled buffer: (out rows, the guards untouched?)"""
    import torch
    buf = torch.full((GUARD + max(len(keep), 1) * k + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    out = buf[GUARD:GUARD + len(keep) * k].view(len(keep), k)
    got = dev.gather_clients(src_t, keep, out=out)
    assert got is out
    assert dev.status() == 0
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + len(keep) * k:] == SENTINEL).all(), \
        "the gather wrote outside its output"
    return host[GUARD:GUARD + len(keep) * k].reshape(len(keep), k)


@pytest.mark.parametrize("keep", KEEPS, ids=lambda s: "keep_" + ("".join(map(str, s)) or "none"))
@pytest.mark.parametrize("k", KS)
def test_gather_equals_numpy_indexing(dev, sources, k, keep):
    import torch
    src = sources[k]
    got = run(dev, torch.from_numpy(src).cuda(), keep, k)
    assert np.array_equal(got, src[keep].reshape(len(keep), k))


@pytest.mark.parametrize("k", [2, 129])
def test_gather_from_a_view_eight_bytes_off(dev, sources, k):
    """the source starts 8 bytes past a 16-byte boundary, the output on one: with k even no
    slice pair agrees modulo 16 (8-byte records throughout); with k odd every other one does
    (a head record, the 16-byte body, no tail)"""
    import torch
    src = sources[k]
    base = torch.zeros(N * k + 3, dtype=torch.int64, device="cuda")
    assert base.data_ptr() % 16 == 0
    view = base[1:1 + N * k].view(N, k)
    view.copy_(torch.from_numpy(src).cuda())
    assert view.data_ptr() % 16 == 8
    for keep in ([1, 2, 3, 4], [0, 2, 4]):
        got = run(dev, view, keep, k)
        assert np.array_equal(got, src[keep])
    # and the output 8 bytes off as well: both ends agree again
    obuf = torch.full((3 * k + 3,), SENTINEL, dtype=torch.int64, device="cuda")
    out = obuf[1:1 + 3 * k].view(3, k)
    assert out.data_ptr() % 16 == 8
    dev.gather_clients(view, [0, 2, 4], out=out)
    assert dev.status() == 0
    h = obuf.cpu().numpy()
    assert h[0] == SENTINEL and (h[1 + 3 * k:] == SENTINEL).all()
    assert np.array_equal(h[1:1 + 3 * k].reshape(3, k), src[[0, 2, 4]])


def test_gather_clamps_an_index_past_n(dev, sources):
    """an index >= n cannot be seen by the host: the kernel clamps it to the last client
    (nothing is read out of bounds) and raises FLTEE_DEV_ERR_LAUNCH in the status word"""
    import torch
    k = 129
    src = sources[k]
    buf = torch.full((GUARD + 2 * k + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    out = buf[GUARD:GUARD + 2 * k].view(2, k)
    dev.gather_clients(torch.from_numpy(src).cuda(), [1, N + 2], out=out)
    assert dev.status() == DEV_ERR_LAUNCH
    assert dev.status() == 0  # (cleared by the read)
    h = buf.cpu().numpy()
    assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + 2 * k:] == SENTINEL).all()
    assert np.array_equal(h[GUARD:GUARD + 2 * k].reshape(2, k), src[[1, N - 1]])


def test_gather_refuses_before_the_device(dev, sources):
    import torch
    src = torch.from_numpy(sources[2]).cuda()
    with pytest.raises(RuntimeError, match="0x2"):
        dev.gather_clients(src, [0, 1, 2, 3, 4, 4])  # n_keep > n
