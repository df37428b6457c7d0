"""Option B (position-range sharded `advanced`) on CPU: the driver in
fltee.parallel with numpy stand-ins for the range pieces, every range in one process
(VirtualRanks) — must equal the oracle's single-process `advanced` bit for bit."""
import numpy as np
import pytest
import torch

from longrun import assert_advanced
from range_ops_np import NumpyRangeOps, init_range


def case(seed, n, d, k, idx_hi=None):
    rng = np.random.default_rng(seed)
    if idx_hi is None:
        idx = np.concatenate([rng.choice(d, k, replace=False) for _ in range(n)]).astype(np.uint32)
    else:
        idx = rng.integers(0, idx_hi, n * k).astype(np.uint32)
    val = rng.normal(0, 0.01, n * k).astype(np.float32)
    return idx, val


@pytest.mark.parametrize("exchange", ["transpose", "pairwise"])
@pytest.mark.parametrize("world,n,d,k,idx_hi", [(1, 5, 200, 30, None), (2, 5, 200, 30, None),
                                                (4, 6, 300, 20, None), (8, 4, 100, 50, None),
                                                (4, 10, 150, 40, 40), (2, 7, 333, 1, None),
                                                (4, 10, 150, 40, 1), (8, 30, 100, 60, 3)])
def test_virtual_ranks_match_oracle(oracle, world, n, d, k, idx_hi, exchange):
    from fltee.parallel import VirtualRanks, index_sharded_advanced
    idx, val = case(world * 100 + n, n, d, k, idx_hi)
    M = oracle.next_pow2(n * k + d)
    C = M // world
    chunks = {r: init_range(idx, val, d, r * C, C) for r in range(world)}
    out = index_sharded_advanced(chunks, world, M, n, k, d, ops=NumpyRangeOps(),
                                 comm=VirtualRanks(world), exchange=exchange)
    ref, st = oracle.advanced(k, oracle.as_weights(idx, val), d, n)
    assert st == 0
    # bit for bit; idx_hi: runs of more than n + 1 entries re-associated (longrun.py)
    nlong = assert_advanced(out.numpy(), ref, idx, val, d, n)
    assert idx_hi is not None or nlong == 0


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_virtual_keyed_shuffle_network(oracle, world):
    """The distributed network in mode 2 (nips19's keyed shuffle) == the oracle's
    single-array shuffle, bit for bit."""
    from fltee.parallel import VirtualRanks, distributed_network
    rng = np.random.default_rng(world)
    m = 1024
    idx = rng.integers(0, 50, m).astype(np.uint32)
    val = np.arange(m, dtype=np.float32)
    w = oracle.as_weights(idx, val)
    full = torch.from_numpy(w.view(np.int64).copy())
    C = m // world
    chunks = {r: full[r * C:(r + 1) * C].clone() for r in range(world)}
    out = distributed_network(chunks, world, m, NumpyRangeOps(), VirtualRanks(world), mode=2,
                              seed=0xC0FFEE)
    got = torch.cat([out[r] for r in range(world)]).numpy()
    ref = oracle.shuffle_keyed(w, 0xC0FFEE)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


# the long-run layouts at n = 6, k = 100, d = 400 (L = 1000, M = 1024): all_one_index's run
# covers positions [7, 607], 5 of 8 ranges; `boundary` ends one long run on the last position
# of a range (M / 2 - 1: a range edge for world 2, 4 and 8) and starts the next key's (16
# entries, then a third key's) on the first position of the next range
LONG_N, LONG_D, LONG_K, LONG_M = 6, 400, 100, 1024


@pytest.mark.parametrize("exchange", ["transpose", "pairwise"])
@pytest.mark.parametrize("lay", ["one_client", "all_one_index", "two_adjacent", "index_zero",
                                 "last_and_beyond", "boundary"])
@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_virtual_ranks_long_run_exact(world, lay, exchange):
    """The driver's carry logic alone (the order of the `prev` totals, which rank patches)
    on exactly summable values: any correct carry gives bincount x 1f32/n bit for bit; a
    total dropped, doubled or added across a key change does not."""
    from longrun import assert_bits, boundary_base, exact_ref, exact_values, layout, run_span

    from fltee.parallel import VirtualRanks, index_sharded_advanced
    n, d, k, M = LONG_N, LONG_D, LONG_K, LONG_M
    assert M == 1 << (n * k + d - 1).bit_length()
    idx, val = layout(lay, n, k, d, boundary=M // 2, mid=n + 10), exact_values(n * k)
    C = M // world
    if lay == "boundary":
        b = boundary_base(M // 2, n * k, d)
        s0, s1, s2 = (run_span(idx, d, b + i) for i in range(3))
        assert s0[1] == M // 2 == s1[0] and s1[1] == s2[0]
        assert min(s0[1] - s0[0], s1[1] - s1[0], s2[1] - s2[0]) > n + 1
        assert world == 1 or (M // 2) % C == 0
    elif lay == "all_one_index":
        s0 = run_span(idx, d, 7)
        assert (s0[1] - 1) // (M // 8) - s0[0] // (M // 8) + 1 == 5
    chunks = {r: init_range(idx, val, d, r * C, C) for r in range(world)}
    out = index_sharded_advanced(chunks, world, M, n, k, d, ops=NumpyRangeOps(),
                                 comm=VirtualRanks(world), exchange=exchange)
    assert_bits(out.numpy(), exact_ref(idx, val, d, n))


@pytest.mark.parametrize("m,halo,fold_len,C", [(4096, 8, 4096, 16), (4096, 8, 3000, 16),
                                               ((1 << 16) + 2, 100, 60001, 16),
                                               (1 << 17, 16, 1 << 17, 64),
                                               (1 << 18, 16, 1 << 18, 128)])
def test_fold_stream_model_is_the_sequential_fold(m, halo, fold_len, C):
    """tests/range_ops_np.py's emulator of the streaming fold + patch on exactly summable
    values: whatever its association, it must be the enclave's sequential fold (one record a
    run with the run's sum, dummies elsewhere, the tail copied) — the emulator's own check,
    before the GPU test compares the device with it bit for bit on N(0, 1) values."""
    from longrun import assert_sequential_fold, sorted_runs
    from range_ops_np import fold_stream_model
    Hr = (halo + 15) // 16 * 16
    idx, _ = sorted_runs(m, Hr, C, seed=m)
    val = (1 + np.arange(m) % 7).astype(np.float32)
    gi, gv = fold_stream_model(idx, val, fold_len, halo, Hr, C)
    assert_sequential_fold(gi, gv, idx, val, fold_len, halo)
