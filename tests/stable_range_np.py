"""numpy stand-ins for the position-range pieces of aggregation_alg 7's stable network
(include/fltee_agg.h: fltee_stable_init_range / _range_sort / _range_exchange /
_range_merge / _range_strip), so the CPU tests can run fltee.parallel.index_sharded_bubble
without a GPU.  Written from the network's definition, not from the kernels: a bitonic
sorting network over M positions in which the compare-exchange of positions (l, l + 2^j) of
stage 2^s leaves the smaller u64 key at l exactly when bit s of the GLOBAL position l is 0;
a range holds the global positions [pos, pos + len).  Records are 16 bytes {u64 key = idx
<< 32 | global position; f32 val; u32 pad}, kept as int64 [m, 2] tensors; a pad is key = ~0,
val = +0.0.  The fold and compaction stand-ins are range_ops_np's.  Test infrastructure
only."""
import numpy as np
import torch

from range_ops_np import NumpyRangeOps

REC16 = np.dtype([("key", "<u8"), ("val", "<f4"), ("pad", "<u4")])
PAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def rec16(x):
    """the structured view of an int64 [m, 2] tensor (shares its memory)"""
    a = x.numpy()
    assert a.dtype == np.int64 and a.ndim == 2 and a.shape[1] == 2 and a.flags.c_contiguous
    return a.reshape(-1).view(REC16)


def init_range16(idx, val, d, pos, C):
    """Entries [pos, pos + C) of records ++ (i, +0.0) for i < d ++ pads, each keyed with its
    global position, as an int64 [C, 2] tensor."""
    idx = np.asarray(idx, np.uint32)
    val = np.asarray(val, np.float32)
    nrec = len(idx)
    p = pos + np.arange(C, dtype=np.int64)
    out = np.zeros(C, REC16)
    out["key"] = PAD_KEY
    isrec = p < nrec
    out["key"][isrec] = (idx[p[isrec]].astype(np.uint64) << np.uint64(32)) | p[isrec].astype(np.uint64)
    out["val"][isrec] = val[p[isrec]]
    zero = (p >= nrec) & (p < nrec + d)
    out["key"][zero] = ((p[zero] - nrec).astype(np.uint64) << np.uint64(32)) | p[zero].astype(np.uint64)
    return torch.from_numpy(out.view(np.int64).reshape(C, 2).copy())


def _step(a, pos, stage, jlog):
    """every compare-exchange of distance 2^jlog < len(a) of stage 2^stage inside the range"""
    j = 1 << jlog
    x = np.arange(len(a) // 2, dtype=np.int64)
    lo = ((x >> jlog) << (jlog + 1)) | (x & (j - 1))
    hi = lo + j
    up = (((pos + lo) >> stage) & 1) == 0
    al, ah = a[lo].copy(), a[hi].copy()
    swap = np.where(up, al["key"] > ah["key"], al["key"] < ah["key"])
    a[lo] = np.where(swap, ah, al)
    a[hi] = np.where(swap, al, ah)


class NumpyStableRangeOps(NumpyRangeOps):
    """range_ops_np's fold / compaction pieces plus the stable network's five."""

    def stable_sort(self, x, pos, valid=None):  # valid: skipping pad blocks changes nothing
        a = rec16(x)
        for stage in range(1, len(a).bit_length()):
            for jlog in range(stage - 1, -1, -1):
                _step(a, pos, stage, jlog)

    def stable_merge(self, x, pos, stage_log):
        a = rec16(x)
        assert 1 << stage_log > len(a)
        for jlog in range(len(a).bit_length() - 2, -1, -1):
            _step(a, pos, stage_log, jlog)

    def stable_exchange(self, x, theirs, pos, pos_theirs, stage_log):
        a, b = rec16(x), rec16(theirs)
        j = abs(pos - pos_theirs)
        assert j >= len(a) and j & (j - 1) == 0 and j < 1 << stage_log and pos ^ pos_theirs == j
        up = ((min(pos, pos_theirs) >> stage_log) & 1) == 0   # the lower one takes the smaller
        take_small = (pos < pos_theirs) == up
        take = b["key"] < a["key"] if take_small else b["key"] > a["key"]
        a[:] = np.where(take, b, a)

    def stable_strip(self, x):
        a = rec16(x)
        out = (a["key"] >> np.uint64(32)) | (a["val"].view(np.uint32).astype(np.uint64) << np.uint64(32))
        return torch.from_numpy(out.view(np.int64).copy())
