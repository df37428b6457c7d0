"""numpy stand-ins for the HIP range pieces of position-sharded `advanced`
(include/fltee_agg.h, SURVEY §8e Option B), so the CPU tests can run
fltee.parallel.index_sharded_advanced — its order of steps and its exchanges —
without a GPU.  Each follows the reference network / fold literally
(advanced.rs:66-101,147-176), with global positions.  Test infrastructure only."""
import numpy as np
import torch

MASK = np.uint64(0xFFFFFFFF)
PAD = 0xFFFFFFFF


def _u(x):
    return x.numpy().view(np.uint64)


def _mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def step_key(seed, ilog, jlog):
    """shuffle_step_key of fl-tee_amd/csrc/common.h (the keyed comparator's per-step key)."""
    return _mix32(_mix32(seed) + ((ilog << 8) | jlog) * 0x9E3779B9)


def _cond2(lo, hi, l, mode, key):
    if mode == 0:
        return (lo & MASK) < (hi & MASK)
    h = ((l.astype(np.uint64) ^ np.uint64(key)) * np.uint64(0x9E3779B1)) & MASK
    return (h >> np.uint64(31)) != 0


def _step(a, pbase, ilog, jlog, mode=0, seed=0):
    """One step (stage 2^ilog, distance 2^jlog < len(a)) of advanced.rs:155-175 (mode 0)
    or of the keyed shuffle (mode 2)."""
    j = 1 << jlog
    x = np.arange(len(a) // 2, dtype=np.int64)
    l = ((x & ~(j - 1)) << 1) | (x & (j - 1))
    m = l + j
    asc = ((pbase + l) & (1 << ilog)) == 0
    al, am = a[l].copy(), a[m].copy()
    key = step_key(seed, ilog, jlog) if mode == 2 else 0
    sw = asc ^ _cond2(al, am, pbase + l, mode, key)
    a[l] = np.where(sw, am, al)
    a[m] = np.where(sw, al, am)


class NumpyRangeOps:
    def pads(self, n, like):
        return torch.full((n,), PAD, dtype=torch.int64)

    def fold_context(self, halo):
        return (halo + 15) // 16 * 16

    def sort(self, x, pos, mode=0, seed=0, valid=None):  # valid: the full network is the same
        a = _u(x)
        for ilog in range(1, len(a).bit_length()):
            for jlog in range(ilog - 1, -1, -1):
                _step(a, pos, ilog, jlog, mode, seed)

    def merge(self, x, pos, stage_log, mode=0, seed=0):
        a = _u(x)
        for jlog in range(len(a).bit_length() - 2, -1, -1):
            _step(a, pos, stage_log, jlog, mode, seed)

    def exchange(self, x, theirs, pos, pos_theirs, stage_log, mode=0, seed=0):
        a, b = _u(x), _u(theirs)
        lower = pos < pos_theirs
        lo, hi = (a, b) if lower else (b, a)
        p = min(pos, pos_theirs) + np.arange(len(a), dtype=np.int64)
        asc = (p & (1 << stage_log)) == 0
        jlog = (abs(pos - pos_theirs)).bit_length() - 1
        key = step_key(seed, stage_log, jlog) if mode == 2 else 0
        sw = asc ^ _cond2(lo, hi, p, mode, key)
        a[:] = np.where(sw, b, a)

    def safe_aggregate(self, x, d):
        """common.rs:25-35 on one range: g[idx] += val for idx < d, in position order."""
        a = _u(x)
        idx = (a & MASK).astype(np.int64)
        val = (a >> np.uint64(32)).astype(np.uint32).view(np.float32)
        out = np.zeros(d, np.float32)
        sel = idx < d
        np.add.at(out, idx[sel], val[sel])
        return torch.from_numpy(out)

    def select(self, x, d):
        a = _u(x)
        return torch.from_numpy(a[(a & MASK) < d].view(np.int64).copy())

    def ordered(self, lst, d, coef):
        """common.rs:25-35 + 14-19 on the concatenated list: in-order f32 sums, x coef."""
        a = _u(lst)
        idx = (a & MASK).astype(np.int64)
        val = (a >> np.uint64(32)).astype(np.uint32).view(np.float32)
        out = np.zeros(d, np.float32)
        np.add.at(out, idx, val)
        return torch.from_numpy(out * np.float32(coef))

    def steps(self, x, pos, stage_log, step_top, step_bot):
        a = _u(x)
        for jlog in range(step_top, step_bot - 1, -1):
            _step(a, pos, stage_log, jlog)

    def fold(self, buf, origin, end, pos_base, fold_len, halo, key=0):
        """fo_fold (advanced.rs:66-101) over the buffer's global positions, one walk from
        local position 1 (the record in front of it tells whether the run there began
        before): the context in front makes the carry exact for every run of <= halo + 1
        entries; a run begun before the walk and ended in [origin, end) is left as a dummy
        and carried by the side record (the device's FoldSide, one walk per range here)."""
        s = _u(buf)
        out = s.copy()
        b, C = 1, end - origin
        hasprev = pos_base + b - 1 >= 0
        kprev = int(s[b - 1] & MASK) if hasprev else None
        started, pre_i, pre_v = False, 0, np.float32(0)
        in_head, unbroken, corr, piece, pfull = False, True, False, False, False
        ck, cs, pf_key, pk, pq = 0, np.float32(0), 0, 0, np.float32(0)
        for q in range(b, end + 1):
            g = pos_base + q
            ci = int(s[q] & MASK)
            cv = np.uint32(int(s[q] >> np.uint64(32))).view(np.float32)
            eq = started and ci == pre_i
            copy = g - 1 >= fold_len
            dmy = g < fold_len and eq
            hend = in_head and not copy and not dmy
            sup = hend and origin <= q - 1 < end
            if origin <= q - 1 < end:
                if copy:
                    out[q - 1] = s[q - 1]
                elif dmy or sup:
                    out[q - 1] = np.uint64(0xFFFFFFFF - (g - 1))
                else:
                    out[q - 1] = np.uint64(pre_i) | (np.uint64(np.float32(pre_v).view(np.uint32)) << np.uint64(32))
            if sup:
                corr, ck, cs = True, pre_i, pre_v
            in_head = in_head and not hend and not copy
            if g >= 0:
                if not started:
                    pf_key = ci
                    in_head = hasprev and ci == kprev
                else:
                    unbroken = unbroken and eq
                pre_v = np.float32(pre_v + cv) if eq else cv
                pre_i = ci
                started = True
            if q == b + C - 1 and started and g >= 0:
                piece, pfull, pk, pq = True, unbroken, pre_i, pre_v
        fl = (1 if piece else 0) | (2 if piece and pfull else 0) | (4 if corr else 0)
        side = np.array([pf_key, pk, np.float32(pq).view(np.uint32), fl, ck,
                         np.float32(cs).view(np.uint32)], dtype=np.uint32)
        return torch.from_numpy(out.view(np.int64).copy()), side

    def total(self, side, span, halo, key=0):
        return torch.from_numpy(np.array([side[0], side[1], side[2], side[3] & 3], np.uint32).view(np.int32))

    @staticmethod
    def _agg(t):
        a = np.asarray(t).view(np.uint32)
        return int(a[0]), int(a[1]), np.uint32(a[2]).view(np.float32), int(a[3]) & 3

    @staticmethod
    def _combine(x, y):
        if not x[3] & 1:
            return y
        if not y[3] & 1:
            return x
        full = bool(x[3] & 2) and bool(y[3] & 2) and x[1] == y[0]
        q = np.float32(x[2] + y[2]) if (y[3] & 2 and y[0] == x[1]) else y[2]
        return x[0], y[1], q, 1 | (2 if full else 0)

    def patch(self, dst, origin, end, pos_base, fold_len, halo, side, prev):
        run = (0, 0, np.float32(0), 0)
        for t in prev:
            run = self._combine(run, self._agg(t.numpy() if hasattr(t, "numpy") else t))
        if side[3] & 4 and run[3] & 1 and run[1] == int(side[4]):
            tot = np.float32(run[2] + np.uint32(side[5]).view(np.float32))
            v = np.uint64(int(side[4])) | (np.uint64(tot.view(np.uint32)) << np.uint64(32))
            dst[origin] = torch.tensor(np.array([v], np.uint64).view(np.int64)[0])

    def compact(self, chunk, d, key=0):
        a = _u(chunk)
        idx = (a & MASK).astype(np.int64)
        val = (a >> np.uint64(32)).astype(np.uint32).view(np.float32)
        out = np.zeros(d, np.float32)
        sel = idx < d
        out[idx[sel]] = val[sel]
        return torch.from_numpy(out)

    def finish(self, out, coef):
        return out * np.float32(coef)

    def dp(self, out, sigma, clipping, n, seed):
        raise NotImplementedError


def init_range(idx, val, d, pos, C):
    """Entries [pos, pos + C) of advanced's padded array (advanced.rs:116-142)."""
    nrec = len(idx)
    p = pos + np.arange(C, dtype=np.int64)
    out = np.full(C, PAD, dtype=np.uint64)
    rec = p < nrec
    out[rec] = idx[p[rec]].astype(np.uint64) | (val[p[rec]].view(np.uint32).astype(np.uint64) << np.uint64(32))
    ini = (p >= nrec) & (p < nrec + d)
    out[ini] = (p[ini] - nrec).astype(np.uint64)
    return torch.from_numpy(out.view(np.int64).copy())


# ---- the streaming fold + patch of a whole array, in the device's own association ----
# (k_fold.hip fold_stream_kernel / fold_patch_kernel, common.h fa_combine; origin = pbase = 0,
# no totals of earlier ranges.)  Aggregates are tuples of arrays (F, K, Q, fl).
def _fa_empty(shape):
    return (np.zeros(shape, np.uint32), np.zeros(shape, np.uint32), np.zeros(shape, np.float32),
            np.zeros(shape, np.uint32))


def _fa_combine(x, y):
    """fa_combine exactly as in common.h, elementwise"""
    xF, xK, xQ, xf = x
    yF, yK, yQ, yf = y
    xe, ye = (xf & 1) == 0, (yf & 1) == 0
    yfull = (yf & 2) != 0
    full = ((xf & 2) != 0) & yfull & (xK == yF)
    r = (xF, yK, np.where(yfull & (yF == xK), (xQ + yQ).astype(np.float32), yQ),
         np.where(full, 3, 1).astype(np.uint32))
    return tuple(np.where(xe, b, np.where(ye, a, c)) for a, b, c in zip(x, y, r))


def _fa_scan(g):
    """the inclusive Hillis-Steele scan along the last axis (the wave's __shfl_up rounds,
    fp_block_scan's LDS rounds): x = the element o in front (empty before the first)"""
    n = g[0].shape[-1]
    o = 1
    while o < n:
        e = _fa_empty(g[0].shape[:-1] + (o,))
        g = _fa_combine(tuple(np.concatenate([ee, a[..., :-o]], axis=-1) for ee, a in zip(e, g)), g)
        o <<= 1
    return g


def _fa_take(g, sel):
    return tuple(a[sel] for a in g)


def fold_stream_model(idx, val, fold_len, halo, Hr, C):
    """fltee_fold_device(src = (idx, val), fold_len, halo) as the device computes it, bit for
    bit, vectorised over lanes; Hr, C: the fold's geometry (fltee_debug_fold_geometry).
    Lane j walks [a - Hr, a + C + 16), a = j C, in order (pre_idx / pre_val, the emitted
    record of q - 1 at step q), keeps its FoldSide (the piece [a - Hr, a - Hr + C): first
    key, last key, the run partial at its last position; the head run's sum when it ends in
    the chunk), the 64 lanes of a wave scan their pieces (Hillis-Steele) into the wave
    aggregate; the patch folds each of its 256 threads' slice of the wave aggregates in front
    of the block left to right, scans the 256 partials, folds the thread's 4 lanes in order,
    scans again, and writes (ck, run.Q + S) at a for every lane with a head run.  Returns
    dst's (idx u32, val f32)."""
    idx = np.ascontiguousarray(idx, np.uint32)
    val = np.ascontiguousarray(val, np.float32)
    m = len(idx)
    assert Hr == (halo + 15) // 16 * 16 and Hr % 16 == 0 and C % 16 == 0
    lanes = (m + C - 1) // C
    waves = (lanes + 63) // 64
    a = np.arange(waves * 64, dtype=np.int64) * C
    b = a - Hr
    live = a < m
    MAXU = np.uint32(0xFFFFFFFF)

    def rd(q):  # the record at q: zeros outside [0, m), as the kernel's window loads
        ok = (q >= 0) & (q < m)
        qc = np.clip(q, 0, m - 1)
        return np.where(ok, idx[qc], np.uint32(0)), np.where(ok, val[qc], np.float32(0))

    fp = np.maximum(b, 0)
    pf_key = np.where(live & (fp < m), idx[np.clip(fp, 0, m - 1)], np.uint32(0)).astype(np.uint32)
    in_head = live & (b - 1 >= 0) & (idx[np.clip(b - 1, 0, m - 1)] == pf_key)
    pre_idx = np.full(len(a), 0xFFFFFFFE, np.uint32)
    pre_val = np.zeros(len(a), np.float32)
    cs = np.zeros(len(a), np.float32)
    corr = np.zeros(len(a), bool)
    piece = np.zeros(len(a), bool)
    pk = np.zeros(len(a), np.uint32)
    pq = np.zeros(len(a), np.float32)
    oi, ov = idx.copy(), val.copy()
    for step in range((Hr + C + 16) // 16 * 16):
        q = b + step
        e = q - 1
        ci, v = rd(q)
        pi, pv = rd(e)
        eq = ci == pre_idx
        copy = e >= fold_len
        dmy = (q < fold_len) & eq
        inchunk = (e >= a) & (e < a + C)
        sup = in_head & ~copy & ~dmy & inchunk
        du = dmy | sup
        st = inchunk & live & (e < m)
        es = e[st]
        oi[es] = np.where(copy, pi, np.where(du, (MAXU - e.astype(np.uint32)), pre_idx))[st]
        ov[es] = np.where(copy, pv, np.where(du, np.float32(0), pre_val))[st]
        cs = np.where(sup, pre_val, cs)
        corr |= sup
        in_head = in_head & (dmy | (step == 0))
        valid = q >= 0
        nv = np.where(eq, (pre_val + v).astype(np.float32), v)
        pre_val = np.where(valid, nv, pre_val)
        pre_idx = np.where(valid, ci, pre_idx)
        if step == C - 1:  # the piece's last position b + C - 1
            piece, pk, pq = valid.copy(), pre_idx.copy(), pre_val.copy()
    fl = np.where(live, piece * 1 + (piece & (pk == pf_key)) * 2, 0).astype(np.uint32)
    corr &= live
    side = (pf_key, pk, pq, fl)
    wagg = _fa_take(_fa_scan(tuple(x.reshape(waves, 64) for x in side)), (slice(None), 63))
    # the patch: blocks of 1,024 lanes = 256 threads x 4
    nblk = (lanes + 1023) // 1024
    pad = nblk * 1024 - len(a)
    if pad > 0:
        side = tuple(np.concatenate([x, np.zeros(pad, x.dtype)]) for x in side)
        corr = np.concatenate([corr, np.zeros(pad, bool)])
        cs = np.concatenate([cs, np.zeros(pad, np.float32)])
    else:
        side, corr, cs = tuple(x[:nblk * 1024] for x in side), corr[:nblk * 1024], cs[:nblk * 1024]
    t = np.arange(256, dtype=np.int64)[None, :]
    wb = (np.arange(nblk, dtype=np.int64) * 16)[:, None]  # the waves in front of the block
    w0, w1 = wb * t // 256, wb * (t + 1) // 256
    acc = _fa_empty((nblk, 256))
    for i in range(int((w1 - w0).max()) if nblk else 0):
        w = w0 + i
        g = _fa_take(wagg, np.clip(w, 0, waves - 1))
        nxt = _fa_combine(acc, g)
        acc = tuple(np.where(w < w1, n_, a_) for n_, a_ in zip(nxt, acc))
    carry = _fa_take(_fa_scan(acc), (slice(None), slice(255, 256)))  # allw (no earlier ranges)
    sd = tuple(x.reshape(nblk, 256, 4) for x in side)
    corr4, cs4 = corr.reshape(nblk, 256, 4), cs.reshape(nblk, 256, 4)
    mine = _fa_empty((nblk, 256))
    for i in range(4):
        mine = _fa_combine(mine, _fa_take(sd, (slice(None), slice(None), i)))
    inc = _fa_scan(mine)
    e1 = _fa_empty((nblk, 1))
    run = _fa_combine(tuple(np.broadcast_to(c, (nblk, 256)) for c in carry),
                      tuple(np.concatenate([ee, x[:, :-1]], axis=1) for ee, x in zip(e1, inc)))
    aj = (np.arange(nblk * 1024, dtype=np.int64) * C).reshape(nblk, 256, 4)
    for i in range(4):
        s_i = _fa_take(sd, (slice(None), slice(None), i))
        ck = s_i[0]  # the head run's key: the piece's first key
        c = corr4[:, :, i] & ((run[3] & 1) != 0) & (run[1] == ck)
        tot = (run[2] + cs4[:, :, i]).astype(np.float32)
        pos = aj[:, :, i][c]
        oi[pos] = ck[c]
        ov[pos] = tot[c]
        run = _fa_combine(run, s_i)
    return oi, ov
