"""The shape plan of aggregate() (engine.h Plan), read on the CPU through fltee_debug_plan:
what a public shape (alg, n, k, d, opts) is refused for, which route and tail it takes, and
the bytes of every scratch buffer that touches.  Host arithmetic only: no device is needed.

The refusal pairs are fltee_aggregate_device's own conditions (each one shape at the limit,
refused with 0x2, and its neighbour just inside, accepted); the byte checks tie the plan to
fltee_workspace_bytes and to the launchers' own size queries.  tests/test_gpu_plan.py runs
the routes named here and checks that a reserved shape allocates nothing."""
import ctypes
import math
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")

# engine.h: Route, Tail, Ws
(R_NONE, R_DENSE, R_SCATTER, R_COUNTING, R_FLAT, R_SWEEP, R_TREE, R_TREE_LAZY, R_ADVANCED, R_BUBBLE,
 R_OPTIMIZED, R_NIPS19) = range(12)
T_NONE, T_FUSED, T_STREAM, T_ONE, T_SORT = range(5)
WS = ("a", "b", "mat", "r", "coef", "rec", "keys", "radix", "oram", "side", "lb", "s16", "cnt", "sel")
INVALID = 0x2


class Plan:
    def __init__(self, alg, n, k, d, **kw):
        from fltee import _lib as L
        from fltee import device as D
        o = D.opts(**kw)
        out = (ctypes.c_uint64 * (4 + len(WS)))()
        self.status = L.lib().fltee_debug_plan(alg, n, k, d, ctypes.byref(o), out)
        self.route, self.tail, self.M, self.halo = out[0], out[1], out[2], out[3]
        self.bytes = dict(zip(WS, list(out)[4:]))
        self.total = sum(self.bytes.values())


def oram_slots(d):  # k_oram.hip: Z = 4 blocks a bucket, 2N - 1 buckets, a stash of 20
    n = 1
    while n < max(d, 1):
        n *= 2
    return 4 * (2 * n - 1) + 20


# The GPU test's table (tests/test_gpu_plan.py imports it): the smallest shape that reaches
# each route, (name, alg, n, k, d, opts, route, tail).
ROUTES = [
    ("dense", 4, 3, 257, 257, dict(dense=True), R_DENSE, T_NONE),
    ("scatter rows", 4, 4, 8, 100, {}, R_SCATTER, T_NONE),
    # the rows are left once n * d > 2^24 cells (and > 64 * next_pow2(n * k))
    ("counting-sort fold", 4, 2, 3, (1 << 23) + 1, {}, R_COUNTING, T_NONE),
    ("sweep", 3, 4, 8, 100, {}, R_SWEEP, T_NONE),
    ("flat-ordered", 3, 3, 64, 64, {}, R_FLAT, T_NONE),
    ("tree", 5, 2, 4, 16, dict(oram_tree=True), R_TREE, T_NONE),
    ("tree lazy", 5, 2, 4, 16, dict(oram_tree=True, oram_lazy=True), R_TREE_LAZY, T_FUSED),
    ("advanced fused", 1, 30, 500, 5000, {}, R_ADVANCED, T_FUSED),
    ("advanced streaming", 1, 400, 1000, 20000, {}, R_ADVANCED, T_STREAM),
    ("advanced second sort", 1, 4, 8, 64, dict(k_req=4), R_ADVANCED, T_SORT),
    ("one entry", 1, 1, 0, 1, {}, R_ADVANCED, T_ONE),
    ("alg 7", 7, 30, 500, 5000, {}, R_BUBBLE, T_FUSED),
    ("alg 6", 6, 10, 50, 500, dict(batch=4), R_OPTIMIZED, T_FUSED),
    ("nips19", 2, 4, 16, 64, dict(seed=7), R_NIPS19, T_NONE),
]
CLIPPED = [
    ("scatter rows, clip", 4, 4, 8, 100, dict(clip=True, clipping=0.5), R_SCATTER, T_NONE),
    ("tree, clip", 5, 2, 4, 16, dict(oram_tree=True, clip=True, clipping=0.5), R_TREE, T_NONE),
]


def option_shapes():
    """The option tests' table (tests/test_gpu_options.py): the fourteen routes at shapes the
    lattice inputs of tests/options_model.py fit (k >= 16 wherever the route has records,
    n = 6 where that is free so that every lattice client occurs), and the dense-flagged
    uploads (k == d) of the algs that have no dense route."""
    change = {
        "dense": dict(n=6),
        "scatter rows": dict(n=6, k=16),
        "counting-sort fold": dict(k=16),
        "sweep": dict(n=6, k=16),
        "flat-ordered": dict(n=6),
        "tree": dict(n=6, k=16, d=32),
        "tree lazy": dict(n=6, k=16, d=32),
        "advanced second sort": dict(k=16),  # (n stays 4: see test_gpu_options.py sums)
        "nips19": dict(n=6),
    }
    out = []
    for name, alg, n, k, d, kw, route, tail in ROUTES:
        c = change.get(name, {})
        out.append((name + ", options", alg, c.get("n", n), c.get("k", k), c.get("d", d), kw, route, tail))
    return out + [
        ("advanced, dense flag", 1, 7, 64, 64, dict(dense=True), R_ADVANCED, T_FUSED),
        ("nips19, dense flag", 2, 7, 64, 64, dict(dense=True, seed=7), R_NIPS19, T_NONE),
        ("alg 6, dense flag", 6, 7, 64, 64, dict(dense=True, batch=3), R_OPTIMIZED, T_FUSED),
        ("alg 7, dense flag", 7, 7, 64, 64, dict(dense=True), R_BUBBLE, T_FUSED),
    ]


OPTION_SHAPES = option_shapes()


@pytest.mark.parametrize("case", ROUTES + CLIPPED + OPTION_SHAPES, ids=lambda c: c[0])
def test_routes_and_tails(case):
    _, alg, n, k, d, kw, route, tail = case
    p = Plan(alg, n, k, d, **kw)
    assert p.status == 0
    assert (p.route, p.tail) == (route, tail)


@pytest.mark.parametrize("case", ROUTES + OPTION_SHAPES, ids=lambda c: c[0])
def test_clip_scratch_of_every_route(case):
    """FLTEE_OPT_CLIP changes no route; a coefficient per client everywhere, and a clipped
    copy of the records on every route but the dense accumulate of algs 3, 4 and 5 (which
    takes the coefficients) — FLTEE_OPT_DENSE on algs 1, 2, 6 and 7 only asserts k == d."""
    _, alg, n, k, d, kw, route, tail = case
    plain, p = Plan(alg, n, k, d, **kw), Plan(alg, n, k, d, clip=True, clipping=0.5, **kw)
    assert p.status == 0 and (p.route, p.tail) == (route, tail)
    assert p.bytes["coef"] == n * 4
    assert p.bytes["rec"] == (0 if route == R_DENSE else n * k * 8)
    assert plain.bytes["coef"] == 0 and plain.bytes["rec"] == 0
    assert {w: b for w, b in p.bytes.items() if w not in ("coef", "rec")} == \
           {w: b for w, b in plain.bytes.items() if w not in ("coef", "rec")}


def nips19_kq(d, n, tf):
    """A request k whose threshold T = 2 k / 100 * ln(d * n) (engine.hip nips19_threshold, in
    f32) truncates to tf, chosen with T's fraction nearest one half so that f32 rounding (T
    near 2^19: steps of 1/16) cannot move it across an integer."""
    step = 2.0 / 100.0 * math.log(d * n)
    k0 = int((tf + 0.5) / step)
    kq = min((k0 - 1, k0, k0 + 1), key=lambda q: abs(q * step - tf - 0.5))
    assert 0.3 < kq * step - tf < 0.7
    return kq


P29, P31 = 1 << 29, 1 << 31
TREE = dict(oram_tree=True)
# (what, alg, refused (n, k, d, opts), accepted (n, k, d, opts))
REFUSALS = [
    ("no clients", 4, (0, 1, 8, {}), (1, 1, 8, {})),
    ("n * k + d >= 2^31 (32-bit positions; the sweep has no other limit)",
     3, (1, 1, P31 - 1, {}), (1, 1, P31 - 2, {})),
    ("advanced: next_pow2(n * k + d) > 2^29", 1, (1, 1, P29, {}), (1, 1, P29 - 1, {})),
    ("alg 7: next_pow2(n * k + d) > 2^29", 7, (1, 1, P29, {}), (1, 1, P29 - 1, {})),
    ("alg 6: a batch's array > 2^29", 6, (4, 1, P29 - 1, dict(batch=2)), (4, 1, P29 - 2, dict(batch=2))),
    ("alg 6: no batch is one batch of n", 6, (4, 1, P29 - 3, {}), (4, 1, P29 - 4, {})),
    ("alg 6: a batch past n is clamped to n", 6, (4, 1, P29 - 3, dict(batch=9)), (4, 1, P29 - 4, dict(batch=9))),
    # n * d > 2^30 cells: never the scatter rows
    ("non_oblivious ordered fold: next_pow2(n * k) > 2^29",
     4, (1, P29 + 1, (1 << 30) + 1, {}), (1, P29, (1 << 30) + 1, {})),
    ("baseline flat-ordered (k == d): next_pow2(n * k) > 2^29",
     3, (3, P29 // 3 + 1, P29 // 3 + 1, {}), (3, P29 // 3, P29 // 3, {})),
    ("path_oram flat-ordered (k == d): next_pow2(n * k) > 2^29",
     5, (3, P29 // 3 + 1, P29 // 3 + 1, {}), (3, P29 // 3, P29 // 3, {})),
    ("nips19 (T = 0): next_pow2(n * k) > 2^29", 2, (1, P29 + 1, 1, dict(k_req=0)), (1, P29, 1, dict(k_req=0))),
    ("nips19: next_pow2(n * k + d * tf) > 2^29 through tf",
     2, (1, 0, 1024, dict(k_req=nips19_kq(1024, 1, (1 << 19) + 1))),
     (1, 0, 1024, dict(k_req=nips19_kq(1024, 1, 1 << 19)))),
    ("alg 7 with k_req != k", 7, (4, 8, 64, dict(k_req=7)), (4, 8, 64, dict(k_req=8))),
    ("alg 7 with k_req != k (above)", 7, (4, 8, 64, dict(k_req=9)), (4, 8, 64, {})),
    ("advanced folding past its array: n * k_req + d > n * k + d",
     1, (4, 8, 64, dict(k_req=9)), (4, 8, 64, dict(k_req=8))),
    ("tree past 2^22 blocks (oram_fits)", 5, (1, 1, (1 << 22) + 1, TREE), (1, 1, 1 << 22, TREE)),
    ("lazy tree past 2^22 blocks (oram_fits)", 5, (1, 1, (1 << 22) + 1, dict(oram_lazy=True, **TREE)),
     (1, 1, 1 << 22, dict(oram_lazy=True, **TREE))),
    # 2 * n * k + 2 * d accesses: next_pow2 > 2^29
    ("tree: the leaf precompute's sort > 2^29 (oram_fits)", 5, (1, (1 << 28) - 15, 16, TREE),
     (1, (1 << 28) - 16, 16, TREE)),
    ("DENSE with k != d", 3, (2, 63, 64, dict(dense=True)), (2, 64, 64, dict(dense=True))),
    ("unknown alg 0", 0, (2, 4, 64, {}), None),
    ("unknown alg 8", 8, (2, 4, 64, {}), None),
    ("the last alg", 7, None, (2, 4, 64, {})),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0])
def test_refusals_at_the_boundary(case):
    _, alg, bad, good = case
    if bad:
        n, k, d, kw = bad
        assert Plan(alg, n, k, d, **kw).status == INVALID
    if good:
        n, k, d, kw = good
        assert Plan(alg, n, k, d, **kw).status == 0


def test_nips19_tf_overflow_is_refused():
    """tf > 2^31 / d guards d * tf against overflow.  Every shape inside it with d * tf > 2^29
    is refused by the network limit (the pair above), so only the refusal is checked here:
    astronomically large request ks, and a tf just past the guard."""
    assert Plan(2, 1, 0, 1 << 20, k_req=1 << 40).status == INVALID
    assert Plan(2, 1, 0, 1024, k_req=nips19_kq(1024, 1, (1 << 21) + 2)).status == INVALID
    assert Plan(2, 1, 0, 1024, k_req=1 << 62).status == INVALID


@pytest.mark.parametrize("case", ROUTES + CLIPPED + [
    ("alg 7 past the limit", 7, 1, 1, P29 + 1, {}, R_BUBBLE, None),
    ("advanced, a wide halo", 1, 2, 3, 40, dict(fold_halo=100), R_ADVANCED, None),
    ("alg 6, one batch", 6, 10, 50, 500, {}, R_OPTIMIZED, None),
    ("nips19 with dummies", 2, 30, 500, 5000, dict(k_req=16), R_NIPS19, None),
] + OPTION_SHAPES + [
    (name + ", clip", alg, n, k, d, dict(kw, clip=True, clipping=0.5), route, tail)
    for name, alg, n, k, d, kw, route, tail in OPTION_SHAPES
], ids=lambda c: c[0])
def test_workspace_bytes_is_the_sum_of_the_plan(case):
    from fltee import device as D
    _, alg, n, k, d, kw, route, _ = case
    p = Plan(alg, n, k, d, **kw)
    assert p.route == route
    assert p.total == D.workspace_bytes(alg, n, k, d, **kw)
    assert p.bytes["sel"] == 0  # data-sized: outside the plan


def test_alg7_is_advanced_plus_the_stable_networks_records():
    for n, k, d in ((30, 500, 5000), (400, 1000, 20000), (3, 5, 11)):
        a, b = Plan(1, n, k, d), Plan(7, n, k, d)
        assert (a.tail, a.M, a.halo) == (b.tail, b.M, b.halo)
        assert b.bytes == dict(a.bytes, s16=a.M * 16)
        assert b.total == a.total + a.M * 16


def test_lazy_tree_plans_its_readout():
    """The lazy tree's readout is `advanced` over one client of oram_slots(d) records, halo 1:
    its side and look-back bytes are that shape's, and its two arrays cover it."""
    for n, k, d in ((2, 4, 16), (3, 100, 5000), (2, 50, 100000)):
        lazy = Plan(5, n, k, d, oram_tree=True, oram_lazy=True)
        nested = Plan(1, 1, oram_slots(d), d, fold_halo=1)
        assert lazy.status == 0 and nested.status == 0
        assert (lazy.tail, lazy.M, lazy.halo) == (nested.tail, nested.M, 1)
        assert lazy.bytes["side"] == nested.bytes["side"] and lazy.bytes["lb"] == nested.bytes["lb"]
        assert lazy.bytes["side"] + lazy.bytes["lb"] > 0
        assert lazy.bytes["a"] >= nested.bytes["a"] and lazy.bytes["b"] >= nested.bytes["b"]
        assert lazy.bytes["oram"] == oram_slots(d) * 24


def fold_side_bytes(span, halo):
    """k_fold.hip fold_side_bytes for a streaming fold (not the one-lane walk): a 32-byte
    side record per lane, 64 lanes a wave, and a 16-byte aggregate per wave; a lane walks a
    chunk of C positions (fold_chunk)."""
    hr = (halo + 15) // 16 * 16
    c = 64
    while c < hr:
        c *= 2
    while c > 16 and span // (64 * c) < 1024:
        c //= 2
    if c >= hr and span // (128 * c) >= 1024:
        c *= 2
    lanes = -(-span // c)
    return -(-lanes // 64) * (64 * 32 + 16)


@pytest.mark.parametrize("n,k,d,k_req", [(4, 8, 64, 4), (30, 500, 5000, 499), (400, 1000, 20000, 0)])
def test_k_req_fold_side_bytes_are_the_real_folds(n, k, d, k_req):
    """k_req != k: the fold runs over the whole array (M positions) with fold_len =
    n * k_req + d and halo n; its side records are planned from that call's own shape."""
    from fltee import _lib as L
    p = Plan(1, n, k, d, k_req=k_req)
    assert p.tail == T_SORT and p.halo == n
    assert n + 1 < n * k_req + d  # not the one-lane walk
    assert p.bytes["side"] == fold_side_bytes(p.M, n)
    assert p.bytes["side"] >= L.lib().fltee_fold_side_bytes(p.M, n)
    assert p.bytes["lb"] == 0


def test_clip_scratch():
    """FLTEE_OPT_CLIP: a coefficient per client, and a clipped copy of the records wherever
    the route reads records (everything but the dense accumulate)."""
    assert Plan(4, 4, 8, 100, clip=True).bytes["coef"] == 16
    assert Plan(4, 4, 8, 100, clip=True).bytes["rec"] == 4 * 8 * 8
    assert Plan(3, 3, 257, 257, dense=True, clip=True).bytes["rec"] == 0
    assert Plan(5, 2, 16, 16, dense=True, clip=True, oram_tree=True).bytes["rec"] == 2 * 16 * 8
    for alg, kw in ((1, {}), (2, dict(seed=7)), (6, dict(batch=3)), (7, {})):  # no dense route
        assert Plan(alg, 4, 64, 64, dense=True, clip=True, **kw).bytes["rec"] == 4 * 64 * 8
    assert Plan(0, 4, 8, 100, clip=True).status == INVALID


def test_alg6_covers_its_short_last_batch():
    """10 clients in batches of 4: the last batch has 2, a smaller array and halo; every
    buffer covers both."""
    p = Plan(6, 10, 50, 500, batch=4)
    full, last = Plan(1, 4, 50, 500), Plan(1, 2, 50, 500)
    for w in WS:
        assert p.bytes[w] == max(full.bytes[w], last.bytes[w]), w
    assert (p.M, p.halo, p.tail) == (full.M, 4, full.tail)
