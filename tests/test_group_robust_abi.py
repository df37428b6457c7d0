"""fltee_krum_gram_ranges_device on the CPU: the header declares it with the signature the library
exports and ctypes mirrors, its refusals are host arithmetic (no device touched: the pointers are
never dereferenced), and the Python mirror raises on the same arguments before it allocates."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")

HEADER = os.path.join(ROOT, "include", "fltee_agg.h")
NAME = "fltee_krum_gram_ranges_device"
INVALID = 0x2


def test_header_declares_and_library_exports_the_symbol():
    from fltee import _lib as L
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"fltee_status_t\s+" + NAME + r"\s*\((.*?)\)\s*;", code, re.S)
    assert decl, "not declared"
    params = [re.sub(r"\s+", " ", p.strip()) for p in decl.group(1).split(",")]
    assert params == ["const void *d_in", "int packed", "size_t n", "size_t d", "uint32_t ranks", "double *d_G_out"]
    assert hasattr(L.lib(), NAME)
    assert L.SIGNATURES[NAME] == (ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t,
                                                    ctypes.c_uint32, ctypes.c_void_p])
    fn = getattr(L.lib(), NAME)
    assert fn.restype is ctypes.c_uint32 and list(fn.argtypes) == L.SIGNATURES[NAME][1]


@pytest.mark.parametrize("packed", [0, 1])
def test_refusals_are_host_arithmetic(packed):
    """no GPU is needed to be refused, and a refused call reads neither pointer"""
    from fltee import _lib as L
    fn = getattr(L.lib(), NAME)
    p = ctypes.c_void_p(16)  # never dereferenced
    n, d = 10, 1101
    assert fn(p, packed, n, d, 0, p) == INVALID                    # no ranks
    assert fn(p, packed, n, d, 65, p) == INVALID                   # more than an eid can have
    assert fn(p, packed, n, d, 0xFFFFFFFF, p) == INVALID
    assert fn(p, packed, L.KRUM_MAX_N + 1, d, 2, p) == INVALID     # n above FLTEE_KRUM_MAX_N
    assert fn(p, packed, 0, d, 2, p) == INVALID                    # no clients
    assert fn(p, packed, n, 1 << 31, 2, p) == INVALID              # past the 32-bit positions
    assert fn(None, packed, n, d, 2, p) == INVALID                 # null pointers
    assert fn(p, packed, n, d, 2, None) == INVALID
    assert fn(None, packed, n, d, 1, None) == INVALID


def test_the_python_mirror_raises_before_it_allocates():
    import torch

    from fltee import _lib as L
    from fltee import device as D
    rec = torch.zeros(16, dtype=torch.int64)  # a host tensor: a refused call never looks at it
    for n, d, ranks in ((10, 8, 0), (10, 8, 65), (10, 8, -1), (L.KRUM_MAX_N + 1, 8, 2), (0, 8, 2), (10, 1 << 31, 2)):
        with pytest.raises(ValueError, match=NAME):
            D.krum_gram_ranges(rec, n, d, ranks)
        with pytest.raises(ValueError, match=NAME):
            D.krum_gram_ranges(rec, n, d, ranks, packed=True)


def test_the_cuts_fall_on_chunk_boundaries():
    """the rule the header states, on the shapes the GPU tests use: range i = the whole chunks
    [chunks i / ranks, chunks (i + 1) / ranks); the geometry is the library's (host arithmetic)"""
    from fltee import _lib as L
    geo = (ctypes.c_uint64 * 6)()
    for (n, d), want_chunks in (((10, 1101), 5), ((10, 200), 1), ((130, 1101), 5), ((17, 4099), 17)):
        L.lib().fltee_debug_krum_geometry(n, d, geo)
        np_, tiles, macros, cols, chunks = list(geo)[:5]
        assert chunks == want_chunks and cols % 16 == 0 and np_ == 16 * tiles
        for ranks in (1, 2, 3, 8):
            cuts = [min(chunks * i // ranks * cols, d) for i in range(ranks + 1)]
            assert cuts[0] == 0 and cuts[-1] == d and cuts == sorted(cuts)
            assert all(c % cols == 0 for c in cuts[:-1])
            local = [-(-(b - a) // cols) for a, b in zip(cuts, cuts[1:])]
            assert sum(local) == chunks
    # (10, 1101) on two ranks: the local chunk counts the trace test looks for
    assert [5 * i // 2 for i in range(3)] == [0, 2, 5]
