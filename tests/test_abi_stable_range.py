"""The C ABI of alg 7's position-range pieces (include/fltee_agg.h: fltee_stable_init_range /
_range_sort / _range_exchange / _range_merge / _range_strip): the five symbols are exported
with the documented argument lists, and every refusal is host arithmetic — it returns
FLTEE_ERROR_INVALID_PARAMETER (0x2) before any device call, so it is checked here without a
GPU (null pointers throughout: a call that got past its checks would not return 0x2)."""
import re

import pytest

from test_abi import HEADER

INVALID = 0x2
T, BIG = 1 << 12, 1 << 29

ARGS = {  # the header's prototypes (the issue's), argument by argument
    "fltee_stable_init_range_device": ["const void *d_records", "size_t nrec", "size_t d",
                                       "size_t pos_base", "size_t m", "void *d_dst16", "void *stream"],
    "fltee_stable_range_sort_device": ["void *d_rec16", "size_t m", "size_t pos_base", "size_t valid",
                                       "void *stream"],
    "fltee_stable_range_exchange_device": ["void *d_mine16", "const void *d_theirs16", "size_t m",
                                           "size_t pos_mine", "size_t pos_theirs", "uint32_t stage_log",
                                           "void *stream"],
    "fltee_stable_range_merge_device": ["void *d_rec16", "size_t m", "size_t pos_base",
                                        "uint32_t stage_log", "void *stream"],
    "fltee_stable_range_strip_device": ["const void *d_rec16", "size_t m", "void *d_dst8", "void *stream"],
}


@pytest.fixture(scope="module")
def lib():
    from fltee import _lib as L
    return L.lib()


def test_the_five_symbols_are_declared_exported_and_bound():
    from fltee import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = L.lib()
    for name, args in ARGS.items():
        m = re.search(r"fltee_status_t\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in fltee_agg.h"
        declared = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert declared == args, name
        assert hasattr(lib, name), f"{name} is not exported"
        res, argtypes = L.SIGNATURES[name]
        assert len(argtypes) == len(args) and res is L._U32, name


def init(lib, nrec, d, pos, m):
    return lib.fltee_stable_init_range_device(None, nrec, d, pos, m, None, None)


def sort(lib, pos, m, valid=1):
    return lib.fltee_stable_range_sort_device(None, m, pos, valid, None)


def merge(lib, pos, m, stage):
    return lib.fltee_stable_range_merge_device(None, m, pos, stage, None)


def exch(lib, mine, theirs, m, stage):
    return lib.fltee_stable_range_exchange_device(None, None, m, mine, theirs, stage, None)


def strip(lib, m):
    return lib.fltee_stable_range_strip_device(None, m, None, None)


@pytest.mark.parametrize("m", [0, 1, T - 1, T + 1, 3 * T, T // 2, 2, BIG + 1, 2 * BIG, 1 << 40])
def test_a_bad_range_length_is_refused_by_every_piece(lib, m):
    """m not a power of two, below one LDS tile (2^12) or above 2^29"""
    assert init(lib, 10, 10, 0, m) == INVALID
    assert sort(lib, 0, m) == INVALID
    assert merge(lib, 0, m, 31) == INVALID
    assert exch(lib, 0, m, m, 31) == INVALID
    assert strip(lib, m) == INVALID


@pytest.mark.parametrize("m,pos", [(T, 1), (T, T - 1), (T, T + T // 2), (2 * T, T), (2 * T, 3 * T),
                                   (BIG, T)])
def test_a_position_that_is_no_multiple_of_m_is_refused(lib, m, pos):
    assert init(lib, 10, 10, pos, m) == INVALID
    assert sort(lib, pos, m) == INVALID
    assert merge(lib, pos, m, 31) == INVALID
    assert exch(lib, pos, pos ^ m, m, 31) == INVALID    # pos_mine
    assert exch(lib, 4 * m, pos, m, 31) == INVALID      # pos_theirs


@pytest.mark.parametrize("m,pos", [(T, 1 << 31), (BIG, 1 << 31), (T, (1 << 31) + T), (2 * T, 1 << 32),
                                   (T, (1 << 63) + T)])
def test_a_range_ending_past_2_31_is_refused(lib, m, pos):
    assert init(lib, 10, 10, pos, m) == INVALID
    assert sort(lib, pos, m) == INVALID
    assert merge(lib, pos, m, 31) == INVALID
    assert exch(lib, pos, pos - m, m, 31) == INVALID
    assert exch(lib, pos - m, pos, m, 31) == INVALID


def test_exchange_refusals(lib):
    for m in (T, 4 * T):
        assert exch(lib, 2 * m, 2 * m, m, 20) == INVALID            # the same range
        assert exch(lib, 0, 3 * m, m, 20) == INVALID                # distance 3 m: no power of two
        assert exch(lib, m, 7 * m, m, 20) == INVALID                # distance 6 m
        assert exch(lib, m, 2 * m, m, 20) == INVALID                # distance m, but two bits differ
        mlog = m.bit_length() - 1
        for j in (0, 1, 3):                                         # distance m << j
            a, b = 0, m << j
            assert exch(lib, a, b, m, mlog + j) == INVALID          # stage = the distance
            assert exch(lib, b, a, m, mlog + j) == INVALID
            assert exch(lib, a, b, m, mlog + j - 1) == INVALID      # below it
            assert exch(lib, a, b, m, 0) == INVALID
        assert exch(lib, 0, m, m, 32) == INVALID                    # no such stage below 2^31


def test_merge_refusals(lib):
    for m in (T, 8 * T):
        mlog = m.bit_length() - 1
        for stage in (0, 1, mlog - 1, mlog, 32, 40):
            assert merge(lib, 0, m, stage) == INVALID, (m, stage)
            assert merge(lib, 2 * m, m, stage) == INVALID, (m, stage)


def test_init_refuses_an_array_past_2_31_entries(lib):
    assert init(lib, (1 << 31) - 5, 5, 0, T) == INVALID
    assert init(lib, 1 << 31, 0, 0, T) == INVALID
    assert init(lib, 0, 1 << 31, 0, T) == INVALID
    assert init(lib, 1 << 63, 1 << 63, 0, T) == INVALID             # (the sum wraps to 0)
