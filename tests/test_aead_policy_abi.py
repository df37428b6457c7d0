"""The C ABI of the authenticated-upload policy (include/fltee_agg.h: fltee_set_upload_aead_policy,
fltee_auth_report, fltee_gather_clients_device): the symbols are declared, exported and bound
with matching prototypes, the three policy constants agree between the header and the Python
mirror, fltee_auth_report answers an unknown fl_id with 0x1, and every refusal of the gather is
host arithmetic — 0x2 before any device call, so it is checked here without a GPU (the pointers
are never dereferenced: a refused call touches nothing, and an empty keep list returns 0 before
the device is looked at).  The server switch: --aead-policy only together with --aead."""
import ctypes
import re

import pytest

from test_abi import HEADER

UNEXPECTED, INVALID = 0x1, 0x2

ARGS = {  # the header's prototypes, argument by argument
    "fltee_set_upload_aead_policy": ("void", ["int policy", "size_t min_survivors"]),
    "fltee_auth_report": ("fltee_status_t", ["fltee_eid_t eid", "uint32_t fl_id", "uint32_t *round",
                                             "uint32_t *failed_ids", "size_t cap", "size_t *n_failed"]),
    "fltee_gather_clients_device": ("fltee_status_t", ["const void *d_records", "size_t n", "size_t k",
                                                       "const uint32_t *d_keep", "size_t n_keep",
                                                       "void *d_out", "void *stream"]),
}


@pytest.fixture(scope="module")
def lib():
    from fltee import _lib as L
    return L.lib()


def test_the_symbols_are_declared_exported_and_bound(lib):
    from fltee import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (res, args) in ARGS.items():
        m = re.search(re.escape(res) + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in fltee_agg.h"
        declared = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert declared == args, name
        assert hasattr(lib, name), f"{name} is not exported"
        r, argtypes = L.SIGNATURES[name]
        assert len(argtypes) == len(args), name
        assert r is (None if res == "void" else L._U32), name
        for a, t in zip(args, argtypes):  # pointers as pointers, sizes as size_t
            want = L._P if "*" in a else {"size_t": L._S, "int": ctypes.c_int, "uint32_t": L._U32,
                                          "fltee_eid_t": L._U64}[a.split()[0]]
            assert t is want, (name, a)


def test_policy_constants_match_the_header():
    from fltee import _lib as L
    from fltee.ecalls import AEAD_POLICIES
    text = open(HEADER).read()
    for name, py in (("FLTEE_AEAD_ABORT", L.AEAD_ABORT), ("FLTEE_AEAD_REPORT", L.AEAD_REPORT),
                     ("FLTEE_AEAD_DROP", L.AEAD_DROP)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", text)
        assert m and int(m.group(1)) == py, name
    assert (L.AEAD_ABORT, L.AEAD_REPORT, L.AEAD_DROP) == (0, 1, 2)
    assert AEAD_POLICIES == {"abort": 0, "report": 1, "drop": 2}


def test_policy_switch_is_callable_without_a_device(lib):
    from fltee.ecalls import set_upload_aead_policy
    try:
        for p in ("report", "drop", 2, 0):
            set_upload_aead_policy(p, 3)
        with pytest.raises((ValueError, KeyError)):
            set_upload_aead_policy("sometimes")
        with pytest.raises(ValueError):
            set_upload_aead_policy(7)
    finally:
        lib.fltee_set_upload_aead_policy(0, 0)


def test_auth_report_of_an_unknown_fl_id_is_unexpected(lib):
    rnd, n = ctypes.c_uint32(77), ctypes.c_size_t(99)
    ids = (ctypes.c_uint32 * 4)()
    for eid in (0, 1, 12345):
        st = lib.fltee_auth_report(eid, 0xDEAD0001, ctypes.byref(rnd), ids, 4, ctypes.byref(n))
        assert st == UNEXPECTED and n.value == 0
        n.value = 99
    # a null count, or room promised with nowhere to write: 0x2
    assert lib.fltee_auth_report(1, 0xDEAD0001, ctypes.byref(rnd), ids, 4, None) == INVALID
    assert lib.fltee_auth_report(1, 0xDEAD0001, ctypes.byref(rnd), None, 4, ctypes.byref(n)) == INVALID


P = ctypes.c_void_p(0x10000)  # never dereferenced: every call below returns before the device


def gather(lib, rec, n, k, keep, n_keep, out):
    return lib.fltee_gather_clients_device(rec, n, k, keep, n_keep, out, None)


def test_gather_refusals_are_host_arithmetic(lib):
    assert gather(lib, None, 5, 8, P, 3, P) == INVALID      # null records
    assert gather(lib, P, 5, 8, None, 3, P) == INVALID      # null keep
    assert gather(lib, P, 5, 8, P, 3, None) == INVALID      # null out
    assert gather(lib, None, 5, 8, None, 0, None) == INVALID  # ... also with nothing to keep
    assert gather(lib, P, 5, 8, P, 6, P) == INVALID         # n_keep > n
    assert gather(lib, P, 0, 8, P, 1, P) == INVALID
    assert gather(lib, P, 5, 0, P, 3, P) == INVALID         # k == 0
    assert gather(lib, P, 5, 0, P, 0, P) == INVALID
    assert gather(lib, P, 1 << 16, 1 << 15, P, 1, P) == INVALID    # n * k == 2^31
    assert gather(lib, P, 1, 1 << 31, P, 1, P) == INVALID
    assert gather(lib, P, 1 << 40, 1 << 40, P, 1, P) == INVALID    # n * k overflows 64 bits' half
    assert gather(lib, P, (1 << 64) - 1, 2, P, 1, P) == INVALID    # the product wraps
    # an empty keep list of an acceptable shape: nothing to do, 0 before any device call
    assert gather(lib, P, 5, 8, P, 0, P) == 0
    assert gather(lib, P, (1 << 31) - 1, 1, P, 0, P) == 0   # n * k == 2^31 - 1 is inside
    assert gather(lib, P, 0, 8, P, 0, P) == 0


def test_server_switch_needs_aead():
    grpc_server = pytest.importorskip("fltee.grpc_server", reason="needs grpcio")
    with pytest.raises(SystemExit) as e:
        grpc_server.main(["--aead-policy", "drop", "--quiet"])
    assert e.value.code == 2
    from fltee.server import Aggregator
    with pytest.raises(ValueError):
        Aggregator(enclave=object(), aead=False, aead_policy="drop")
    with pytest.raises(ValueError):
        Aggregator(enclave=object(), aead=True, aead_policy="sometimes")
