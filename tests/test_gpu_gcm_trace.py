"""The authenticated ECALL's launch trace, up to and including the fail-word readback, is a
function of the public sizes alone (the helpers of tests/test_gpu_oblivious.py): random
uploads, adversarial uploads (every record on one index) and a tampered upload of the same
sizes give the same lines — every launch (site, grid, block, LDS), copy, memset and sync of
the key upload, the powers of H, the CTR decryption, GHASH and the tag check."""
import numpy as np
import pytest

from conftest import gpu_available
from test_gpu_oblivious import assert_same_trace, traced, uploads

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

READBACK = "memcpy||4|2|0"  # the 4-byte device-to-host copy of the word gathering the failures


def through_readback(lines):
    last = max(i for i, line in enumerate(lines) if "ghash_finish_kernel" in line)
    i = lines.index(READBACK, last)
    assert lines[i + 1].startswith("sync|stream"), lines[i + 1]
    return lines[:i + 2]


@pytest.mark.parametrize("alg", [1, 6])
@pytest.mark.parametrize("n,d,k", [(5, 3000, 300), (40, 60000, 1500)])  # one and two segments
def test_aead_ecall_trace_is_data_independent(oracle, alg, n, d, k):
    import torch

    from fltee import client as C
    from fltee.ecalls import Enclave, set_upload_aead
    torch.cuda.init()
    ids = np.arange(40, 40 + n, dtype=np.uint32)
    fl = 8600 + alg
    encs = []
    for i, kind in enumerate(("random", "one_index")):
        idx, val = uploads(np.random.default_rng(60 + i), n, d, k, kind)
        rec = torch.from_numpy(oracle.as_weights(idx, val).view(np.int64).copy()).cuda()
        encs.append(C.encrypt_parameters_auth(rec, ids, fl, 0, alg).cpu().numpy())
    tampered = encs[0].copy()
    tampered[(n - 1) * (k * 8 + 16) + 5] ^= 0x10
    E = Enclave(0)

    def call(enc, want):
        assert E.ecall_fl_init(fl, ids, d, k, 1.12, 1.0, 0.1, 1.0, alg, 0, 0) == (0, 0)
        assert E.ecall_start_round(fl, 0, n)[:2] == (0, 0)
        if alg == 6:
            st, rv, _, _ = E.ecall_client_size_optimized_secure_aggregation(fl, 0, 7, ids, enc, d, k, alg)
        else:
            st, rv, _, _ = E.ecall_secure_aggregation(fl, 0, ids, enc, d, k, alg)
        assert (st, rv) == (0, want)

    set_upload_aead(True)
    try:
        call(encs[0], 0)  # the shape's scratch
        tr = [traced(lambda e=e, w=w: call(e, w)) for e, w in ((encs[0], 0), (encs[1], 0), (tampered, 0x3001))]
    finally:
        set_upload_aead(False)
        E.destroy()
    assert any("ghash_bulk_kernel" in line for line in tr[0]) and any("ghash_powers_kernel" in line for line in tr[0])
    assert_same_trace(tr[0], tr[1], f"authenticated ECALL alg {alg} n={n}: one_index")
    head = through_readback(tr[0])
    assert_same_trace(head, through_readback(tr[2]), f"authenticated ECALL alg {alg} n={n}: tampered")
    assert tr[2] == head, "nothing is launched after a failed batch"
