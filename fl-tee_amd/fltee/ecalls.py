"""Host-side mirror of secure_aggregation/app/src/ecalls.rs over the C ABI.

`Enclave` replaces `init_enclave()` / `SgxEnclave` (ecalls.rs:66-83) and
exposes the four ECALLs with the argument meaning of ecalls.rs:6-64.  Each
method returns `(bridge_status, retval, ...)` exactly like the Rust host sees
them (`result`, `retval`): the server panics unless both are SUCCESS
(server.rs:80-82,96-98,159-161,180-182,202-204).
"""
import ctypes

import numpy as np

from . import _lib as L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _as_u8(buf):
    """bytes / bytearray / numpy array -> flat uint8 view (no copy of large payloads)."""
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return np.frombuffer(buf, dtype=np.uint8)
    return np.frombuffer(bytes(buf), dtype=np.uint8)  # e.g. fl_main.py's list of ints


class Enclave:
    """device: one HIP device id, or a list of them for an eid over several GPUs
    (fltee_device_init_multi: the ECALLs shard internally; the same id repeated gives
    virtual ranks on one GPU)."""

    def __init__(self, device=0):
        self.lib = L.lib()
        eid = ctypes.c_uint64(0)
        if isinstance(device, (list, tuple)):
            devs = (ctypes.c_int * len(device))(*device)
            st = self.lib.fltee_device_init_multi(devs, len(device), ctypes.byref(eid))
        else:
            st = self.lib.fltee_device_init(device, ctypes.byref(eid))
        if st != L.SUCCESS:
            raise RuntimeError(f"fltee_device_init({device}) failed: {st:#x}")
        self.eid = eid.value

    def device_count(self):
        return self.lib.fltee_device_count(self.eid)

    def geteid(self):
        return self.eid

    def destroy(self):
        if self.eid:
            self.lib.fltee_device_fini(self.eid)
            self.eid = 0

    # lib.rs:113-180
    def ecall_fl_init(self, fl_id, client_ids, num_of_parameters, num_of_sparse_parameters,
                      sigma, clipping, alpha, sampling_ratio, aggregation_alg, verbose, dp):
        ids = np.ascontiguousarray(client_ids, dtype=np.uint32)
        rv = ctypes.c_uint32(0xFFFFFFFF)
        st = self.lib.ecall_fl_init(self.eid, ctypes.byref(rv), fl_id, _p(ids), len(ids),
                                    num_of_parameters, num_of_sparse_parameters, sigma, clipping,
                                    alpha, sampling_ratio, aggregation_alg, int(verbose), int(dp))
        return st, rv.value

    # lib.rs:182-219
    def ecall_start_round(self, fl_id, round_, sample_size):
        out = np.zeros(max(sample_size, 1), dtype=np.uint32)
        rv = ctypes.c_uint32(0xFFFFFFFF)
        st = self.lib.ecall_start_round(self.eid, ctypes.byref(rv), fl_id, round_, sample_size,
                                        _p(out))
        return st, rv.value, out[:sample_size]

    # lib.rs:221-423
    def ecall_secure_aggregation(self, fl_id, round_, client_ids, encrypted_parameters,
                                 num_of_parameters, num_of_sparse_parameters, aggregation_alg):
        ids = np.ascontiguousarray(client_ids, dtype=np.uint32)
        enc = _as_u8(encrypted_parameters)
        out = np.empty(num_of_parameters, dtype=np.float32)  # written whole by the call
        times = np.full(3, np.nan, dtype=np.float32)
        rv = ctypes.c_uint32(0xFFFFFFFF)
        st = self.lib.ecall_secure_aggregation(
            self.eid, ctypes.byref(rv), fl_id, round_, _p(ids), len(ids), _p(enc), enc.nbytes,
            num_of_parameters, num_of_sparse_parameters, aggregation_alg, _p(out), _p(times))
        return st, rv.value, out, times

    # lib.rs:425-592
    def ecall_client_size_optimized_secure_aggregation(self, fl_id, round_, optimal_num_of_clients,
                                                       client_ids, encrypted_parameters,
                                                       num_of_parameters, num_of_sparse_parameters,
                                                       aggregation_alg):
        ids = np.ascontiguousarray(client_ids, dtype=np.uint32)
        enc = _as_u8(encrypted_parameters)
        need = len(ids) * (num_of_sparse_parameters * 8 + (L.GCM_TAG_BYTES if _upload_aead else 0))
        if enc.nbytes < need:  # [user_check]: the enclave would read past the buffer
            raise ValueError(f"payload has {enc.nbytes} bytes, alg 6 reads {need}")
        out = np.full(num_of_parameters, np.nan, dtype=np.float32)
        times = np.full(3, np.nan, dtype=np.float32)
        rv = ctypes.c_uint32(0xFFFFFFFF)
        st = self.lib.ecall_client_size_optimized_secure_aggregation(
            self.eid, ctypes.byref(rv), fl_id, round_, optimal_num_of_clients, _p(ids), len(ids),
            _p(enc), num_of_parameters, num_of_sparse_parameters, aggregation_alg, _p(out),
            _p(times))
        return st, rv.value, out, times

    def set_dense_trim(self, per_mille):
        """fltee_set_dense_trim (process-wide; see the module function of the same name)."""
        set_dense_trim(per_mille)

    def set_dense_krum(self, f, m):
        """fltee_set_dense_krum (process-wide; see the module function of the same name)."""
        set_dense_krum(f, m)

    def set_dense_gmed(self, iters, nu=2.0 ** -20):
        """fltee_set_dense_gmed (process-wide; see the module function of the same name)."""
        set_dense_gmed(iters, nu)

    def set_dense_trim_select(self, on):
        """fltee_set_dense_trim_select (process-wide; see the module function of the same name)."""
        set_dense_trim_select(on)

    def auth_report(self, fl_id):
        """fltee_auth_report: (round, [failed client ids in upload order]) of fl_id's last
        authenticated ECALL under the "report" / "drop" policies; an empty list after a clean
        call, and when nothing was stored."""
        rnd, n = ctypes.c_uint32(0), ctypes.c_size_t(0)
        st = self.lib.fltee_auth_report(self.eid, fl_id, ctypes.byref(rnd), None, 0, ctypes.byref(n))
        ids = np.zeros(max(n.value, 1), dtype=np.uint32)
        if st == L.SUCCESS and n.value:
            st = self.lib.fltee_auth_report(self.eid, fl_id, ctypes.byref(rnd), _p(ids), n.value,
                                            ctypes.byref(n))
        if st != L.SUCCESS:
            raise RuntimeError(f"fltee_auth_report({fl_id}) failed: {st:#x}")
        return rnd.value, [int(x) for x in ids[:n.value]]


def set_debug_seed(seed):
    """Deterministic RNG for sampling / nips19 / DP (tests only; 0 restores RDRAND-like)."""
    L.lib().fltee_debug_set_seed(seed)


def set_path_oram_tree(on):
    """aggregation_alg 5 through the ECALLs: the tree Path ORAM (oram.rs:64-118) when on, the
    output-equivalent oblivious sweep (default) when off (fltee_set_path_oram_tree)."""
    L.lib().fltee_set_path_oram_tree(1 if on else 0)


_upload_aead = False


def set_upload_aead(on):
    """The ECALLs' upload format: plain AES-128-CTR when off (default, lib.rs:312-343);
    AES-128-GCM when on — a client's slice is ciphertext || 16-byte tag under IV = BE32(fl_id)
    || BE32(round) || BE32(0) and AAD = BE32(fl_id) || BE32(round) || BE32(client_id) ||
    BE32(aggregation_alg) (fltee.client.encrypt_parameters_auth builds it); a slice that does
    not verify ends the ECALL with retval 0x3001 (fltee_set_upload_aead)."""
    global _upload_aead
    L.lib().fltee_set_upload_aead(1 if on else 0)
    _upload_aead = bool(on)


def set_upload_packed(on):
    """Packed dense uploads (fltee_set_upload_packed; off by default): while on, an
    ecall_secure_aggregation call whose request declares a dense upload (num_of_sparse_parameters
    0 or d, d >= 2) and whose clients each send exactly 8 * ceil(d / 2) ciphertext bytes (plus
    the tag under AEAD) is read as value-only slices (fltee.client.pack_dense /
    produce_payloads(packed=True)): half the bytes, the same [out] bit for bit.  Every other
    call — a dense 8 * d-byte upload too — is read as records, as before."""
    L.lib().fltee_set_upload_packed(1 if on else 0)


def set_dense_trim(per_mille):
    """Robust aggregation (fltee_set_dense_trim; 0, the default, is off): while on, a dense or
    packed ecall_secure_aggregation call on algs 3, 4, 5 returns the coordinate-wise trimmed mean
    — per coordinate the t = trim_count(n', per_mille) smallest and the t largest client values
    are removed (a NaN is always an extreme) and the rest averaged over n' - 2 t; 500 asks for
    the median.  Every call that cannot be trimmed (algs 1, 2, 6, 7, a sparse upload, the tree)
    ends with retval 0x2, never with an untrimmed mean."""
    if not 0 <= int(per_mille) <= 500:
        raise ValueError(f"trim per mille {per_mille!r} is not in 0..500")
    L.lib().fltee_set_dense_trim(int(per_mille))


def set_dense_trim_select(on):
    """Trim by selection (fltee_set_dense_trim_select; off by default): while on, a call under
    set_dense_trim whose trim count exceeds TRIM_MAX (the median from 131 clients on) is answered
    by the selection kernel for up to TRIM_SELECT_MAX_N clients instead of ending with 0x2; a
    call with a trim count up to TRIM_MAX runs as before."""
    L.lib().fltee_set_dense_trim_select(1 if on else 0)


def set_dense_krum(f, m):
    """Multi-Krum (fltee_set_dense_krum; (0, 0), the default, is off): while on, a dense or packed
    ecall_secure_aggregation call on algs 3, 4, 5 scores every client by the squared distances to
    its n' - f - 2 nearest neighbours and returns the mean of the m best-scored clients, whole.
    Every call that cannot be answered so (algs 1, 2, 6, 7, a sparse upload, the tree,
    n' < 2 f + 3, m > n' - f, more than KRUM_MAX_N clients, set_dense_trim on as well) ends with
    retval 0x2, never with a plain mean."""
    f, m = int(f), int(m)
    if f < 0 or m < 0 or f >= 2 ** 32 or m >= 2 ** 32:
        raise ValueError(f"krum (f, m) = ({f}, {m}) is not a pair of u32")
    L.lib().fltee_set_dense_krum(f, m)


def set_dense_gmed(iters, nu=2.0 ** -20):
    """The geometric median (fltee_set_dense_gmed; iters = 0, the default, is off): while on, a dense
    or packed ecall_secure_aggregation call on algs 3, 4, 5 returns the smoothed Weiszfeld iterate
    after `iters` iterations — every valid client weighted by 1 / max(nu, its distance to the
    iterate), the weights normalised to one.  Every call that cannot be answered so (algs 1, 2, 6,
    7, a sparse upload, the tree, more than KRUM_MAX_N clients, more than GMED_MAX_ITERS iterations,
    a nu that is not a finite value above 0, set_dense_trim or set_dense_krum on as well) ends with
    retval 0x2, never with a plain mean."""
    iters, nu = int(iters), float(nu)
    if iters < 0 or iters >= 2 ** 32:
        raise ValueError(f"gmed iters = {iters} is not a u32")
    L.lib().fltee_set_dense_gmed(iters, nu)


def trim_count(n, per_mille):
    """fltee_trim_count: min(n * per_mille // 1000, (n - 1) // 2) clients trimmed on each side."""
    return int(L.lib().fltee_trim_count(n, per_mille))


def upload_is_packed(on, d, k_req, ct_bytes):
    """fltee_upload_is_packed: the packed-call rule on one client's ciphertext bytes."""
    return bool(L.lib().fltee_upload_is_packed(1 if on else 0, d, k_req, ct_bytes))


def set_upload_bf16(on):
    """bf16 dense uploads (fltee_set_upload_bf16; off by default): while on, an
    ecall_secure_aggregation call whose request declares a dense upload (num_of_sparse_parameters
    0 or d, d >= 3) and whose clients each send exactly 8 * ceil(d / 4) ciphertext bytes (plus
    the tag under AEAD) is read as bf16 slices (fltee.client.pack_dense_bf16 /
    produce_payloads(bf16=True)): a quarter of the bytes, [out] the in-order f32 sum of the
    widened values bit for bit.  Every other call is read as before; with set_upload_packed on
    too, one server answers records, packed and bf16 uploads by their size."""
    L.lib().fltee_set_upload_bf16(1 if on else 0)


def upload_is_bf16(on, d, k_req, ct_bytes):
    """fltee_upload_is_bf16: the bf16-call rule on one client's ciphertext bytes."""
    return bool(L.lib().fltee_upload_is_bf16(1 if on else 0, d, k_req, ct_bytes))


def set_upload_fp8(on):
    """fp8 dense uploads (fltee_set_upload_fp8; off by default): while on, an
    ecall_secure_aggregation call that declares a dense upload of d >= 13 parameters and
    carries 8 * (ceil(d / 8) + 1) bytes per client (plus the tag under AEAD) is read as fp8
    slices (fltee.client.pack_dense_fp8 / produce_payloads(fp8=True)): e4m3fn codes and one f32
    scale per client, [out] the in-order f32 sum of the values code * scale, bit for bit what
    they give as records.  With set_upload_packed and set_upload_bf16 on too, one server answers
    records, packed, bf16 and fp8 uploads by their size."""
    L.lib().fltee_set_upload_fp8(1 if on else 0)


def upload_is_fp8(on, d, k_req, ct_bytes):
    """fltee_upload_is_fp8: the fp8-call rule on one client's ciphertext bytes."""
    return bool(L.lib().fltee_upload_is_fp8(1 if on else 0, d, k_req, ct_bytes))


AEAD_POLICIES = {"abort": L.AEAD_ABORT, "report": L.AEAD_REPORT, "drop": L.AEAD_DROP}


def set_upload_aead_policy(policy, min_survivors=1):
    """What an authenticated ECALL does after a failed tag (fltee_set_upload_aead_policy;
    no effect while AEAD is off).  policy: "abort" (default: 0x3001, nothing more), "report"
    (0x3001, and Enclave.auth_report names the failed clients) or "drop" (the verified
    clients are aggregated, with n' in every divisor, when at least min_survivors verified;
    else as "report"), or the FLTEE_AEAD_* value."""
    code = AEAD_POLICIES[policy] if isinstance(policy, str) else int(policy)
    if code not in AEAD_POLICIES.values():
        raise ValueError(f"unknown AEAD policy {policy!r}")
    L.lib().fltee_set_upload_aead_policy(code, int(min_survivors))


def set_bubble_ecall(on):
    """aggregation_alg 7 (lib.rs:389) through ecall_secure_aggregation: refused with 0x2 when
    off (default), answered with the enclave's in-order result when on
    (fltee_set_bubble_ecall)."""
    L.lib().fltee_set_bubble_ecall(1 if on else 0)


def set_advanced_exact_runs(on):
    """aggregation_alg 1 and 6 through the ECALLs when some index has a run of more than
    n + 1 entries (a client repeated an index): off (default) answers at the fixed cost of
    the halo fold plus its long-run carry (that run's sum re-associated at the walk
    boundaries); on folds any run exactly, as advanced.rs:66-101 does, at the public
    worst-case cost (fltee_set_advanced_exact_runs)."""
    L.lib().fltee_set_advanced_exact_runs(1 if on else 0)
