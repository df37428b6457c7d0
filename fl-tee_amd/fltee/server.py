"""The Aggregator service logic of secure_aggregation/app/src/server.rs, over the C ABI.

`Aggregator.start` / `Aggregator.aggregate` take and return exactly the fields of
proto/secure_aggregation.proto's StartRequestParameters / AggregateRequestParameters
(and the response messages), so a gRPC front end only has to (de)serialise.  Where
server.rs panics, these raise `ServerPanic` (a tonic handler panic aborts the
request).  Documented deviations from the reference host:

  * server.rs:126-128 rejects `optimal_num_of_clients > |client_ids|` for EVERY
    algorithm, which kills fl_main.py's defaults (n=30 < 100) for algs 1-5.  The
    check is applied only when aggregation_alg == 6 (`strict_reference=True`
    restores the reference behaviour).
  * server.rs:237 hard-wires dp = false; here it is a constructor argument.
  * `aead=True` (off by default) switches the uploads to AES-128-GCM: the request's
    encrypted_parameters then carries ciphertext || 16-byte tag per client (the proto is
    unchanged), and a slice that does not verify is a ServerPanic naming the MAC mismatch.
  * `aead_policy` (with `aead=True`): "abort" (default) as above; "report": the same panic,
    and the clients whose slices failed are kept in `last_failed_clients` and logged;
    "drop": the verified clients are aggregated (the averages take their count) as long as
    `min_survivors` of them verified, the failed ones kept and logged the same way.  The
    reply has no field for the list (the proto is unchanged): the host reads it here.
  * `packed=True` (off by default) accepts packed dense uploads: a request that declares a
    dense upload and carries 8 * ceil(d / 2) bytes per client (value-only slices,
    fltee.client.pack_dense) is aggregated from half the bytes, with the same reply; every
    other request, a dense 8 * d-byte one too, is answered as before.
  * `bf16=True` (off by default) accepts bf16 dense uploads: a request that declares a dense
    upload of d >= 3 parameters and carries 8 * ceil(d / 4) bytes per client (bf16 slices,
    fltee.client.pack_dense_bf16) is aggregated from a quarter of the bytes — the in-order f32
    sum of the values as sent; every other request is answered as before, and with `packed`
    on too one server answers all three formats.
  * `fp8=True` (off by default) accepts fp8 dense uploads: a request that declares a dense
    upload of d >= 13 parameters and carries 8 * (ceil(d / 8) + 1) bytes per client (e4m3fn
    codes and one f32 scale, fltee.client.pack_dense_fp8) is aggregated from an eighth of the
    bytes — the in-order f32 sum of the values code * scale; every other request is answered as
    before, and with `packed` and `bf16` on too one server answers all four formats.
  * `trim_per_mille=N` (0, off, by default; 0..500) answers dense uploads to algs 3, 4, 5 with
    the coordinate-wise trimmed mean: per coordinate the N per mille smallest and largest
    client values are removed (500: the median), so a client sealing 1e30 or NaN no longer
    owns the round.  Every request that cannot be trimmed (another alg, a sparse upload) is a
    ServerPanic (retval 0x2), never an untrimmed mean.
  * `trim_select=True` (off by default) lets `trim_per_mille` trim more than 64 clients a side
    (the median from 131 clients on, up to 4096 clients): such a request is answered by the
    selection kernel instead of refused; requests that trim up to 64 run as before.
  * `krum=(f, m)` (None, off, by default) answers dense uploads to algs 3, 4, 5 with Multi-Krum:
    every client is scored by the squared distances to its n - f - 2 nearest neighbours and the
    m best-scored clients are averaged whole.  An alternative to `trim_per_mille` (both on: every
    request is refused); a request that cannot be answered so is a ServerPanic (retval 0x2),
    never a plain mean.
  * `gmed=(iters, nu)` (None, off, by default) answers dense uploads to algs 3, 4, 5 with the
    geometric median (RFA): `iters` smoothed Weiszfeld iterations with the floor `nu`, every valid
    client kept with a smooth weight.  An alternative to `trim_per_mille` and `krum`; a request that
    cannot be answered so is a ServerPanic (retval 0x2), never a plain mean.
"""
import argparse
import time

from . import _lib as L
from .ecalls import (AEAD_POLICIES, Enclave, set_dense_gmed, set_dense_krum, set_dense_trim, set_dense_trim_select, set_upload_aead,
                     set_upload_aead_policy, set_upload_bf16, set_upload_fp8, set_upload_packed)


class ServerPanic(RuntimeError):
    pass


def per_mille(text):
    """argparse type of --trim-per-mille: an integer in 0..500"""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not an integer")
    if not 0 <= v <= 500:
        raise argparse.ArgumentTypeError(f"{v} is not in 0..500")
    return v


class Aggregator:
    def __init__(self, device=0, verbose=False, dp=False, strict_reference=False, enclave=None,
                 aead=False, aead_policy="abort", min_survivors=1, packed=False, trim_per_mille=0,
                 bf16=False, trim_select=False, fp8=False, krum=None, gmed=None):
        if aead_policy not in AEAD_POLICIES:
            raise ValueError(f"aead_policy must be one of {sorted(AEAD_POLICIES)}")
        if aead_policy != "abort" and not aead:
            raise ValueError("aead_policy needs aead=True")
        self.enclave = enclave if enclave is not None else Enclave(device)
        self.aead = bool(aead)
        self.aead_policy = aead_policy
        self.last_failed_clients = []  # of the last aggregate, under "report" / "drop"
        if self.aead:  # process-wide, like the enclave's other start-up switches
            set_upload_aead(True)
            set_upload_aead_policy(aead_policy, min_survivors)
        self.packed = bool(packed)
        if self.packed:  # process-wide too
            set_upload_packed(True)
        self.bf16 = bool(bf16)
        if self.bf16:  # process-wide too
            set_upload_bf16(True)
        self.fp8 = bool(fp8)
        if self.fp8:  # process-wide too
            set_upload_fp8(True)
        self.trim_per_mille = int(trim_per_mille)
        if not 0 <= self.trim_per_mille <= 500:
            raise ValueError("trim_per_mille must be in 0..500")
        if self.trim_per_mille:  # process-wide too
            set_dense_trim(self.trim_per_mille)
        self.trim_select = bool(trim_select)
        if self.trim_select:  # process-wide too
            set_dense_trim_select(True)
        self.krum = tuple(int(v) for v in krum) if krum is not None else None
        if self.krum is not None:  # process-wide too
            set_dense_krum(*self.krum)
        self.gmed = (int(gmed[0]), float(gmed[1])) if gmed is not None else None
        if self.gmed is not None:  # process-wide too
            set_dense_gmed(*self.gmed)
        self.verbose = verbose
        self.dp = dp
        self.strict_reference = strict_reference

    # server.rs:44-108
    def start(self, fl_id, client_ids, sigma, clipping, alpha, sampling_ratio, aggregation_alg,
              num_of_parameters, num_of_sparse_parameters):
        st, rv = self.enclave.ecall_fl_init(fl_id, client_ids, num_of_parameters,
                                            num_of_sparse_parameters, sigma, clipping, alpha,
                                            sampling_ratio, aggregation_alg, self.verbose, self.dp)
        if st != L.SUCCESS or rv != L.SUCCESS:
            raise ServerPanic("Error at ecall_fl_init")
        import numpy as np
        sample_size = int(np.float32(sampling_ratio) * np.float32(len(client_ids)))  # f32 then as usize
        st, rv, sampled = self.enclave.ecall_start_round(fl_id, 0, sample_size)
        if st != L.SUCCESS or rv != L.SUCCESS:
            raise ServerPanic("Error at ecall_start_round")
        return dict(fl_id=fl_id, round=0, client_ids=[int(x) for x in sampled])

    def _note_failed_clients(self, fl_id, round, st, rv):
        """under "report" / "drop", after an ECALL that reached its verdict (answered, or a
        MAC mismatch): keep and log the clients whose slices did not verify"""
        if not self.aead or self.aead_policy == "abort" or st != L.SUCCESS:
            return
        if rv not in (L.SUCCESS, L.ERROR_MAC_MISMATCH):
            return
        rnd, failed = self.enclave.auth_report(fl_id)
        if rnd == round and failed:
            self.last_failed_clients = failed
            print(f"[Server] fl_id={fl_id} round={round}: {len(failed)} client(s) failed "
                  f"authentication: {failed}", flush=True)

    # server.rs:111-215
    def aggregate(self, fl_id, round, encrypted_parameters, num_of_parameters,
                  num_of_sparse_parameters, optimal_num_of_clients, aggregation_alg, client_ids):
        if optimal_num_of_clients > len(client_ids) and (self.strict_reference or aggregation_alg == 6):
            raise ServerPanic(f"optimal_num_of_clients is more than client size {len(client_ids)}")
        t0 = time.perf_counter()
        self.last_failed_clients = []
        if aggregation_alg == 6:
            st, rv, out, times = self.enclave.ecall_client_size_optimized_secure_aggregation(
                fl_id, round, optimal_num_of_clients, client_ids, encrypted_parameters,
                num_of_parameters, num_of_sparse_parameters, aggregation_alg)
            self._note_failed_clients(fl_id, round, st, rv)
            if st == L.SUCCESS and rv == L.ERROR_MAC_MISMATCH:
                raise ServerPanic("MAC mismatch at ecall_client_size_optimized_secure_aggregation")
            if st != L.SUCCESS or rv != L.SUCCESS:
                raise ServerPanic("Error at ecall_client_size_optimized_secure_aggregation")
        else:
            st, rv, out, times = self.enclave.ecall_secure_aggregation(
                fl_id, round, client_ids, encrypted_parameters, num_of_parameters,
                num_of_sparse_parameters, aggregation_alg)
            self._note_failed_clients(fl_id, round, st, rv)
            if st == L.SUCCESS and rv == L.ERROR_MAC_MISMATCH:
                raise ServerPanic("MAC mismatch at ecall_secure_aggregation")
            if st != L.SUCCESS or rv != L.SUCCESS:
                raise ServerPanic("Error at ecall_secure_aggregation")
        elapsed = time.perf_counter() - t0
        # "Assuming that the next round is the same number of participants." (server.rs:188)
        st, rv, sampled = self.enclave.ecall_start_round(fl_id, round + 1, len(client_ids))
        if st != L.SUCCESS or rv != L.SUCCESS:
            raise ServerPanic("[Server] Error at ecall_start_round")
        return dict(updated_parameters=out, execution_time=float(elapsed),
                    client_ids=[int(x) for x in sampled], round=round + 1,
                    enclave_times=times)
