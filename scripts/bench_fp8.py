"""fp8 dense uploads (FLTEE_OPT_FP8, fltee_set_upload_fp8) against records, packed slices and bf16
slices in ONE process.  Records and packed slices carry the values the fp8 slices stand for
(code * scale), so their [out] is compared bit for bit first; the bf16 slices carry those values
narrowed once more (the same bytes per parameter as any bf16 upload: a timing, not a comparison).

    python scripts/bench_fp8.py [--shapes headline,c3] [--warmup 2] [--reps 5]
                                [--eager] [--no-ecall] [--out FILE]

device  per shape (headline: 100 x 1M; c3 = configs[2] dense: 100 x 50,890): alg 3 on records,
        packed rows, bf16 rows and fp8 rows, and the streaming-read floor (fltee_debug_read_floor)
        over each buffer: warm-up calls, then `reps` interleaved event-timed groups of `inner`
        calls of each (a group is captured once as a graph and replayed; --eager launches from the
        host); medians per call.  Every call reads a copy of its input that the calls before it
        have pushed out of the 256 MB Infinity Cache (the copies rotate).
ecall   the host-inclusive alg-3 ECALL at 100 x 1M from pageable host memory, the four formats,
        CTR and AEAD: wall time and the call's three timers, medians of `reps` interleaved calls.
One JSON line per measurement, appended to profiles/r16/fp8.jsonl by default.  A session is one
run of this script in a fresh process; DESIGN says how many sessions its figures rest on."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fl-tee_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_packed import CACHE_BYTES, SHAPES, emit, timed_groups  # noqa: E402

FORMATS = ("records", "packed", "bf16", "fp8")
OPT = {"records": dict(dense=True), "packed": dict(packed=True), "bf16": dict(bf16=True), "fp8": dict(fp8=True)}


def fp8_values(torch, C, D, n, d, scale=1.0):
    """(fp8 rows, the values they stand for as f32 [n, d])"""
    rows = C.pack_dense_fp8(torch.randn((n, d), device="cuda", dtype=torch.float32) * scale)
    rec = D.unpack_fp8(rows, n, d)
    x = rec.view(torch.float32).reshape(n, d, 2)[:, :, 1].contiguous()
    return rows, x


def device_rows(args, torch, np, L, C, D, name):
    n, d = SHAPES[name]
    lib = L.lib()
    nbytes = {"records": n * d * 8, "packed": n * D.packed_row(d) * 4, "bf16": n * D.bf16_row(d) * 2,
              "fp8": n * D.fp8_row(d)}
    rows, x = fp8_values(torch, C, D, n, d)
    make = {"records": lambda: C.serialize_dense(x), "packed": lambda: C.pack_dense(x),
            "bf16": lambda: C.pack_dense_bf16(x), "fp8": lambda: rows.clone()}
    bufs = {f: [make[f]() for _ in range(max(2, -(-CACHE_BYTES // nbytes[f])))] for f in FORMATS}
    del x
    out = torch.empty(d, dtype=torch.float32, device="cuda")
    sink = torch.zeros(4096, dtype=torch.int32, device="cuda")
    turn = {f: 0 for f in FORMATS}

    def nxt(f):
        turn[f] = (turn[f] + 1) % len(bufs[f])
        return bufs[f][turn[f]]

    def floor(f):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # (a capture has its own)
        assert lib.fltee_debug_read_floor(ctypes.c_void_p(nxt(f).data_ptr()), nbytes[f] // 16 * 16,
                                          ctypes.c_void_p(sink.data_ptr()), 2048, stream) == 0

    calls = {f: (lambda f=f: D.aggregate(3, nxt(f), n, d, d, out=out, **OPT[f])) for f in FORMATS}
    for f in FORMATS:
        calls[f + "_floor"] = (lambda f=f: floor(f))
    # the same bits first
    ref = D.aggregate(3, bufs["records"][0], n, d, d, dense=True)
    for f in ("packed", "fp8"):
        got = D.aggregate(3, bufs[f][0], n, d, d, **OPT[f])
        assert D.status() == 0 and torch.equal(got.view(torch.int32), ref.view(torch.int32)), f
    med, mn = timed_groups(torch, np, calls, args.warmup, args.reps, args.inner, not args.eager)
    emit(args.out, dict(kind="device", shape=name, n=n, d=d, bytes=nbytes,
                        copies={f: len(bufs[f]) for f in FORMATS}, reps=args.reps, inner=args.inner,
                        timing="eager" if args.eager else "graph replay",
                        median_us=med, min_us=mn,
                        tb_per_s={f: nbytes[f] / med[f] / 1e6 for f in FORMATS},
                        floor_over_kernel={f: med[f + "_floor"] / med[f] for f in FORMATS},
                        fp8_over_bf16=med["fp8"] / med["bf16"],
                        fp8_over_records=med["fp8"] / med["records"],
                        version=lib.fltee_version().decode()))


def ecall_rows(args, torch, np, L, C, D):
    from fltee import ecalls as EC
    n, d = SHAPES["headline"]
    ids = np.arange(1, n + 1, dtype=np.uint32)
    rows, x = fp8_values(torch, C, D, n, d, 0.01)
    fl = 9900
    E = EC.Enclave(0)
    plain = {"records": lambda: C.serialize_dense(x), "packed": lambda: C.pack_dense(x),
             "bf16": lambda: C.pack_dense_bf16(x), "fp8": lambda: rows}
    payload = {}
    for f in FORMATS:
        p = plain[f]()
        fmt = {} if f == "records" else {f: True}
        payload[(f, "ctr")] = C.encrypt_parameters(p, ids).cpu().numpy()
        payload[(f, "aead")] = C.encrypt_parameters_auth(p, ids, fl, 0, 3, **fmt).cpu().numpy()
        del p
    del rows, x
    torch.cuda.empty_cache()
    EC.set_upload_packed(True)
    EC.set_upload_bf16(True)
    EC.set_upload_fp8(True)
    outs, wall, timers = {}, {k: [] for k in payload}, {k: [] for k in payload}
    try:
        for rep in range(args.warmup + args.reps):
            for key, enc in payload.items():
                EC.set_upload_aead(key[1] == "aead")
                assert E.ecall_fl_init(fl, ids, d, d, 1.12, 1.0, 0.1, 1.0, 3, 0, 0) == (0, 0)
                assert E.ecall_start_round(fl, 0, n)[:2] == (0, 0)
                t0 = time.perf_counter()
                st, rv, out, times = E.ecall_secure_aggregation(fl, 0, ids, enc, d, d, 3)
                t1 = time.perf_counter()
                assert (st, rv) == (0, 0), (key, st, rv)
                outs[key] = out
                if rep >= args.warmup:
                    wall[key].append((t1 - t0) * 1e3)
                    timers[key].append([float(v) * 1e3 for v in times])
    finally:
        EC.set_upload_aead(False)
        EC.set_upload_packed(False)
        EC.set_upload_bf16(False)
        EC.set_upload_fp8(False)
        E.destroy()
    ref = outs[("records", "ctr")].view(np.uint32)
    assert all(np.array_equal(o.view(np.uint32), ref) for k, o in outs.items() if k[0] != "bf16")
    for key in payload:
        t = np.median(np.array(timers[key]), axis=0)
        emit(args.out, dict(kind="ecall", shape="headline", n=n, d=d, format=key[0], crypto=key[1],
                            payload_bytes=int(payload[key].nbytes), reps=args.reps,
                            wall_ms=float(np.median(wall[key])), wall_min_ms=float(np.min(wall[key])),
                            loading_ms=float(t[0]), decryption_ms=float(t[1]), aggregation_ms=float(t[2]),
                            version=L.lib().fltee_version().decode()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,c3")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per event-timed group")
    ap.add_argument("--eager", action="store_true",
                    help="launch every timed call from the host (default: each group captured once as a "
                         "graph and replayed, so a ~10 us call is not timed at the host's launch rate)")
    ap.add_argument("--no-ecall", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "fp8.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from fltee import _lib as L
    from fltee import client as C
    from fltee import device as D
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for name in args.shapes.split(","):
        if name:
            device_rows(args, torch, np, L, C, D, name)
            torch.cuda.empty_cache()
    if not args.no_ecall:
        ecall_rows(args, torch, np, L, C, D)


if __name__ == "__main__":
    main()
