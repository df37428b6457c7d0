"""Packed dense uploads (FLTEE_OPT_PACKED, fltee_set_upload_packed) against records of the same
values, in ONE process.

    python scripts/bench_packed.py [--shapes headline,c3] [--warmup 2] [--reps 5]
                                   [--eager] [--no-ecall] [--out FILE]

device  per shape (headline: 100 x 1M; c3 = configs[2] dense: 100 x 50,890): alg 3 on records
        (the dense accumulate) and on packed rows (the packed accumulate), and the streaming-
        read floor (fltee_debug_read_floor) over each buffer: warm-up calls, then `reps`
        interleaved event-timed groups of `inner` calls of each (a group is captured once as a
        graph and replayed; --eager launches from the host); medians per call.  Every call
        reads a copy of its input that the calls before it have pushed out of the 256 MB
        Infinity Cache (the copies rotate).
ecall   the host-inclusive alg-3 ECALL at 100 x 1M from pageable host memory, records against
        packed, CTR and AEAD: wall time and the call's three timers, medians of `reps`
        interleaved calls.
One JSON line per measurement, appended to profiles/r11/packed.jsonl by default."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fl-tee_amd"))
sys.path.insert(0, ROOT)

SHAPES = {"headline": (100, 1_000_000), "c3": (100, 50890)}
CACHE_BYTES = 512 << 20  # twice the Infinity Cache: the copies a call rotates through


def emit(out, line):
    text = json.dumps(line)
    print(text, flush=True)
    with open(out, "a") as f:
        f.write(text + "\n")


def timed_groups(torch, np, calls, warmup, reps, inner, graph):
    for _ in range(warmup):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    groups = {}
    for a, c in calls.items():  # a group: `inner` calls back to back
        def eager(c=c):
            for _ in range(inner):
                c()
        groups[a] = eager
        if graph:  # captured once, replayed: the host's launch rate stays out of a ~10 us call
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                eager()
            groups[a] = g.replay
    for g in groups.values():
        g()
    torch.cuda.synchronize()
    times = {a: [] for a in calls}
    for _ in range(reps):
        for a, run in groups.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[a].append(e0.elapsed_time(e1) * 1e3 / inner)  # us per call
    return {a: float(np.median(t)) for a, t in times.items()}, {a: float(np.min(t)) for a, t in times.items()}


def device_rows(args, torch, np, L, C, D, name):
    n, d = SHAPES[name]
    lib = L.lib()
    row = D.packed_row(d)
    rec_bytes, pk_bytes = n * d * 8, n * row * 4
    copies = max(2, -(-CACHE_BYTES // pk_bytes))
    values = torch.randn((n, d), device="cuda", dtype=torch.float32)
    recs = [C.serialize_dense(values) for _ in range(max(2, -(-CACHE_BYTES // rec_bytes)))]
    rows = [C.pack_dense(values) for _ in range(copies)]
    out = torch.empty(d, dtype=torch.float32, device="cuda")
    sink = torch.zeros(4096, dtype=torch.int32, device="cuda")
    turn = {"rec": 0, "pk": 0}

    def nxt(what, bufs):
        turn[what] = (turn[what] + 1) % len(bufs)
        return bufs[turn[what]]

    def floor(bufs, what, nbytes):
        b = nxt(what, bufs)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # (a capture has its own)
        assert lib.fltee_debug_read_floor(ctypes.c_void_p(b.data_ptr()), nbytes // 16 * 16,
                                          ctypes.c_void_p(sink.data_ptr()), 2048, stream) == 0

    calls = {"records": lambda: D.aggregate(3, nxt("rec", recs), n, d, d, out=out, dense=True),
             "records_floor": lambda: floor(recs, "rec", rec_bytes),
             "packed_floor": lambda: floor(rows, "pk", pk_bytes),
             "packed": lambda: D.aggregate(3, nxt("pk", rows), n, d, d, out=out, packed=True)}
    # the same bits first
    ref = D.aggregate(3, recs[0], n, d, d, dense=True)
    got = D.aggregate(3, rows[0], n, d, d, packed=True)
    assert D.status() == 0 and torch.equal(got.view(torch.int32), ref.view(torch.int32))
    med, mn = timed_groups(torch, np, calls, args.warmup, args.reps, args.inner, not args.eager)
    emit(args.out, dict(kind="device", shape=name, n=n, d=d, records_bytes=rec_bytes, packed_bytes=pk_bytes,
                        copies=dict(records=len(recs), packed=len(rows)), reps=args.reps, inner=args.inner,
                        timing="eager" if args.eager else "graph replay",
                        median_us=med, min_us=mn,
                        records_tb_per_s=rec_bytes / med["records"] / 1e6,
                        packed_tb_per_s=pk_bytes / med["packed"] / 1e6,
                        packed_over_records=med["packed"] / med["records"],
                        version=lib.fltee_version().decode()))


def ecall_rows(args, torch, np, L, C):
    from fltee import ecalls as EC
    n, d = SHAPES["headline"]
    ids = np.arange(1, n + 1, dtype=np.uint32)
    values = torch.randn((n, d), device="cuda", dtype=torch.float32) * 0.01
    fl = 9900
    E = EC.Enclave(0)
    payload = {("records", "ctr"): C.produce_payloads(values, ids).cpu().numpy(),
               ("packed", "ctr"): C.produce_payloads(values, ids, packed=True).cpu().numpy(),
               ("records", "aead"): C.encrypt_parameters_auth(C.serialize_dense(values), ids, fl, 0, 3).cpu().numpy(),
               ("packed", "aead"): C.encrypt_parameters_auth(C.pack_dense(values), ids, fl, 0, 3,
                                                             packed=True).cpu().numpy()}
    del values
    torch.cuda.empty_cache()
    EC.set_upload_packed(True)
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
                    timers[key].append([float(x) * 1e3 for x in times])
    finally:
        EC.set_upload_aead(False)
        EC.set_upload_packed(False)
        E.destroy()
    ref = outs[("records", "ctr")].view(np.uint32)
    assert all(np.array_equal(o.view(np.uint32), ref) for o in outs.values())
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "packed.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from fltee import _lib as L
    from fltee import client as C
    from fltee import device as D
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for name in args.shapes.split(","):
        device_rows(args, torch, np, L, C, D, name)
        torch.cuda.empty_cache()
    if not args.no_ecall:
        ecall_rows(args, torch, np, L, C)


if __name__ == "__main__":
    main()
