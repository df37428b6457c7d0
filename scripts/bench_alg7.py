"""aggregation_alg 7 (the stable network, k_stable.hip) against advanced, device-resident,
in ONE process.

    python scripts/bench_alg7.py [--shapes c3,c5] [--warmup 2] [--reps 5] [--out FILE]

Per shape (configs[2]: 100 x 5,089 of 50,890; configs[4]: 1000 x 100K of 10M): warm-up
calls, then `reps` interleaved event-timed calls of each alg; one JSON line with both
medians (and minima), their ratio, and the stable network's passes with the HBM bytes each
moves (the library's launch-side accounting, read from the launch trace).  Appended to
profiles/r07/alg7.jsonl by default.

    python scripts/bench_alg7.py --ranks 2,4,8 [--shapes c3,c5] [--out FILE]

The alg-7 ECALL (host ciphertext in, f32[d] out) on a one-GPU eid and on eids of W virtual
ranks (the same device W times: every range on one GPU, the exchanges device copies), the
same method: warm-up calls, then `reps` interleaved calls per eid; per shape one JSON line
with each eid's median host wall time and median "Aggregation" phase
(execution_time_results[2]), and per W the accounted bytes of one rank's passes and of the
exchanges (a rank's link volume on distinct devices).  Virtual ranks on one device show
the sharding's overhead only, not its gain.  Appended to profiles/r07/alg7_group.jsonl by
default."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fl-tee_amd"))
sys.path.insert(0, ROOT)

SHAPES = {"c3": (100, 5089, 50890), "c5": (1000, 100_000, 10_000_000)}


def network_passes(torch, lib, call):
    """[(kernel, bytes)] of the accounted streaming passes of one call (trace 'bytes' lines)"""
    lib.fltee_debug_trace.argtypes = [ctypes.c_int]
    lib.fltee_debug_trace.restype = None
    lib.fltee_debug_trace_text.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    lib.fltee_debug_trace_text.restype = ctypes.c_size_t
    torch.cuda.synchronize()
    lib.fltee_debug_trace(1)
    try:
        call()
        torch.cuda.synchronize()
    finally:
        lib.fltee_debug_trace(0)
    n = lib.fltee_debug_trace_text(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.fltee_debug_trace_text(buf, n + 1)
    passes = []
    for line in buf.value.decode().splitlines():
        f = line.split("|")
        if f[0] == "bytes":
            passes.append((f[1], int(f[2])))
    return passes


def bench_ranks(args, ranks):
    import time

    import numpy as np
    import torch

    import bench_legs
    from fltee import _lib as L
    from fltee import device as D
    from fltee.ecalls import Enclave, set_bubble_ecall
    torch.cuda.init()
    set_bubble_ecall(True)
    eids = {1: Enclave(0)}
    for w in ranks:
        eids[w] = Enclave([0] * w)
    fl = 9700
    try:
        for name in args.shapes.split(","):
            n, k, d = SHAPES[name]
            ids = np.arange(1, n + 1, dtype=np.uint32)
            rec = bench_legs.make_records(torch, n, d, k, 11, "cuda")
            cipher = torch.empty_like(rec)
            D.decrypt(ids, rec, k * 8, cipher)  # CTR: encryption == decryption
            host = cipher.cpu().numpy().view(np.uint8)
            del rec, cipher
            fls = {}
            for w, E in eids.items():
                fl += 1
                fls[w] = fl
                assert E.ecall_fl_init(fl, ids, d, k, 1.12, 1.0, 0.1, 1.0, L.ALG_BUBBLE, 0, 0) == (0, 0)
            walls, aggs, rounds = {w: [] for w in eids}, {w: [] for w in eids}, {w: 0 for w in eids}
            outs = {}

            def call(w):
                E, r = eids[w], rounds[w]
                assert E.ecall_start_round(fls[w], r, n)[:2] == (0, 0)
                t0 = time.perf_counter()
                st, rv, out, tt = E.ecall_secure_aggregation(fls[w], r, ids, host, d, k, L.ALG_BUBBLE)
                wall = time.perf_counter() - t0
                assert (st, rv) == (0, 0), (w, st, rv)
                rounds[w] = r + 1
                return wall, float(tt[2]), out

            for _ in range(args.warmup):
                for w in eids:
                    call(w)
            for _ in range(args.reps):
                for w in eids:
                    wall, agg, outs[w] = call(w)
                    walls[w].append(wall * 1e3)
                    aggs[w].append(agg * 1e3)
            for w in ranks:  # the same bits as one GPU
                assert np.array_equal(outs[w].view(np.uint32), outs[1].view(np.uint32)), w
            M = 1 << (n * k + d - 1).bit_length()
            acct = {}
            for w in eids:
                every = network_passes(torch, L.lib(), lambda: call(w))
                net = [(kname, b) for kname, b in every if kname.startswith("stable_")]
                ex = [b for kname, b in net if kname == "stable_exchange"]
                acct[w] = dict(network_launches=len(net), network_bytes=sum(b for _, b in net),
                               per_rank_pass_bytes=(sum(b for _, b in net) - sum(ex)) // w,
                               exchange_launches=len(ex),
                               exchange_steps_per_rank=len(ex) // w,
                               exchange_link_bytes_per_rank=sum(ex) // 3 // w,
                               bytes_per_launch_max=max(b for _, b in net))
            line = dict(mode="ecall_virtual_ranks", shape=name, n=n, k=k, d=d, M=M, reps=args.reps,
                        payload_bytes=n * k * 8,
                        wall_ms={str(w): float(np.median(walls[w])) for w in eids},
                        aggregation_ms={str(w): float(np.median(aggs[w])) for w in eids},
                        aggregation_min_ms={str(w): float(np.min(aggs[w])) for w in eids},
                        accounted={str(w): acct[w] for w in eids},
                        version=L.lib().fltee_version().decode())
            text = json.dumps(line)
            print(text, flush=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
            del host
    finally:
        set_bubble_ecall(False)
        for E in eids.values():
            E.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c3,c5")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranks", default="", help="e.g. 2,4,8: time the alg-7 ECALL on virtual-rank eids")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r07", "alg7_group.jsonl" if args.ranks else "alg7.jsonl")
    if args.ranks:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        return bench_ranks(args, [int(w) for w in args.ranks.split(",")])
    import numpy as np
    import torch

    import bench_legs
    from fltee import _lib as L
    from fltee import device as D
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for name in args.shapes.split(","):
        n, k, d = SHAPES[name]
        rec = bench_legs.make_records(torch, n, d, k, 11, "cuda")
        out = torch.empty(d, dtype=torch.float32, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        algs = {"alg7": L.ALG_BUBBLE, "advanced": L.ALG_ADVANCED}
        for alg in algs.values():
            D.reserve(alg, n, k, d)
            for _ in range(args.warmup):
                D.aggregate(alg, rec, n, k, d, out=out, status=st)
        torch.cuda.synchronize()
        times = {a: [] for a in algs}
        for _ in range(args.reps):
            for a, alg in algs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                D.aggregate(alg, rec, n, k, d, out=out, status=st)
                e1.record()
                torch.cuda.synchronize()
                times[a].append(e0.elapsed_time(e1))
        assert int(st.item()) == 0
        every = network_passes(torch, L.lib(),
                               lambda: D.aggregate(L.ALG_BUBBLE, rec, n, k, d, out=out, status=st))
        passes = [p for p in every if p[0].startswith("stable_")]
        tail = [p for p in every if not p[0].startswith("stable_")]  # fold, compaction: shared
        adv = network_passes(torch, L.lib(),
                             lambda: D.aggregate(L.ALG_ADVANCED, rec, n, k, d, out=out, status=st))
        med = {a: float(np.median(t)) for a, t in times.items()}
        M = 1 << (n * k + d - 1).bit_length()
        line = dict(shape=name, n=n, k=k, d=d, M=M, reps=args.reps,
                    alg7_ms=med["alg7"], advanced_ms=med["advanced"],
                    alg7_min_ms=float(np.min(times["alg7"])),
                    advanced_min_ms=float(np.min(times["advanced"])),
                    ratio=med["alg7"] / med["advanced"],
                    network_passes=len(passes),
                    network_bytes=sum(b for _, b in passes),
                    bytes_per_pass_max=max(b for _, b in passes),
                    tail_passes=len(tail), tail_bytes=sum(b for _, b in tail),
                    advanced_passes=len(adv), advanced_bytes=sum(b for _, b in adv),
                    passes=[[kname, b] for kname, b in passes],
                    version=L.lib().fltee_version().decode())
        text = json.dumps(line)
        print(text, flush=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
        del rec, out


if __name__ == "__main__":
    main()
