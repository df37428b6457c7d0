"""Trim by selection (FLTEE_OPT_TRIM_SELECT, k_trim_select.hip) against the list route
(k_trim.hip) and the untrimmed dense / packed accumulate, device-resident; and the flag-off
calls of this build against another build of the library (the parent commit's), alternating in
one run.

    python scripts/bench_trim_select.py [--parent-lib PATH] [--sessions 3] [--rows all]
                                        [--warmup 2] [--reps 5] [--out FILE]

Every session is a fresh process bound to one library (FLTEE_LIB).  A row is a shape, and per
layout (records, packed) a set of alg-3 calls timed interleaved: 2 warm-ups, then the median of
5 event-timed calls each; every call reads a copy of its input that the calls before it have
pushed out of the 256 MB Infinity Cache.
  headline  100 x 1M      untrimmed; t = 10 and 49 on the list route and by selection
  c4       1000 x 100K    untrimmed; t = 100 and 499 by selection (the list route refuses them)
  cap129    129 x 50,890  untrimmed; the median (t = 64) on the list route and by selection
  cap131    131 x 50,890  untrimmed; the median (t = 65) by selection (past the list's cap)
read_tb_per_s counts ONE read of the input, n * d * (8 or 4) + d * 4 bytes, for every call (the
list route reads it twice).  With --parent-lib the sessions alternate parent, this (flag-off
calls alone: untrimmed, and the list route at t = 1 and 49 on 100 x 1M), this with the
selection calls, parent, ...; the last lines state this build's flag-off median next to the
parent's own session range.  One JSON line per measurement, appended to
profiles/r15/trim_select.jsonl by default."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fl-tee_amd"))

# row -> (n, d, [(t, select)] timed next to the untrimmed call)
ROWS = {
    "headline": (100, 1_000_000, [(10, False), (10, True), (49, False), (49, True)]),
    "c4": (1000, 100_000, [(100, True), (499, True)]),
    "cap129": (129, 50890, [(64, False), (64, True)]),
    "cap131": (131, 50890, [(65, True)]),
}
PARITY = {"headline": (100, 1_000_000, [(1, False), (49, False)])}  # what the parent build answers too
CACHE_BYTES = 512 << 20  # twice the Infinity Cache: the copies a call rotates through


def worker(args):
    import numpy as np
    import torch

    from fltee import _lib as L
    from fltee import client as C
    from fltee import device as D
    lib = L.lib()
    table = PARITY if args.parity else ROWS
    for name in args.rows:
        if name not in table:
            continue
        n, d, trimmed = table[name]
        values = torch.randn((n, d), device="cuda", dtype=torch.float32)
        out = torch.empty(d, dtype=torch.float32, device="cuda")
        for layout, make, per in (("records", C.serialize_dense, 8), ("packed", C.pack_dense, 4)):
            nbytes = n * (d if layout == "records" else D.packed_row(d)) * per
            bufs = [make(values) for _ in range(max(2, -(-CACHE_BYTES // nbytes)))]
            turn = [0]
            kw = dict(packed=True) if layout == "packed" else dict(dense=True)

            def call(case):
                t, select = case
                turn[0] = (turn[0] + 1) % len(bufs)
                more = dict(trim=t) if t else {}
                if select:
                    more["trim_select"] = True
                D.aggregate(3, bufs[turn[0]], n, d, d, out=out, **kw, **more)

            cases = [(0, False)] + list(trimmed)
            for _ in range(args.warmup):
                for case in cases:
                    call(case)
            torch.cuda.synchronize()
            times = {case: [] for case in cases}
            for _ in range(args.reps):
                for case in cases:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(case)
                    e1.record()
                    torch.cuda.synchronize()
                    times[case].append(e0.elapsed_time(e1) * 1e3)
            assert D.status() == 0
            base = float(np.median(times[(0, False)]))
            for case in cases:
                us = float(np.median(times[case]))
                reads = nbytes + d * 4
                print(json.dumps(dict(kind="device", build=args.build, row=name, n=n, d=d, layout=layout, t=case[0],
                                      route="untrimmed" if not case[0] else "select" if case[1] else "list",
                                      median_us=us, min_us=float(np.min(times[case])), ratio_to_untrimmed=us / base,
                                      single_read_bytes=reads, read_tb_per_s=reads / us / 1e6, reps=args.reps,
                                      version=lib.fltee_version().decode())), flush=True)
            del bufs


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent-lib", default=None, help="libfltee_agg.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--rows", default="all")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "trim_select.jsonl"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--build", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--parity", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.rows = list(ROWS) if args.rows == "all" else args.rows.split(",")
    if args.worker:
        return worker(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = []
    for s in range(args.sessions):
        # like for like: a parity session of either build times the flag-off calls alone
        for build, libpath, parity in (("parent", args.parent_lib, True), ("this", None, True), ("this", None, False)):
            if parity and not args.parent_lib:
                continue
            env = dict(os.environ)
            env.pop("FLTEE_LIB", None)
            if libpath:
                env["FLTEE_LIB"] = os.path.abspath(libpath)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--build", build, "--rows",
                   ",".join(args.rows), "--warmup", str(args.warmup), "--reps", str(args.reps)]
            cmd += ["--parity"] if parity else []
            res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=900, check=True)
            for text in res.stdout.splitlines():
                if text.startswith("{"):
                    line = dict(json.loads(text), session=s, parity=parity)
                    lines.append(line)
                    print(json.dumps(line), flush=True)
                    with open(args.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
    if args.parent_lib:  # the flag-off calls against the parent's own session range
        keys = sorted({(x["row"], x["layout"], x["t"]) for x in lines if x["parity"]})
        for row, layout, t in keys:
            pick = lambda b: [x["median_us"] for x in lines
                              if x["parity"] and (x["build"], x["row"], x["layout"], x["t"]) == (b, row, layout, t)]
            par, this = pick("parent"), pick("this")
            med = sorted(this)[len(this) // 2]
            line = dict(kind="flag_off_parity", row=row, layout=layout, t=t, parent_us=par, this_us=this,
                        parent_spread=max(par) / min(par) - 1, this_median_us=med,
                        inside=min(par) <= med <= max(par), no_slower=med <= max(par))
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
