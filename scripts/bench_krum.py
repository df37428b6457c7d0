"""Multi-Krum (FLTEE_OPT_KRUM, k_krum.hip) against the untrimmed dense / packed accumulate,
device-resident; and the flag-off calls of this build against another build of the library (the
parent commit's), alternating in one run.

    python scripts/bench_krum.py [--parent-lib PATH] [--sessions 3] [--rows all]
                                 [--warmup 2] [--reps 5] [--out FILE]

Every session is a fresh process bound to one library (FLTEE_LIB).  A row is a shape, and per
layout a set of alg-3 calls timed interleaved: 2 warm-ups, then the median of 5 event-timed calls
each; every call reads a copy of its input that the calls before it have pushed out of the 256 MB
Infinity Cache.
  headline  100 x 1M      records and packed: untrimmed; f = 10, m = 1 and m = 90
  c3        300 x 50,890  packed: untrimmed; f = 30, m = 240
  c4       1000 x 100K    packed: untrimmed; f = 100, m = 800
Per Krum case two lines: the whole call, and its selection alone (fltee_krum_select_device: the
Gram pass, the reduce, the scores and the ranking — the Gram kernel dominates it; the difference
to the whole call is the accumulate).  Each carries its ratio to the untrimmed call of the same
session, the two-read floor's bytes 2 n d (8 | 4) + d 4 with the rate they imply, the MFMA count
ceil(n/16) (ceil(n/16) + 1) / 2 * ceil(d/4) and, for the selection, the cycles per MFMA and SIMD
that count implies at --mhz (2400) on 1024 SIMDs: an upper bound on the instruction's issue
interval, since it charges the staging, the reduce and the sort to it.  With --parent-lib the
sessions alternate parent, this (flag-off calls alone), this with the Krum calls, parent, ...;
the last lines state this build's flag-off median next to the parent's own session range.  One
JSON line per measurement, appended to profiles/r17/krum.jsonl by default."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fl-tee_amd"))

# row -> (n, d, layouts, [(f, m)] timed next to the untrimmed call)
ROWS = {
    "headline": (100, 1_000_000, ("records", "packed"), [(10, 1), (10, 90)]),
    "c3": (300, 50890, ("packed",), [(30, 240)]),
    "c4": (1000, 100_000, ("packed",), [(100, 800)]),
}
PARITY = {name: (n, d, lay, []) for name, (n, d, lay, _) in ROWS.items()}  # what the parent build answers too
CACHE_BYTES = 512 << 20  # twice the Infinity Cache: the copies a call rotates through
SIMDS = 256 * 4


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
        n, d, layouts, krums = table[name]
        values = torch.randn((n, d), device="cuda", dtype=torch.float32)
        out = torch.empty(d, dtype=torch.float32, device="cuda")
        for layout in layouts:
            make, per = (C.serialize_dense, 8) if layout == "records" else (C.pack_dense, 4)
            nbytes = n * (d if layout == "records" else D.packed_row(d)) * per
            bufs = [make(values) for _ in range(max(2, -(-CACHE_BYTES // nbytes)))]
            turn = [0]
            kw = dict(packed=True) if layout == "packed" else dict(dense=True)
            sel_kw = dict(packed=True) if layout == "packed" else {}

            def call(case):
                what, fm = case
                turn[0] = (turn[0] + 1) % len(bufs)
                if what == "select":
                    D.krum_select(bufs[turn[0]], n, d, *fm, **sel_kw)
                else:
                    D.aggregate(3, bufs[turn[0]], n, d, d, out=out, **kw, **(dict(krum=fm) if fm else {}))

            cases = [("call", None)] + [(w, fm) for fm in krums for w in ("call", "select")]
            for fm in krums:
                D.reserve(3, n, d, d, krum=fm, **kw)
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
            base = float(np.median(times[("call", None)]))
            tiles = -(-n // 16)
            mfma = tiles * (tiles + 1) // 2 * -(-d // 4)
            for case in cases:
                what, fm = case
                us = float(np.median(times[case]))
                reads = (2 if fm else 1) * nbytes + d * 4
                line = dict(kind="device", build=args.build, row=name, n=n, d=d, layout=layout,
                            route="untrimmed" if not fm else "krum" if what == "call" else "krum_select",
                            f=fm[0] if fm else 0, m=fm[1] if fm else 0, median_us=us,
                            min_us=float(np.min(times[case])), ratio_to_untrimmed=us / base, floor_bytes=reads,
                            floor_tb_per_s=reads / us / 1e6, reps=args.reps, version=lib.fltee_version().decode())
                if fm:
                    line.update(mfma=mfma)
                if what == "select":
                    line.update(cycles_per_mfma_per_simd=us * args.mhz * SIMDS / mfma)
                print(json.dumps(line), flush=True)
            del bufs


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent-lib", default=None, help="libfltee_agg.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--rows", default="all")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mhz", type=float, default=2400.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "krum.jsonl"))
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
                   ",".join(args.rows), "--warmup", str(args.warmup), "--reps", str(args.reps), "--mhz", str(args.mhz)]
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
        keys = sorted({(x["row"], x["layout"]) for x in lines if x["parity"]})
        for row, layout in keys:
            pick = lambda b: [x["median_us"] for x in lines
                              if x["parity"] and (x["build"], x["row"], x["layout"]) == (b, row, layout)]
            par, this = pick("parent"), pick("this")
            med = sorted(this)[len(this) // 2]
            line = dict(kind="flag_off_parity", row=row, layout=layout, parent_us=par, this_us=this,
                        parent_spread=max(par) / min(par) - 1, this_median_us=med,
                        inside=min(par) <= med <= max(par), no_slower=med <= max(par))
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
