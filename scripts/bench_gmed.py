"""The geometric median (FLTEE_OPT_GMED, k_gmed.hip) against the plain dense / packed accumulate
and the Multi-Krum call of the same shape, device-resident; and the flag-off calls of this build
against another build of the library (the parent commit's), alternating in one run.

    python scripts/bench_gmed.py [--parent-lib PATH] [--sessions 3] [--rows all]
                                 [--warmup 2] [--reps 5] [--out FILE]

Every session is a fresh process bound to one library (FLTEE_LIB).  A row is a shape, and per
layout a set of alg-3 calls timed interleaved: 2 warm-ups, then the median of 5 event-timed calls
each; every call reads a copy of its input that the calls before it have pushed out of the 256 MB
Infinity Cache.
  headline  100 x 1M      records and packed
  c3        300 x 50,890  packed
  c4       1000 x 100K    packed
Per row and layout, in one session: the plain call; the Multi-Krum call (f = n / 10, m = n - 2 f);
and for R in {1, 8} the geometric-median call and its weights alone (fltee_gmed_weights_device:
the Gram pass, the reduce, the init and R x (matvec, update); the difference to the whole call is
the weighted accumulate).  Each line carries its ratio to the plain call and to the Krum call of
the same session.  With --parent-lib the sessions alternate parent, this (flag-off calls alone),
this with every call, parent, ...; the last lines state this build's flag-off median next to the
parent's own session range.  One JSON line per measurement, appended to profiles/r18/gmed.jsonl by
default."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fl-tee_amd"))

# row -> (n, d, layouts)
ROWS = {
    "headline": (100, 1_000_000, ("records", "packed")),
    "c3": (300, 50890, ("packed",)),
    "c4": (1000, 100_000, ("packed",)),
}
ITERS = (1, 8)
NU = 2.0 ** -20
CACHE_BYTES = 512 << 20  # twice the Infinity Cache: the copies a call rotates through


def worker(args):
    import numpy as np
    import torch

    from fltee import _lib as L
    from fltee import client as C
    from fltee import device as D
    lib = L.lib()
    for name in args.rows:
        if name not in ROWS:
            continue
        n, d, layouts = ROWS[name]
        krum = (n // 10, n - 2 * (n // 10))
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
                what, arg = case
                turn[0] = (turn[0] + 1) % len(bufs)
                buf = bufs[turn[0]]
                if what == "plain":
                    D.aggregate(3, buf, n, d, d, out=out, **kw)
                elif what == "krum":
                    D.aggregate(3, buf, n, d, d, out=out, krum=arg, **kw)
                elif what == "gmed":
                    D.aggregate(3, buf, n, d, d, out=out, gmed=(arg, NU), **kw)
                else:
                    D.gmed_weights(buf, n, d, arg, NU, **sel_kw)

            cases = [("plain", None)]
            if not args.parity:  # (what the parent build answers too: the plain call alone)
                cases += [("krum", krum)] + [(w, r) for r in ITERS for w in ("gmed", "gmed_weights")]
                D.reserve(3, n, d, d, krum=krum, **kw)
                D.reserve(3, n, d, d, gmed=(1, NU), **kw)
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
            base = float(np.median(times[("plain", None)]))
            kbase = float(np.median(times[("krum", krum)])) if not args.parity else None
            for case in cases:
                what, arg = case
                us = float(np.median(times[case]))
                line = dict(kind="device", build=args.build, row=name, n=n, d=d, layout=layout, route=what,
                            iters=arg if what.startswith("gmed") else 0, median_us=us,
                            min_us=float(np.min(times[case])), max_us=float(np.max(times[case])),
                            ratio_to_plain=us / base, ratio_to_krum=us / kbase if kbase else None,
                            reps=args.reps, version=lib.fltee_version().decode())
                print(json.dumps(line), flush=True)
            del bufs


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent-lib", default=None, help="libfltee_agg.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--rows", default="all")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "gmed.jsonl"))
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
            res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=600, check=True)
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
