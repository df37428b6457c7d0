"""The trimmed mean (FLTEE_OPT_TRIM, k_trim.hip) against the untrimmed dense / packed
accumulate, device-resident, and the flag-off path of this build against another build of the
library (the parent commit's), alternating in one session.

    python scripts/bench_trim.py [--parent-lib PATH] [--sessions 3] [--shapes headline,c3]
                                 [--warmup 2] [--reps 5] [--out FILE]

Every session is a fresh process bound to one library (FLTEE_LIB): this build times, per shape
(headline: 100 x 1M; c3: 100 x 50,890) and layout (records, packed), alg 3 untrimmed (t = 0,
flag off) alone in one session and, in another, next to t in {1, 10, 49}; the parent build
times the untrimmed calls alone.  2
warm-ups, then the median of 5 interleaved event-timed calls; every call reads a copy of its
input that the calls before it have pushed out of the 256 MB Infinity Cache.  With
--parent-lib the sessions alternate parent, this, this with the trimmed calls, parent, ... and
the last lines state
the flag-off ratio next to the parent's own session-to-session spread.  A trimmed call reads
its input twice: read_tb_per_s counts 2 * n * d * (8 or 4) + d * 4 bytes.  One JSON line per
measurement, appended to profiles/r12/trim.jsonl by default."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fl-tee_amd"))

SHAPES = {"headline": (100, 1_000_000), "c3": (100, 50890)}
TRIMS = (1, 10, 49)
CACHE_BYTES = 512 << 20  # twice the Infinity Cache: the copies a call rotates through


def worker(args):
    import numpy as np
    import torch

    from fltee import _lib as L
    from fltee import client as C
    from fltee import device as D
    lib = L.lib()
    trims = TRIMS if args.trimmed and hasattr(lib, "fltee_trim_count") else ()
    for name in args.shapes:
        n, d = SHAPES[name]
        values = torch.randn((n, d), device="cuda", dtype=torch.float32)
        out = torch.empty(d, dtype=torch.float32, device="cuda")
        for layout, make, per in (("records", C.serialize_dense, 8), ("packed", C.pack_dense, 4)):
            nbytes = n * (d if layout == "records" else D.packed_row(d)) * per
            bufs = [make(values) for _ in range(max(2, -(-CACHE_BYTES // nbytes)))]
            turn = [0]
            kw = dict(packed=True) if layout == "packed" else dict(dense=True)

            def call(t):
                turn[0] = (turn[0] + 1) % len(bufs)
                D.aggregate(3, bufs[turn[0]], n, d, d, out=out, **kw, **(dict(trim=t) if t else {}))

            cases = (0,) + tuple(trims)
            for _ in range(args.warmup):
                for t in cases:
                    call(t)
            torch.cuda.synchronize()
            times = {t: [] for t in cases}
            for _ in range(args.reps):
                for t in cases:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(t)
                    e1.record()
                    torch.cuda.synchronize()
                    times[t].append(e0.elapsed_time(e1) * 1e3)
            assert D.status() == 0
            for t in cases:
                us = float(np.median(times[t]))
                reads = (2 if t else 1) * nbytes + d * 4
                print(json.dumps(dict(kind="device", build=args.build, shape=name, n=n, d=d, layout=layout, t=t,
                                      flag=bool(t), median_us=us, min_us=float(np.min(times[t])),
                                      read_bytes=reads, read_tb_per_s=reads / us / 1e6, reps=args.reps,
                                      version=lib.fltee_version().decode())), flush=True)
            del bufs


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent-lib", default=None, help="libfltee_agg.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--shapes", default="headline,c3")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "trim.jsonl"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--build", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--trimmed", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.shapes = args.shapes.split(",")
    if args.worker:
        return worker(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = []
    for s in range(args.sessions):
        # like for like: a parity session of either build times the untrimmed calls alone (after
        # a long trimmed kernel an untrimmed call of ~20 us is timed at other clocks)
        for build, libpath, trimmed in (("parent", args.parent_lib, False), ("this", None, False),
                                        ("this", None, True)):
            if build == "parent" and not libpath:
                continue
            env = dict(os.environ)
            env.pop("FLTEE_LIB", None)
            if libpath:
                env["FLTEE_LIB"] = os.path.abspath(libpath)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--build", build, "--shapes",
                   ",".join(args.shapes), "--warmup", str(args.warmup), "--reps", str(args.reps)]
            cmd += ["--trimmed"] if trimmed else []
            res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=600, check=True)
            for text in res.stdout.splitlines():
                if text.startswith("{"):
                    line = dict(json.loads(text), session=s, with_trimmed=trimmed)
                    lines.append(line)
                    print(json.dumps(line), flush=True)
                    with open(args.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
    if args.parent_lib:  # the flag-off path against the parent's own spread
        for name in args.shapes:
            for layout in ("records", "packed"):
                pick = lambda b: [x["median_us"] for x in lines if (x["build"], x["shape"], x["layout"], x["t"],
                                                                    x["with_trimmed"]) == (b, name, layout, 0, False)]
                par, this = pick("parent"), pick("this")
                line = dict(kind="flag_off_parity", shape=name, layout=layout, parent_us=par, this_us=this,
                            parent_spread=max(par) / min(par) - 1,
                            this_median_us=sorted(this)[len(this) // 2],
                            inside=sorted(this)[len(this) // 2] <= max(par))  # no slower than the parent's slowest
                print(json.dumps(line), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
