"""The robust dense ECALLs on multi-GPU eids (alg 3, k = d, records uploads), host-inclusive:
the plain call and the four robust aggregates — trimmed mean by lists (t <= 64), trim by selection
(t > 64), Multi-Krum, the geometric median — CTR and GCM, on a one-GPU eid, on eids of 2, 4 and 8
virtual ranks (one device, one PCIe link: the sharded path's overhead, no speed-up expected) and,
where the box has them, on 2, 4 and 8 distinct GPUs.

    python scripts/bench_group_robust.py [--shapes 100x1000000,1000x100000] [--modes ctr,gcm]
        [--warmup 1] [--reps 3] [--sessions 3] [--baseline-lib PATH] [--out FILE]

A process holds one library, so every session is a fresh child process; with --baseline-lib (the
parent commit's build, FLTEE_LIB) the sessions alternate this build and the baseline, and the
comparison of a multi-GPU cell is this build against the BASELINE on the same eid (where the root
ran the call whole), never this build against itself.  Within a session the eids are interleaved
call by call.  Every eid's [out] must be the one-GPU eid's, bit for bit.  One JSON line per
(session, build, shape, mode, aggregate, eid): the median wall time of the ECALL and of the
enclave's timers; appended to profiles/r19/group_robust.jsonl by default.  A cell that cannot be
measured on the box (fewer GPUs than ranks) is written with "unmeasured": true.

The aggregates: trim = per mille chosen so that t = 10 (n = 100) or 50 (n = 1000), the list
kernel; select = per mille 100 with fltee_set_dense_trim_select at n >= 650 (t > 64; not
applicable below: t is capped at (n - 1) / 2); krum = (f, m) = (n / 10, n / 2); gmed = 8
iterations."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fl-tee_amd"))
sys.path.insert(0, ROOT)
ALG = 3
AGGS = ("plain", "trim", "select", "krum", "gmed")


def switch(EC, agg, n):
    """the process-wide switches of one aggregate (everything else off); False: not applicable"""
    has_select = hasattr(EC, "set_dense_trim_select")
    EC.set_dense_trim(0)
    if has_select:
        EC.set_dense_trim_select(False)
    EC.set_dense_krum(0, 0)
    EC.set_dense_gmed(0, 0.0)
    if agg == "trim":
        EC.set_dense_trim(100 if n <= 640 else 50)
    elif agg == "select":
        if n < 650 or not has_select:
            return False
        EC.set_dense_trim(100)
        EC.set_dense_trim_select(True)
    elif agg == "krum":
        EC.set_dense_krum(n // 10, n // 2)
    elif agg == "gmed":
        EC.set_dense_gmed(8, 2.0 ** -20)
    return True


def measure(args, label):
    import numpy as np
    import torch

    from fltee import _lib as L
    from fltee import client as C
    from fltee import ecalls as EC
    torch.cuda.init()
    ngpu = torch.cuda.device_count()
    eids = {"one_gpu": 0, "virtual_x2": [0] * 2, "virtual_x4": [0] * 4, "virtual_x8": [0] * 8}
    unmeasured = []
    for w in (2, 4, 8):
        if ngpu >= w:
            eids[f"gpus_x{w}"] = list(range(w))
        else:
            unmeasured.append(f"gpus_x{w}")
    fl = 9950

    def emit(line):
        print("RESULT " + json.dumps(line), flush=True)

    for shape in args.shapes.split(","):
        n, d = (int(x) for x in shape.split("x"))
        ids = np.arange(1, n + 1, dtype=np.uint32)
        val = torch.randn(n * d, device="cuda") * 0.01
        idx = torch.arange(d, device="cuda", dtype=torch.int64).repeat(n)
        rec = idx | (val.view(torch.int32).to(torch.int64) << 32)
        del val, idx
        for mode in args.modes.split(","):
            aead = mode == "gcm"
            enc = (C.encrypt_parameters_auth(rec, ids, fl, 0, ALG) if aead else C.encrypt_parameters(rec, ids)).cpu().numpy()
            torch.cuda.empty_cache()
            EC.set_upload_aead(aead)
            enclaves = {name: EC.Enclave(devs) for name, devs in eids.items()}

            def call(E):
                # the same round every time: the config re-initialised, the payload bound to round 0
                assert E.ecall_fl_init(fl, ids, d, d, 1.12, 1.0, 0.1, 1.0, ALG, 0, 0) == (0, 0)
                assert E.ecall_start_round(fl, 0, n)[:2] == (0, 0)
                t0 = time.perf_counter()
                st, rv, out, times = E.ecall_secure_aggregation(fl, 0, ids, enc, d, d, ALG)
                dt = time.perf_counter() - t0
                assert (st, rv) == (0, 0), (st, rv)
                return dt, times, out

            try:
                for agg in AGGS:
                    base = dict(build=label, n=n, d=d, mode=mode, agg=agg, payload_bytes=int(enc.nbytes), gpus=ngpu,
                                reps=args.reps, version=L.lib().fltee_version().decode())
                    if not switch(EC, agg, n):
                        emit(dict(base, eid="all", not_applicable=True))
                        continue
                    outs = {}
                    for _ in range(args.warmup):
                        for name, E in enclaves.items():
                            outs[name] = call(E)[2]
                    ref = outs["one_gpu"].view(np.uint32)
                    for name, out in outs.items():
                        assert np.array_equal(out.view(np.uint32), ref), f"{shape} {mode} {agg} {name}: not the one-GPU bits"
                    wall = {name: [] for name in enclaves}
                    timers = {name: [] for name in enclaves}
                    for _ in range(args.reps):
                        for name, E in enclaves.items():
                            dt, times, _ = call(E)
                            wall[name].append(dt * 1e3)
                            timers[name].append([float(t) * 1e3 for t in times])
                    for name in enclaves:
                        t = np.median(np.array(timers[name]), axis=0)
                        emit(dict(base, eid=name, ecall_ms=float(np.median(wall[name])),
                                          ecall_min_ms=float(np.min(wall[name])), ecall_max_ms=float(np.max(wall[name])),
                                          loading_ms=float(t[0]), decryption_ms=float(t[1]), aggregation_ms=float(t[2])))
                    for name in unmeasured:
                        emit(dict(base, eid=name, unmeasured=True))
            finally:
                switch(EC, "plain", n)
                EC.set_upload_aead(False)
                for E in enclaves.values():
                    E.destroy()
            del enc
        del rec
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100x1000000,1000x100000")
    ap.add_argument("--modes", default="ctr,gcm")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "group_robust.jsonl"))
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--label", default=None, help="(a child session: measure and print)")
    args = ap.parse_args()
    if args.label:
        measure(args, args.label)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    builds = [("this", None)] + ([("baseline", args.baseline_lib)] if args.baseline_lib else [])
    for session in range(args.sessions):
        for label, lib in builds:
            env = dict(os.environ)
            env.pop("FLTEE_LIB", None)
            if lib:
                env["FLTEE_LIB"] = os.path.abspath(lib)
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--label", label, "--shapes", args.shapes,
                                  "--modes", args.modes, "--warmup", str(args.warmup), "--reps", str(args.reps)],
                                 env=env, stdout=subprocess.PIPE, text=True)
            for text in p.stdout:  # written as they arrive: a long session still shows progress
                if not text.startswith("RESULT "):
                    continue
                line = dict(session=session, **json.loads(text[7:]))
                print(json.dumps(line), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            if p.wait() != 0:
                sys.exit(p.returncode)


if __name__ == "__main__":
    main()
