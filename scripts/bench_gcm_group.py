"""The authenticated dense ECALL (fltee_set_upload_aead(1), alg 3, k = d) at the headline shape
on one GPU and on multi-GPU eids, host-inclusive, by scripts/bench_gcm.py's method: warm-up
calls, then `reps` interleaved calls of every eid, the median of each.

    python scripts/bench_gcm_group.py [--n 100] [--d 1000000] [--warmup 2] [--reps 5] [--out FILE]
        [--baseline-lib PATH [--sessions 2]]

Eids: Enclave(0); four virtual ranks [0, 0, 0, 0] (one device, one PCIe link: the sharded
path's cost, no speed-up expected); and, on a box with more than one GPU, its distinct devices
(a power of two of them).  One JSON line per eid: the wall time of the ECALL and the enclave's
own timers (Loading / Decryption / Aggregation).  The output bits of every eid must agree.

--baseline-lib: another build of the library (the parent commit's, FLTEE_LIB) measured by the
same calls.  A process holds one library, so every measurement is a fresh child process, and
the sessions alternate this build and the baseline: the baseline's session-to-session spread
is the yardstick for "parity".  Appended to profiles/r09/gcm_group.jsonl by default."""
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


def measure(args, label):
    import numpy as np
    import torch

    from fltee import _lib as L
    from fltee import client as C
    from fltee.ecalls import Enclave, set_upload_aead
    torch.cuda.init()
    n, d = args.n, args.d
    ids = np.arange(1, n + 1, dtype=np.uint32)
    fl = 9900
    val = torch.randn(n * d, device="cuda") * 0.01
    idx = torch.arange(d, device="cuda", dtype=torch.int64).repeat(n)
    rec = idx | (val.view(torch.int32).to(torch.int64) << 32)
    enc = C.encrypt_parameters_auth(rec, ids, fl, 0, ALG).cpu().numpy()
    del val, idx, rec
    torch.cuda.empty_cache()
    eids = {"one_gpu": 0, "virtual_x4": [0, 0, 0, 0]}
    ngpu = torch.cuda.device_count()
    if ngpu > 1:
        w = 1 << (ngpu.bit_length() - 1)
        eids[f"gpus_x{w}"] = list(range(w))
    set_upload_aead(True)
    enclaves = {name: Enclave(devs) for name, devs in eids.items()}

    def call(E):
        # the same round every time: the config re-initialised, the payload bound to round 0
        assert E.ecall_fl_init(fl, ids, d, d, 1.12, 1.0, 0.1, 1.0, ALG, 0, 0) == (0, 0)
        assert E.ecall_start_round(fl, 0, n)[:2] == (0, 0)
        t0 = time.perf_counter()
        st, rv, out, times = E.ecall_secure_aggregation(fl, 0, ids, enc, d, d, ALG)
        dt = time.perf_counter() - t0
        assert (st, rv) == (0, 0)
        return dt, times, out

    try:
        outs = {}
        for _ in range(args.warmup):
            for name, E in enclaves.items():
                outs[name] = call(E)[2]
        ref = outs["one_gpu"].view(np.uint32)
        for name, out in outs.items():
            assert np.array_equal(out.view(np.uint32), ref), f"{name}: not the one-GPU bits"
        wall = {name: [] for name in enclaves}
        timers = {name: [] for name in enclaves}
        for _ in range(args.reps):
            for name, E in enclaves.items():
                dt, times, _ = call(E)
                wall[name].append(dt * 1e3)
                timers[name].append([float(t) * 1e3 for t in times])
    finally:
        set_upload_aead(False)
        for E in enclaves.values():
            E.destroy()
    lines = []
    for name in enclaves:
        t = np.median(np.array(timers[name]), axis=0)
        lines.append(dict(build=label, eid=name, devices=eids[name], n=n, d=d,
                          payload_bytes=int(enc.nbytes), reps=args.reps,
                          ecall_ms=float(np.median(wall[name])), ecall_min_ms=float(np.min(wall[name])),
                          ecall_max_ms=float(np.max(wall[name])), loading_ms=float(t[0]),
                          decryption_ms=float(t[1]), aggregation_ms=float(t[2]), gpus=ngpu,
                          version=L.lib().fltee_version().decode()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--d", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "gcm_group.jsonl"))
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--sessions", type=int, default=2)
    ap.add_argument("--label", default=None, help="(a child session: measure and print)")
    args = ap.parse_args()
    if args.label:
        for line in measure(args, args.label):
            print("RESULT " + json.dumps(line), flush=True)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    builds = [("this", None)] + ([("baseline", args.baseline_lib)] if args.baseline_lib else [])
    for session in range(args.sessions if args.baseline_lib else 1):
        for label, lib in builds:
            env = dict(os.environ)
            env.pop("FLTEE_LIB", None)
            if lib:
                env["FLTEE_LIB"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--label", label, "--n", str(args.n),
                                "--d", str(args.d), "--warmup", str(args.warmup), "--reps", str(args.reps)],
                               env=env, capture_output=True, text=True, timeout=400)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-2000:])
                sys.exit(p.returncode)
            for text in p.stdout.splitlines():
                if not text.startswith("RESULT "):
                    continue
                line = dict(session=session, **json.loads(text[7:]))
                print(json.dumps(line), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
