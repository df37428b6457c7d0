"""The authenticated ECALL under the failure policies (fltee_set_upload_aead_policy), host-inclusive,
by scripts/bench_gcm_group.py's method: warm-up calls, then `reps` interleaved calls of every
mode, the median of each.

    python scripts/bench_gcm_policy.py [--warmup 2] [--reps 5] [--out FILE]
        [--baseline-lib PATH [--sessions 2]]

Shapes: alg 3 dense at 100 x 1M (800 MB) and alg 1 at configs[2] (100 x 5089 of 50890).  Modes,
one JSON line each: abort_clean (the default policy), drop_clean (DROP, no failure: the wider
verdict readback is the only difference), drop_one_failed (client 0's tag flipped: every other
slice moves), and drop_one_failed on four virtual ranks (the group stops at its verdict and
the root loads again: overhead only, one device).  Beside them the gather kernel alone
(device-resident, hipEvents, client 0 dropped) with its bytes moved per second, and the
same-run streaming-read floor of bench_legs.read_floor over the same number of bytes.

--baseline-lib: another build of the library (the parent commit's, FLTEE_LIB), which knows
abort_clean only, measured by the same calls.  A process holds one library, so every
measurement is a fresh child process, and the sessions alternate this build and the baseline:
the baseline's session-to-session spread is the yardstick for "parity".  Appended to
profiles/r10/gcm_policy.jsonl by default."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fl-tee_amd"))
sys.path.insert(0, ROOT)

SHAPES = {"ns": dict(alg=3, n=100, d=1_000_000, k=1_000_000),
          "c3": dict(alg=1, n=100, d=50890, k=5089)}


def payload(torch, C, np, shape, ids, fl):
    alg, n, d, k = shape["alg"], shape["n"], shape["d"], shape["k"]
    val = torch.randn(n * k, device="cuda") * 0.01
    if k == d:
        idx = torch.arange(d, device="cuda", dtype=torch.int64).repeat(n)
    else:  # k distinct indices per client: a run from a random offset, mod d
        off = torch.randint(0, d, (n, 1), device="cuda")
        idx = ((torch.arange(k, device="cuda").unsqueeze(0) + off) % d).reshape(-1).to(torch.int64)
    rec = idx | (val.view(torch.int32).to(torch.int64) << 32)
    return C.encrypt_parameters_auth(rec, ids, fl, 0, alg).cpu().numpy()


def gather_alone(torch, np, n, k, reps):
    """the kernel by itself: client 0 dropped, median of `reps` event-timed launches"""
    from fltee import device as D
    rec = torch.randint(-2 ** 62, 2 ** 62, (n, k), dtype=torch.int64, device="cuda")
    keep = torch.arange(1, n, dtype=torch.int32, device="cuda")
    out = torch.empty((n - 1, k), dtype=torch.int64, device="cuda")
    ms = []
    for i in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        D.gather_clients(rec, keep, out=out)
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(a.elapsed_time(b))
    assert D.status() == 0 and torch.equal(out, rec[1:])
    moved = 2 * (n - 1) * k * 8
    t = float(np.median(ms))
    return dict(gather_ms=t, gather_bytes_moved=moved, gather_tbs=moved / (t * 1e-3) / 1e12)


def measure(args, label):
    import numpy as np
    import torch

    from fltee import _lib as L
    from fltee import client as C
    from fltee.ecalls import Enclave, set_upload_aead
    torch.cuda.init()
    lib = L.lib()
    has_policy = hasattr(lib, "fltee_set_upload_aead_policy")
    lines = []
    set_upload_aead(True)
    E1, E4 = Enclave(0), (Enclave([0, 0, 0, 0]) if has_policy else None)
    try:
        for sname, shape in SHAPES.items():
            alg, n, d, k = shape["alg"], shape["n"], shape["d"], shape["k"]
            ids = np.arange(1, n + 1, dtype=np.uint32)
            fl = 9910
            enc = payload(torch, C, np, shape, ids, fl)
            bad = enc.copy()
            bad[k * 8 + 3] ^= 0x20  # client 0's tag
            torch.cuda.empty_cache()
            modes = [("abort_clean", E1, 0, enc)]
            if has_policy:
                modes += [("drop_clean", E1, 2, enc), ("drop_one_failed", E1, 2, bad),
                          ("drop_one_failed_virtual_x4", E4, 2, bad)]

            def call(E, policy, e):
                if has_policy:
                    lib.fltee_set_upload_aead_policy(policy, 1)
                # the same round every time: the config re-initialised, the payload bound to round 0
                assert E.ecall_fl_init(fl, ids, d, k, 1.12, 1.0, 0.1, 1.0, alg, 0, 0) == (0, 0)
                assert E.ecall_start_round(fl, 0, n)[:2] == (0, 0)
                t0 = time.perf_counter()
                st, rv, out, times = E.ecall_secure_aggregation(fl, 0, ids, e, d, k, alg)
                dt = time.perf_counter() - t0
                assert (st, rv) == (0, 0)
                return dt, times, out

            outs = {}
            for _ in range(args.warmup):
                for name, E, policy, e in modes:
                    outs[name] = call(E, policy, e)[2]
            if has_policy:
                assert np.array_equal(outs["abort_clean"].view(np.uint32), outs["drop_clean"].view(np.uint32))
                assert np.array_equal(outs["drop_one_failed"].view(np.uint32),
                                      outs["drop_one_failed_virtual_x4"].view(np.uint32))
                assert E1.auth_report(fl)[1] in ([], [1])
            wall = {m[0]: [] for m in modes}
            timers = {m[0]: [] for m in modes}
            for _ in range(args.reps):
                for name, E, policy, e in modes:
                    dt, times, _ = call(E, policy, e)
                    wall[name].append(dt * 1e3)
                    timers[name].append([float(t) * 1e3 for t in times])
            extra = {}
            if has_policy:
                import bench_legs
                extra = gather_alone(torch, np, n, k, args.reps)
                floor = bench_legs.read_floor(torch, extra["gather_bytes_moved"] // 2, torch.device("cuda"),
                                              reps=2, steps=10)
                extra.update(read_floor_gbs=floor["gbs"], read_floor_us=floor["us"])
            for name, E, policy, e in modes:
                t = np.median(np.array(timers[name]), axis=0)
                lines.append(dict(build=label, shape=sname, mode=name, alg=alg, n=n, d=d, k=k,
                                  payload_bytes=int(enc.nbytes), reps=args.reps,
                                  ecall_ms=float(np.median(wall[name])), ecall_min_ms=float(np.min(wall[name])),
                                  ecall_max_ms=float(np.max(wall[name])), loading_ms=float(t[0]),
                                  decryption_ms=float(t[1]), aggregation_ms=float(t[2]),
                                  version=lib.fltee_version().decode(),
                                  **(extra if name == "drop_one_failed" else {})))
            del enc, bad
    finally:
        if has_policy:
            lib.fltee_set_upload_aead_policy(0, 0)
        set_upload_aead(False)
        E1.destroy()
        if E4:
            E4.destroy()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "gcm_policy.jsonl"))
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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--label", label,
                                "--warmup", str(args.warmup), "--reps", str(args.reps)],
                               env=env, capture_output=True, text=True, timeout=500)
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
