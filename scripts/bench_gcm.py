"""Authenticated decryption (AES-128-GCM: fltee_decrypt_auth_device, k_aes.hip + k_ghash.hip)
against the plain CTR decryption (fltee_decrypt_device), device-resident, in ONE process.

    python scripts/bench_gcm.py [--shapes headline,c3] [--warmup 2] [--reps 5] [--out FILE]

Per shape (headline: 100 x 1M dense records, 800 MB; c3 = configs[2]: 100 x 5,089 records,
the small-payload kernels): warm-up calls, then `reps` interleaved event-timed calls of each;
one JSON line with both medians (and minima), their ratio, the bytes per second of each, and
the authenticated call's kernels from the launch trace.  Both entry points end with their own
stream synchronisation and upload their keys first, so the timings include that fixed host
part on both sides.  Appended to profiles/r08/gcm.jsonl by default."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fl-tee_amd"))
sys.path.insert(0, ROOT)

SHAPES = {"headline": (100, 1_000_000), "c3": (100, 5089)}
# VALU instructions of one gf128_mul per lane (k_ghash.hip's header; the bulk kernel's loop
# body in the gfx950 ISA) and what the bulk kernel spends per 16-byte block
GHASH_VALU_PER_MUL = 800
GHASH_MULS_PER_BLOCK = 1 + 1 / 8


def launches(torch, lib, call):
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
    out = []
    for line in buf.value.decode().splitlines():
        f = line.split("|")
        if f[0] == "launch":
            out.append([f[1], int(f[2]) >> 32, int(f[3]) & 0xFFFFFFFF])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,c3")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "gcm.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from fltee import _lib as L
    from fltee import client as C
    from fltee import device as D
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    iv = C.ecall_iv(9800, 3)
    for name in args.shapes.split(","):
        n, k = SHAPES[name]
        B = k * 8
        ids = np.arange(1, n + 1, dtype=np.uint32)
        aad = C.ecall_aad(9800, 3, ids, 3)
        plain = torch.randint(-2 ** 62, 2 ** 62, (n * k,), dtype=torch.int64, device="cuda")
        ctr = torch.empty_like(plain)
        D.decrypt(ids, plain, B, ctr)  # CTR: encryption == decryption
        gcm = C.encrypt_parameters_gcm(plain, ids, iv, aad).reshape(-1)
        rec = torch.empty_like(plain)
        calls = {"ctr": lambda: D.decrypt(ids, ctr, B, rec),
                 "gcm": lambda: D.decrypt_auth(ids, gcm, B, iv, aad, records=rec)}
        for _ in range(args.warmup):
            for c in calls.values():
                c()
        _, fail = calls["gcm"]()
        assert not fail.any().item() and D.status() == 0 and torch.equal(rec, plain)
        calls["ctr"]()
        assert torch.equal(rec, plain)
        times = {a: [] for a in calls}
        for _ in range(args.reps):
            for a, c in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                c()
                e1.record()
                torch.cuda.synchronize()
                times[a].append(e0.elapsed_time(e1))
        med = {a: float(np.median(t)) for a, t in times.items()}
        line = dict(shape=name, n=n, records_per_client=k, ciphertext_bytes=n * B, reps=args.reps,
                    ctr_ms=med["ctr"], gcm_ms=med["gcm"],
                    ctr_min_ms=float(np.min(times["ctr"])), gcm_min_ms=float(np.min(times["gcm"])),
                    ratio=med["gcm"] / med["ctr"],
                    ctr_gb_per_s=n * B / med["ctr"] / 1e6, gcm_gb_per_s=n * B / med["gcm"] / 1e6,
                    ghash_valu_per_block=GHASH_VALU_PER_MUL * GHASH_MULS_PER_BLOCK,
                    ghash_wave_instructions_per_block=GHASH_VALU_PER_MUL * GHASH_MULS_PER_BLOCK / 64,
                    gcm_launches=launches(torch, L.lib(), calls["gcm"]),
                    ctr_launches=launches(torch, L.lib(), calls["ctr"]),
                    version=L.lib().fltee_version().decode())
        text = json.dumps(line)
        print(text, flush=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")
        del plain, ctr, gcm, rec


if __name__ == "__main__":
    main()
