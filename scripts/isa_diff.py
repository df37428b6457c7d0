#!/usr/bin/env python3
"""Compare the device assembly of two builds, kernel by kernel.

    make -C fl-tee_amd asm BUILD=/tmp/a        # on one tree
    make -C fl-tee_amd asm BUILD=/tmp/b        # on the other
    scripts/isa_diff.py /tmp/a /tmp/b

For every function of every *.s file (kernels and the device functions hipcc did not
inline) the instruction body and, for kernels, the .amdhsa_* descriptor values are
compared after normalising the function's own symbol name and the per-function numbering
of local labels.  Each function is reported as identical, changed, only-in-A or only-in-B;
an only-in-A and an only-in-B function with equal bodies are a rename (a template
parameter was dropped).  Exit status 1 on any changed or only-in-B function.  The last
column says whether the two files are the same text as a whole, the __hip_cuid_<hash>
symbol apart (hipcc derives it from the source path).

CPU only: it reads text files.  -v lists the identical functions too.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys

TYPE_RE = re.compile(r"^\s*\.type\s+(\S+),@function")
LABEL_RE = re.compile(r"\.L([A-Za-z_]+?)(\d+)_(\d+)")
FUNC_RE = re.compile(r"\.Lfunc_(begin|end)\d+")
COMMENT_BB_RE = re.compile(r"\bBB\d+_(\d+)")  # "Header=BB12_3" in the loop comments
KERNEL_RE = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
CUID_RE = re.compile(r"__hip_cuid_[0-9a-f]+")


def parse(path):
    """{symbol: normalised text} of one assembly file."""
    bodies, descs = {}, {}
    name, buf, kern = None, None, None
    with open(path, errors="replace") as f:
        for line in f:
            if name is None and kern is None:
                m = TYPE_RE.match(line)
                if m:
                    name, buf = m.group(1), []
                    continue
                m = KERNEL_RE.match(line)
                if m:
                    kern, buf = m.group(1), []
                continue
            s = line.strip()
            if name is not None:
                if s.startswith(".size") and name in s:
                    bodies[name] = buf
                    name = None
                    continue
                if s:
                    buf.append(" ".join(s.split()))  # (comment columns move with the label width)
            else:
                if s.startswith(".end_amdhsa_kernel"):
                    descs[kern] = buf
                    kern = None
                    continue
                if s.startswith(".amdhsa_"):
                    buf.append(s)
    out = {}
    for sym, body in bodies.items():
        text = "\n".join(body + ["--descriptor--"] + descs.get(sym, []))
        text = text.replace(sym, "@SELF")
        text = LABEL_RE.sub(lambda m: ".L%s_%s" % (m.group(1), m.group(3)), text)
        text = FUNC_RE.sub(lambda m: ".Lfunc_" + m.group(1), text)
        text = COMMENT_BB_RE.sub(lambda m: "BB_" + m.group(1), text)
        out[sym] = (hashlib.sha256(text.encode()).hexdigest(), sym in descs)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    lines = r.stdout.split("\n")
    return {n: (lines[i] if i < len(lines) and lines[i] else n) for i, n in enumerate(names)}


def same_text(a, b):
    """Whole-file equality, but for hipcc's __hip_cuid_<hash> symbol (it hashes the source
    path, so it differs between two checkouts of the same source)."""
    with open(a, errors="replace") as fa, open(b, errors="replace") as fb:
        while True:
            x, y = fa.readline(), fb.readline()
            if x != y and CUID_RE.sub("__hip_cuid_", x) != CUID_RE.sub("__hip_cuid_", y):
                return False
            if not x and not y:
                return True


def main(argv):
    verbose = "-v" in argv
    dirs = [a for a in argv[1:] if a != "-v"]
    if len(dirs) != 2:
        print(__doc__)
        return 2
    A, B = dirs
    files = sorted({f for d in (A, B) for f in os.listdir(d) if f.endswith(".s")})
    bad = False
    print("%-16s %7s %7s %9s %7s %7s %9s %9s  %s" % ("file", "A", "B", "identical", "renamed", "changed",
                                                    "only-in-A", "only-in-B", "file"))
    detail = []
    for f in files:
        pa, pb = os.path.join(A, f), os.path.join(B, f)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print("%-16s only in %s" % (f, A if os.path.exists(pa) else B))
            bad = bad or not os.path.exists(pa)
            continue
        a, b = parse(pa), parse(pb)
        ident = [n for n in a if n in b and a[n] == b[n]]
        changed = [n for n in a if n in b and a[n] != b[n]]
        only_a = [n for n in a if n not in b]
        only_b = [n for n in b if n not in a]
        by_hash = {}
        for n in only_b:
            by_hash.setdefault(b[n], []).append(n)
        renamed = []
        for n in list(only_a):
            cand = by_hash.get(a[n])
            if cand:
                renamed.append((n, cand.pop(0)))
                only_a.remove(n)
        gone_b = {m for _, m in renamed}
        only_b = [n for n in only_b if n not in gone_b]
        print("%-16s %7d %7d %9d %7d %7d %9d %9d  %s" % (
            f, len(a), len(b), len(ident), len(renamed), len(changed), len(only_a), len(only_b),
            "same" if same_text(pa, pb) else "differ"))
        bad = bad or bool(changed) or bool(only_b)
        names = demangle(changed + only_a + only_b + [x for p in renamed for x in p] + (ident if verbose else []))
        for n in changed:
            detail.append("%s: changed    %s" % (f, names[n]))
        for n in only_b:
            detail.append("%s: only-in-B  %s" % (f, names[n]))
        for n in only_a:
            detail.append("%s: only-in-A  %s" % (f, names[n]))
        for n, m in renamed:
            detail.append("%s: renamed    %s\n%s         -> %s" % (f, names[n], " " * len(f), names[m]))
        if verbose:
            for n in ident:
                detail.append("%s: identical  %s" % (f, names[n]))
    print()
    print("\n".join(detail))
    print("\nFAIL: changed or only-in-B functions" if bad else "\nOK: every function of B is identical to, or a rename of, one of A")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
