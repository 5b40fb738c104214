#!/usr/bin/env python3
"""One line per GPU kernel of the given .hip files: mangled name, SHA-256 of its assembly, VGPRs, SGPRs, scratch, LDS.

    tools/kernel_digest.py bioen_amd/csrc/kernels_forces.hip ... [--extra=-DSTRIP_DIAG=4] [-j 8] > table.txt
    tools/kernel_digest.py --compare before.txt after.txt
    tools/kernel_digest.py old/kernels_x.hip --rename 11FGram16ArgsE=9FGramArgsE > before.txt

Each file is compiled with the Makefile's flags plus `--cuda-device-only -S` into a temporary directory (no GPU needed).  A
kernel's text runs from its label to its `.Lfunc_end`, the `.amdhsa_kernel` block included; before hashing, local labels are
renumbered (`.LBB<n>_` -> `.LBB_`), comments dropped and whitespace collapsed, so that a kernel hashes the same whichever file
it is compiled from and whatever stands in front of it there.  Two trees whose tables are equal run the same instructions.
`--rename OLD=NEW` replaces OLD by NEW throughout the assembly before anything is hashed: for a kernel whose mangled name
changed between the two trees (an argument struct renamed) and whose instructions are to be compared all the same.
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bioen_amd", "csrc")
FIELDS = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("scratch", "private_segment_fixed_size"),
          ("lds", "group_segment_fixed_size"))


def makefile_flags():
    """HIPCC and CXXFLAGS as csrc/Makefile sets them ($(ARCH) and $(EXTRA) expanded here)."""
    var = {}
    with open(os.path.join(CSRC, "Makefile")) as f:
        for line in f:
            m = re.match(r"(\w+)\s*\??=\s*(.*)", line)
            if m:
                var.setdefault(m.group(1), m.group(2).strip())
    flags = var["CXXFLAGS"].replace("$(ARCH)", var["ARCH"]).replace("$(EXTRA)", "").split()
    flags = ["-I" + os.path.join(CSRC, f[2:]) if f.startswith("-I") else f for f in flags]
    return os.environ.get("HIPCC", var["HIPCC"]), flags


def kernels_of(asm):
    """{name: (digest, {field: value})} of one assembly file."""
    lines = asm.splitlines()
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    label = {m.group(1): i for i, m in enumerate(re.match(r"(\w+):", ln) for ln in lines) if m}
    out = {}
    for name in names:
        first = label[name]
        last = next(i for i in range(first, len(lines)) if lines[i].startswith(".Lfunc_end"))
        text = []
        for ln in lines[first:last + 1]:
            ln = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+", r".\1", ln.split(";")[0])
            ln = " ".join(ln.split())
            if ln:
                text.append(ln)
        body = "\n".join(text)
        desc = {short: re.search(r"\.amdhsa_%s (\S+)" % key, body).group(1) for short, key in FIELDS}
        out[name] = (hashlib.sha256(body.encode()).hexdigest(), desc)
    return out


def digest_file(path, hipcc, flags, tmp, renames=()):
    s = os.path.join(tmp, os.path.basename(path) + ".s")
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-o", s, path], stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    with open(s) as f:
        asm = f.read()
    for old, new in renames:
        asm = asm.replace(old, new)
    return kernels_of(asm)


def compare(a, b):
    def table(path):
        with open(path) as f:
            return {ln.split()[0]: ln.split()[1:] for ln in f if ln.startswith("_Z")}
    ta, tb = table(a), table(b)
    moved = sorted(k for k in ta.keys() & tb.keys() if ta[k] != tb[k])
    only_a, only_b = sorted(ta.keys() - tb.keys()), sorted(tb.keys() - ta.keys())
    for tag, ks in (("differs", moved), ("only in " + a, only_a), ("only in " + b, only_b)):
        for k in ks:
            print(tag + ": " + k)
    print("%d kernels in %s, %d in %s: %d differ, %d + %d unmatched" % (len(ta), a, len(tb), b, len(moved), len(only_a), len(only_b)))
    return 1 if moved or only_a or only_b else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="*")
    ap.add_argument("--extra", action="append", default=[], help="a further compiler flag (the Makefile's EXTRA=)")
    ap.add_argument("-j", type=int, default=1, help="files compiled side by side")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="replace OLD by NEW in the assembly before hashing")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two tables written by this tool")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    hipcc, flags = makefile_flags()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    merged = {}
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(args.j) as pool:
        for ks in pool.map(lambda p: digest_file(p, hipcc, flags + args.extra, tmp, renames), args.files):
            dup = merged.keys() & ks.keys()
            if dup:
                sys.exit("kernel defined twice: " + sorted(dup)[0])
            merged.update(ks)
    for name in sorted(merged):
        sha, d = merged[name]
        print(name, sha, *("%s=%s" % (short, d[short]) for short, _ in FIELDS))
    return 0


if __name__ == "__main__":
    sys.exit(main())
