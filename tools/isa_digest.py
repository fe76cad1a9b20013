#!/usr/bin/env python3
"""Digest of the device code of every csrc/*.hip: one JSON object keyed by kernel symbol.

Each file is compiled with build.HIPCC_FLAGS plus "--cuda-device-only -S" (no GPU needed) and every kernel in the
assembly gets {"sha256", and from its .amdhsa_kernel block "vgpr" (next_free_vgpr), "sgpr" (next_free_sgpr), "accum_offset",
"lds" (group_segment_fixed_size) and "scratch" (private_segment_fixed_size)}, one kernel per line.  Two trees whose
digests are equal run the same instructions with the same register, LDS and scratch use: the check for a change that
is meant to move or deduplicate source only.

What is hashed is the text between the kernel's label and its .Lfunc_end label, minus comments and assembler
directives, with the function index taken out of the basic-block labels (.LBB<f>_<n> -> .LBB_<n>: <f> counts the
functions of the file and changes when a kernel moves to another file).  Mnemonics and all other operands are hashed
as the compiler wrote them.

    python tools/isa_digest.py --out profiles/r06_isa_digest.json [--root OTHER_TREE] [--keep DIR] [--jobs N]
    python tools/isa_digest.py --compare A.json B.json
"""
from __future__ import annotations

import argparse
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

# .amdhsa_<directive> -> key in the digest
RESOURCES = {"next_free_vgpr": "vgpr", "next_free_sgpr": "sgpr", "accum_offset": "accum_offset", "group_segment_fixed_size": "lds",
             "private_segment_fixed_size": "scratch"}
LBB = re.compile(r"\.LBB\d+_(\d+)")


def load_build(root):
    spec = importlib.util.spec_from_file_location("_emd_build", os.path.join(root, "ai-cv-automation-elect-micr_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def kernels_of(asm_text):
    """{symbol: {"sha256", resources...}} of one device assembly file."""
    lines = [l.split(";")[0].rstrip() for l in asm_text.splitlines()]   # ';' starts a comment, to the end of the line
    out = {}
    for i, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        sym, res = m.group(1), {}
        for l in lines[i + 1:]:
            if l.strip() == ".end_amdhsa_kernel":
                break
            f = l.split()
            if len(f) == 2 and f[0].startswith(".amdhsa_") and f[0][len(".amdhsa_"):] in RESOURCES:
                res[RESOURCES[f[0][len(".amdhsa_"):]]] = int(f[1], 0)
        assert set(res) == set(RESOURCES.values()), (sym, res)
        out[sym] = res
    # a device function that is not inlined would run outside every kernel's hash: there must be none
    funcs = {m.group(1) for l in lines if (m := re.match(r"\s*\.type\s+(\S+),@function", l))}
    assert funcs == set(out), f"functions without a kernel descriptor: {sorted(funcs - set(out))}"
    for sym, res in out.items():
        start = lines.index(sym + ":")
        body = []
        for l in lines[start + 1:]:
            s = l.strip()
            if s.startswith(".Lfunc_end"):
                break
            if not s or s.startswith(";") or (s.startswith(".") and not s.endswith(":")):
                continue
            body.append(LBB.sub(r".LBB_\1", s))
        else:
            raise AssertionError(f"no end label behind {sym}")
        res["sha256"] = hashlib.sha256("\n".join(body).encode()).hexdigest()
    return out


def digest(root, keep, jobs):
    b = load_build(root)
    srcs = [s for s in b.sources() if s.endswith(".hip")]
    hipcc = b._hipcc()
    with tempfile.TemporaryDirectory() as tmp:
        asm_dir = keep or tmp
        os.makedirs(asm_dir, exist_ok=True)

        def one(src):
            dst = os.path.join(asm_dir, os.path.splitext(os.path.basename(src))[0] + ".s")
            r = subprocess.run([hipcc, *b.HIPCC_FLAGS, "--cuda-device-only", "-S", src, "-o", dst], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
            with open(dst) as f:
                return kernels_of(f.read())

        with ThreadPoolExecutor(max_workers=max(1, min(jobs, 16))) as ex:
            per_file = list(ex.map(one, srcs))
    out = {}
    for ks in per_file:
        assert not set(ks) & set(out), sorted(set(ks) & set(out))
        out.update(ks)
    return dict(sorted(out.items()))


def compare(a, b):
    """Lines that name every difference."""
    keys = ("sha256", *RESOURCES.values())
    diffs = [f"only in the first: {s}" for s in sorted(set(a) - set(b))] + [f"only in the second: {s}" for s in sorted(set(b) - set(a))]
    for s in sorted(set(a) & set(b)):
        for k in keys:
            if a[s][k] != b[s][k]:
                diffs.append(f"{s}: {k} {a[s][k]} -> {b[s][k]}")
    return diffs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree to digest (default: this one)")
    ap.add_argument("--out", help="JSON file to write (default: stdout)")
    ap.add_argument("--keep", help="directory that keeps the .s files")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two digests; exit status 1 if they differ")
    a = ap.parse_args()
    if a.compare:
        da, db = (json.load(open(p)) for p in a.compare)
        diffs = compare(da, db)
        print("\n".join(diffs + [f"{len(da)} / {len(db)} kernels, {len(diffs)} differences"]))
        return 1 if diffs else 0
    d = digest(a.root, a.keep, a.jobs)
    text = "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in d.items()) + "\n}\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
