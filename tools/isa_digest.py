#!/usr/bin/env python3
"""Digest of the gfx950 device code of every kernel unit: `sha256  unit` per .hip file.

Each lqr.jl_amd/csrc/*.hip is compiled with the Makefile's own HIPCC / ARCH / CXXFLAGS plus
`--cuda-device-only -S` (the compiles run concurrently), `__hip_cuid_<hex>` — a symbol that hashes
the source text — is replaced by a fixed token, and the SHA-256 of the listing is printed.  Two
trees whose digests agree ship the same device code: the evidence for a refactor of these files
(profiles/r08/knobs/).  Reads nothing but the tree; needs no GPU.

With --per-kernel: one line `sha256  unit  symbol` per function, sorted by symbol, for a refactor
that reorders the functions of a unit (profiles/r09/kinds/).  The hash covers the function's body,
label to `.Lfunc_end`, and its `.amdhsa_kernel … .end_amdhsa_kernel` block, after stripping `;`
comments and trailing blanks and rewriting what only says where the function stands in the unit:
`BB<i>_<j>` → `BB_<j>`, `.Lfunc_end<i>` → `.Lfunc_end`, and the long-branch labels
`.Lpost_getpc<i>`, which the assembler printer numbers across the unit, renumbered from 0 in each
function.

  tools/isa_digest.py [--per-kernel] [--root TREE] [--jobs N] [--keep DIR] [unit.hip ...]
"""
import argparse
import concurrent.futures
import hashlib
import pathlib
import re
import subprocess
import sys


def make_var(makefile, name):
    """The (continued) right-hand side of `NAME = value` / `NAME ?= value` in the Makefile."""
    text = makefile.read_text().replace("\\\n", " ")
    m = re.search(rf"^{name}\s*\??=\s*(.*)$", text, re.M)
    if not m:
        sys.exit(f"isa_digest: no {name} in {makefile}")
    return m.group(1).strip()


def normalise(asm):
    return re.sub(rb"__hip_cuid_[0-9a-f]+", b"__hip_cuid_X", asm)


def per_kernel(asm):
    """{symbol: sha256} of every function of a listing (bytes), position-independent."""
    text = re.sub(r"[ \t]*;[^\n]*", "", normalise(asm).decode(errors="replace"))
    text = re.sub(r"[ \t]+$", "", text, flags=re.M)
    text = re.sub(r"BB\d+_(\d+)", r"BB_\1", text)
    text = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", text)
    funcs = set(re.findall(r"^\s*\.type\s+([^\s,]+),\s*@function", text, re.M))
    parts, sym, end = {f: [] for f in funcs}, None, None
    for line in text.split("\n"):
        if sym is None:
            m = re.match(r"\s*\.amdhsa_kernel (\S+)$", line)
            if line.endswith(":") and line[:-1] in funcs:
                sym, end = line[:-1], ".Lfunc_end:"
            elif m and m.group(1) in funcs:
                sym, end = m.group(1), ".end_amdhsa_kernel"
        if sym is not None:
            parts[sym].append(line)
            if line.strip() == end:
                sym = None
    if sym is not None or not all(parts.values()):
        sys.exit("isa_digest: a function without a body or an end in the listing")
    out = {}
    for f, lines in parts.items():
        body, order = "\n".join(lines), {}
        for lab in re.findall(r"\.Lpost_getpc\d+", body):     # numbered across the unit: renumber per function
            order.setdefault(lab, len(order))
        body = re.sub(r"\.Lpost_getpc\d+", lambda m: f".Lpost_getpc_{order[m.group(0)]}", body)
        out[f] = hashlib.sha256(body.encode()).hexdigest()
    return out


def digest(csrc, hipcc, flags, unit, keep, split):
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", unit, "-o", "-"],
                       cwd=csrc, capture_output=True)
    if r.returncode:
        return unit, None, r.stderr.decode(errors="replace")
    asm = normalise(r.stdout)
    if keep:
        (keep / (unit + ".s")).write_bytes(asm)
    return unit, per_kernel(asm) if split else hashlib.sha256(asm).hexdigest(), ""


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", type=pathlib.Path, default=pathlib.Path(__file__).resolve().parent.parent,
                    help="tree to digest (default: the one this script is in)")
    ap.add_argument("--per-kernel", action="store_true", help="one line per function instead of one per unit")
    ap.add_argument("--jobs", type=int, default=10)
    ap.add_argument("--keep", type=pathlib.Path, help="also write the normalised listings here")
    ap.add_argument("units", nargs="*", help="unit file names (default: every csrc/*.hip)")
    a = ap.parse_args()
    csrc = a.root / "lqr.jl_amd" / "csrc"
    mk = csrc / "Makefile"
    arch = make_var(mk, "ARCH")
    flags = make_var(mk, "CXXFLAGS").replace("$(ARCH)", arch).split()
    hipcc = make_var(mk, "HIPCC")
    units = a.units or sorted(p.name for p in csrc.glob("*.hip"))
    if a.keep:
        a.keep.mkdir(parents=True, exist_ok=True)
        a.keep = a.keep.resolve()
    bad, lines = 0, []
    with concurrent.futures.ThreadPoolExecutor(max(1, a.jobs)) as ex:
        for unit, sha, err in ex.map(lambda u: digest(csrc, hipcc, flags, u, a.keep, a.per_kernel), units):
            if sha is None:
                bad += 1
                print(f"isa_digest: {unit} failed to compile\n{err}", file=sys.stderr)
            elif a.per_kernel:
                lines += [(sym, f"{h}  {unit}  {sym}") for sym, h in sha.items()]
            else:
                print(f"{sha}  {unit}", flush=True)
    for _, line in sorted(lines):
        print(line)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
