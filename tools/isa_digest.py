#!/usr/bin/env python3
"""Digest of the gfx950 device code of every kernel unit: `sha256  unit` per .hip file.

Each lqr.jl_amd/csrc/*.hip is compiled with the Makefile's own HIPCC / ARCH / CXXFLAGS plus
`--cuda-device-only -S` (the compiles run concurrently), `__hip_cuid_<hex>` — a symbol that hashes
the source text — is replaced by a fixed token, and the SHA-256 of the listing is printed.  Two
trees whose digests agree ship the same device code: the evidence for a refactor of these files
(profiles/r08/knobs/).  Reads nothing but the tree; needs no GPU.

  tools/isa_digest.py [--root TREE] [--jobs N] [--keep DIR] [unit.hip ...]
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


def digest(csrc, hipcc, flags, unit, keep):
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", unit, "-o", "-"],
                       cwd=csrc, capture_output=True)
    if r.returncode:
        return unit, None, r.stderr.decode(errors="replace")
    asm = re.sub(rb"__hip_cuid_[0-9a-f]+", b"__hip_cuid_X", r.stdout)
    if keep:
        (keep / (unit + ".s")).write_bytes(asm)
    return unit, hashlib.sha256(asm).hexdigest(), ""


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", type=pathlib.Path, default=pathlib.Path(__file__).resolve().parent.parent,
                    help="tree to digest (default: the one this script is in)")
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
    bad = 0
    with concurrent.futures.ThreadPoolExecutor(max(1, a.jobs)) as ex:
        for unit, sha, err in ex.map(lambda u: digest(csrc, hipcc, flags, u, a.keep), units):
            if sha is None:
                bad += 1
                print(f"isa_digest: {unit} failed to compile\n{err}", file=sys.stderr)
            else:
                print(f"{sha}  {unit}", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
