"""Per-section instruction tally of a path through a kernel's gfx950 listing.

    python tools/knot_tally.py ASM.s FUNCTION_SUBSTRING NAME:A-B[+C-D…] [NAME:…]

ASM.s: `hipcc --cuda-device-only -S` output.  A section is one or more ranges of line numbers
counted from the function's label (line 0), the numbering tools/chain_len.py prints — the basic
blocks the path of interest runs through, picked by reading the listing (a block is counted whole).
Per section: MFMA, other VALU (with the v_readlane/v_writelane, DPP and v_mov/v_cndmask among them
listed separately), s_nop wait states (s_nop N counts N + 1), other SALU, LDS, vector-memory
instructions and s_waitcnt.  Counts are static issue counts of the listed blocks, not times.
"""
import re
import sys
from collections import Counter


def tally(lines):
    c = Counter()
    for l in lines:
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        op, _, rest = t.partition(" ")
        if "mfma" in op:
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if op.startswith(("v_readlane", "v_writelane")):
                c["lane"] += 1
            if "dpp" in op or "row_shr" in rest or "row_bcast" in rest:
                c["dpp"] += 1
            if op.startswith(("v_mov", "v_cndmask", "v_accvgpr")):
                c["mov"] += 1
        elif op == "s_nop":
            c["nop_ws"] += int(rest.strip() or 0) + 1
        elif op == "s_waitcnt":
            c["waitcnt"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        else:
            c["vmem"] += 1
    return c


def main():
    path, fn = sys.argv[1], sys.argv[2]
    s = open(path).read()
    name = next(n for n in re.findall(r"^(_Z\w+):", s, re.M) if fn in n)
    body = s[s.find(name + ":"):s.find(".Lfunc_end", s.find(name + ":"))].split("\n")
    cols = ["mfma", "valu", "lane", "dpp", "mov", "nop_ws", "salu", "lds", "vmem", "waitcnt"]
    print(name)
    print(f"{'section':14s}" + "".join(f"{c:>8s}" for c in cols) + "   lines")
    tot = Counter()
    for spec in sys.argv[3:]:
        sec, _, rng = spec.partition(":")
        lines = []
        for part in rng.split("+"):
            a, b = (int(v) for v in part.split("-"))
            lines += body[a:b + 1]
        c = tally(lines)
        tot.update(c)
        print(f"{sec:14s}" + "".join(f"{c[k]:8d}" for k in cols) + "   " + rng)
    print(f"{'total':14s}" + "".join(f"{tot[k]:8d}" for k in cols))


if __name__ == "__main__":
    main()
