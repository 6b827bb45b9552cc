"""Instruction tally of a kernel's knot loop — every block of the loop, all paths — from a gfx950 listing.

    python tools/knot_loop_tally.py ASM.s FUNCTION_SUBSTRING

The loop is the depth-1 loop of the function that holds the most MFMAs; the columns are
tools/knot_tally.py's.  A static count over all of the loop's blocks (the Newton–Schulz rounds past
the first and the exact sweep included), so two variants of a kernel compare by their difference;
the common path alone is what tools/knot_tally.py counts from hand-picked blocks.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knot_tally import tally  # noqa: E402

COLS = ["mfma", "valu", "lane", "dpp", "mov", "nop_ws", "salu", "lds", "vmem", "waitcnt"]


def function_body(listing, fn):
    """(symbol, lines) of the first function whose symbol contains fn, label to .Lfunc_end."""
    name = next(n for n in re.findall(r"^(_Z\w+):", listing, re.M) if fn in n)
    start = listing.find(name + ":")
    return name, listing[start:listing.find(".Lfunc_end", start)].split("\n")


def loop_extent(body, i, label):
    """[lo, hi) of the loop headed by `label` at line i: its header, every block the listing tags as
    in the loop, and its back edges; hi runs to the end of the last such block."""
    back = [j for j, x in enumerate(body) if j > i and re.search(r"s_c?branch\S*\s+" + re.escape(label) + r"\b", x)]
    tag = "Header=" + label[2:]
    tagged = [j for j, x in enumerate(body) if tag in x]
    lo, hi = min([i] + tagged), max(back + tagged + [i]) + 1
    while hi < len(body) and not re.match(r"\.LBB\d+_\d+:", body[hi]):
        hi += 1
    return lo, hi


def main():
    path, fn = sys.argv[1], sys.argv[2]
    name, body = function_body(open(path).read(), fn)
    best = None
    for i, line in enumerate(body):
        m = re.match(r"(\.LBB\d+_\d+):.*Loop Header: Depth=1", line)
        if not m:
            continue
        lo, hi = loop_extent(body, i, m.group(1))
        c = tally(body[lo:hi])
        if best is None or c["mfma"] > best[0]["mfma"]:
            best = (c, lo, hi, m.group(1))
    c, lo, hi, label = best
    print(name)
    print(f"knot loop {label}, listing lines {lo}-{hi} of the function (every block of the loop, all paths)")
    print("".join(f"{k:>9s}" for k in COLS))
    print("".join(f"{c[k]:9d}" for k in COLS))


if __name__ == "__main__":
    main()
