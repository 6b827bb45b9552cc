"""The compile-time switches of lqr.jl_amd/csrc are an explicit, short list (CPU, source scan only).

Every `#ifndef NAME` / `#define NAME default` pair, and every `#ifdef` / `#if defined(...)` /
`#ifndef` of a name that no file of the tree defines, is a switch that a `-D` on the compiler's
command line can flip.  The set found must equal SWITCHES below: diagnostics (timing ablations,
debug checks, the test-only wait slack, the build-provenance hash), no settled A/B alternative.
A new switch has to be added here deliberately; a settled one is folded into the code instead.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lqr.jl_amd", "csrc")

# name → file that declares it (once, in the block at the top of that file)
SWITCHES = {
    "KB_ABL": "lqrx_kkt_big.hip",              # timing ablations of the general forward kernel (wrong results)
    "KB_PROF": "lqrx_kkt_big.hip",             # per-phase shader-clock counters (timing only)
    "KF_NOLEAF": "lqrx_kkt_big.hip",           # no 16×16 leaf factor (timing only, wrong results)
    "KU_ABL_MM": "lqrx_kkt_big.hip",           # fused stream without its MFMAs (timing only, wrong results)
    "LQRX_FIL_ABL": "lqrx_kkt_fil.hip",        # ablations of the LDS-ring kernel (timing only, wrong results)
    "LQRX_FIL_WAIT_SLACK": "lqrx_kkt_fil.hip", # negative control of tests/test_isa_guards.py
    "LQRX_DP_TVABL": "lqrx_dp.hip",            # time-varying inputs re-read from knot 1 (timing only)
    "LQRX_DP_TVEXTRA": "lqrx_dp.hip",          # extra VAR bits of the time-varying launch (timing only)
    "LQRX_KKT_DMACHECK": "lqrx_kkt.hip",       # debug: staged images compared against global reads
    "LQRX_SRC_HASH": "lqrx_api.cpp",           # build provenance, set by the Makefile
}
INCLUDE_GUARDS = set()                         # the headers use #pragma once


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".cpp")):
            text = open(os.path.join(CSRC, f), encoding="utf-8").read()
            # comments out, line continuations joined
            text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).replace("\\\n", " ")
            yield f, text


def _scan():
    defined, guarded, tested = set(), {}, {}
    for f, text in _sources():
        lines = [ln.strip() for ln in text.split("\n") if ln.strip()]
        for i, ln in enumerate(lines):
            m = re.match(r"#\s*define\s+(\w+)", ln)
            if m:
                defined.add(m.group(1))
            m = re.match(r"#\s*ifndef\s+(\w+)", ln)
            if m:
                nxt = lines[i + 1] if i + 1 < len(lines) else ""
                if re.match(r"#\s*define\s+%s\b" % re.escape(m.group(1)), nxt):
                    guarded.setdefault(m.group(1), []).append(f)
                else:
                    tested.setdefault(m.group(1), set()).add(f)
            m = re.match(r"#\s*ifdef\s+(\w+)", ln)
            if m:
                tested.setdefault(m.group(1), set()).add(f)
            if re.match(r"#\s*(if|elif)\b", ln):
                for name in re.findall(r"defined\s*\(?\s*(\w+)", ln):
                    tested.setdefault(name, set()).add(f)
    undefined = {n: fs for n, fs in tested.items() if n not in defined and not n.startswith("__")}
    return guarded, undefined


def test_scanner_sees_the_sources():
    names = [f for f, _ in _sources()]
    assert len([f for f in names if f.endswith(".hip")]) >= 10 and "lqrx_api.cpp" in names, names


def test_build_switches_are_the_declared_list():
    guarded, undefined = _scan()
    found = set(guarded) | set(undefined)
    assert found == set(SWITCHES) | INCLUDE_GUARDS, (sorted(found - set(SWITCHES) - INCLUDE_GUARDS),
                                                      sorted(set(SWITCHES) - found))


def test_each_switch_is_declared_once_in_its_file():
    guarded, undefined = _scan()
    for name, where in SWITCHES.items():
        files = guarded.get(name, []) or sorted(undefined.get(name, ()))
        assert set(files) == {where}, (name, files)
        assert len(guarded.get(name, [])) <= 1, (name, guarded[name])
