"""The DP solve entries' argument table (lqrx._lib.DP_ENTRY_ARGS) against include/lqrx.h, the ctypes
signatures generated from it, and the argument code of every pointer of every entry.  No device is
needed: every code below is decided before the library touches one.
"""
import ctypes as C
import re

import numpy as np
import pytest

KINDS = ("lqrx_dp_solve", "lqrx_dp_solve_linear", "lqrx_dp_solve_affine", "lqrx_dp_solve_cross",
         "lqrx_dp_solve_value")
ENTRIES = [k + s for k in KINDS for s in ("", "_host")] + [k + "_host_devices" for k in KINDS[:2]]
OPTIONAL = ("info", "stream")              # NULL is a valid argument
LIN_MEMBERS = ("q", "r", "qf", "d", "p")


def header_params(name):
    """[(type, name), …] of the prototype of `name` in include/lqrx.h, desc first."""
    from lqrx import _lib

    src = open(_lib.HEADER_PATH).read()
    mt = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, re.M)
    assert mt, name
    out = []
    for prm in mt.group(1).split(","):
        ty, nm = re.fullmatch(r"\s*(.*?)(\w+)\s*", prm, re.S).groups()
        out.append((" ".join(ty.split()), nm))
    assert out[0] == ("const lqrx_dp_desc *", "desc")
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_table_follows_the_header(lqrx, entry):
    from lqrx import _lib

    assert sorted(_lib.DP_ENTRY_ARGS) == sorted(ENTRIES)
    assert list(_lib.DP_ENTRY_ARGS[entry]) == [nm for _, nm in header_params(entry)[1:]]


def test_generated_signatures_are_the_literal_ones(lqrx):
    """The argtypes of the twelve entries as they were written out by hand before the table."""
    from lqrx import _lib

    D, L, W, V, I = C.POINTER(_lib.DpDesc), C.POINTER(_lib.DpLinear), C.POINTER(_lib.DpValue), C.c_void_p, C.c_int32
    want = {
        "lqrx_dp_solve": [D] + [V] * 10 + [V, V],
        "lqrx_dp_solve_host": [D] + [V] * 10 + [V],
        "lqrx_dp_solve_linear": [D] + [V] * 6 + [L] + [V] * 4 + [V, V],
        "lqrx_dp_solve_linear_host": [D] + [V] * 6 + [L] + [V] * 5,
        "lqrx_dp_solve_affine": [D] + [V] * 7 + [L] + [V] * 4 + [V, V],
        "lqrx_dp_solve_affine_host": [D] + [V] * 7 + [L] + [V] * 5,
        "lqrx_dp_solve_cross": [D] + [V] * 8 + [L] + [V] * 4 + [V, V],
        "lqrx_dp_solve_cross_host": [D] + [V] * 8 + [L] + [V] * 5,
        "lqrx_dp_solve_value": [D] + [V] * 8 + [L] + [W] + [V] * 4 + [V, V],
        "lqrx_dp_solve_value_host": [D] + [V] * 8 + [L] + [W] + [V] * 5,
        "lqrx_dp_solve_host_devices": [D] + [V] * 10 + [V, V, I],
        "lqrx_dp_solve_linear_host_devices": [D] + [V] * 6 + [L] + [V] * 5 + [V, I],
    }
    assert sorted(want) == sorted(ENTRIES)
    for name, args in want.items():
        assert _lib._SIGS[name] == (C.c_int, args), name
        assert getattr(lqrx.load(), name).argtypes == args, name


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_sweep_gives_the_argument_position(lqrx, entry):
    """A valid descriptor (n=8, m=4, N=10, batch=4); each argument NULL in turn, and each member of
    lin (val->s too; val->dV and val->J may be NULL): the code is minus the argument's position in
    the header's prototype, the text names the argument.  ndev = 0 gives ndev's position."""
    from lqrx import _lib

    lib = lqrx.load()
    fn = getattr(lib, entry)
    params = header_params(entry)
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.c_void_p)
    dv = np.zeros(1, np.int32)
    desc = _lib.DpDesc(8, 4, 10, 0, 4, 0, 0, 0, 0)
    keep = []

    def args(null=None, member=None):
        a = []
        for ty, nm in params:
            if nm == "desc":
                v = C.byref(desc)
            elif nm in OPTIONAL:
                v = None
            elif nm == "lin":
                s = _lib.DpLinear(*[None if member == (nm, k) else p.value for k in LIN_MEMBERS])
                keep.append(s)
                v = C.byref(s)
            elif nm == "val":
                s = _lib.DpValue(None if member == (nm, "s") else p.value,
                                 None if member == (nm, "opt") else p.value, None if member == (nm, "opt") else p.value)
                keep.append(s)
                v = C.byref(s)
            elif nm == "ndev":
                v = 1
            elif nm == "devices":
                v = dv.ctypes.data_as(C.c_void_p)
            else:
                assert ty in ("const void *", "void *"), (ty, nm)
                v = p
            if nm == null:
                v = 0 if nm == "ndev" else None
            a.append(v)
        return a

    swept = 0
    for pos, (ty, nm) in enumerate(params, start=1):
        if nm in OPTIONAL:
            continue
        assert fn(*args(null=nm)) == -pos, (entry, nm, lib.lqrx_last_error().decode())
        if nm != "desc":
            assert nm in lib.lqrx_last_error().decode()
        swept += 1
        for k in LIN_MEMBERS if nm == "lin" else ("s",) if nm == "val" else ():
            assert fn(*args(member=(nm, k))) == -pos, (entry, nm, k, lib.lqrx_last_error().decode())
            assert k in lib.lqrx_last_error().decode()
    assert swept == len(params) - sum(nm in OPTIONAL for _, nm in params)
    if "val" in [nm for _, nm in params]:      # dV, J NULL: validation goes on to the next fault
        a = args(member=("val", "opt"), null="U")
        assert fn(*a) == -(1 + [nm for _, nm in params].index("U"))


def test_linear_entries_report_the_descriptor_first(lqrx):
    """An invalid descriptor and lin == NULL together: −1, as in every other entry."""
    from lqrx import _lib

    lib = lqrx.load()
    p = np.zeros(16).ctypes.data_as(C.c_void_p)
    bad = _lib.DpDesc(0, 4, 10, 0, 4, 0, 0, 0, 0)
    dv = np.zeros(1, np.int32).ctypes.data_as(C.c_void_p)
    assert lib.lqrx_dp_solve_linear(C.byref(bad), p, p, p, p, p, p, None, p, p, p, p, None, None) == -1
    assert lib.lqrx_dp_solve_linear_host(C.byref(bad), p, p, p, p, p, p, None, p, p, p, p, None) == -1
    assert lib.lqrx_dp_solve_linear_host_devices(C.byref(bad), p, p, p, p, p, p, None, p, p, p, p, None, dv, 1) == -1
