"""Guard-zone tests of the DP family: no device entry of lqrx_dp_solve[_linear|_affine|_cross|_value]
or lqrx_dp_compute_ctg reads or writes outside the documented extents of its arguments, and each
writes every element of every output.

Every case runs the same entry twice on the null stream: once on plain exact-size tensors whose
outputs are pre-filled with the guard pattern (never torch.empty, which hands back the previous
solve's values), once on tensors from tests/guarded.py ([NaN guard | payload | NaN guard], outputs
filled with the pattern too).  Asserted: guarded.check() passes (every guard of every input and
output untouched, every output element written and finite); the guarded outputs are the plain
outputs bit for bit (a read past an input that reached the result would differ, the neighbour now
being a NaN); info == 0; and the plain outputs meet the project's checkers at the project's
tolerances — dp_truth.dp_solve_abi_np for K, P, X, U, d, p and for s, dV, J,
TOL64 = 1e-10 / TOL32 = 1e-4 on the measures of tests/test_dp_cross_gpu.py and test_dp_value_gpu.py.
No tolerance is introduced here.

Shapes (n, m, N, batch) are the smallest that reach each kernel and each padding case; N ≤ 5.
The n ≤ 4 shapes run under LQRX_DP_SMALL = lane, quad and hex where those kernels serve the kind
(quad: plain and linear, time-invariant; hex: plain, time-invariant).

Observed on an MI355X (every figure here is from the run kept in
profiles/r08/guards/guard_gpu_tests.log: the four test_guard_*_gpu.py files together, 314 cases,
4.09 s wall; the slowest case, 0.28 s, is the first, which loads the library).
No guard was touched and no output element was left unwritten.  Worst parity error per family, the
largest of K, P, d, p, X, U, s, dV, J on the measures above: n ≤ 4 kernels fp64 7.9e-15, fp32 2.8e-6;
register tiles fp64 7.0e-15, fp32 1.9e-6; workgroup kernel fp64 6.2e-15, fp32 3.4e-6;
lqrx_dp_compute_ctg 2.2e-15.  The `_host` entries are compared bit for bit (no figure).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from dp_truth import (cross_problem, dp_solve_abi_np, logical, relerr_per_knot, relerr_traj, to_batch,
                      value_errors)
from guarded import check as guard_check, guard_all, pattern_filled

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL32 = 1e-4
SMALL = [(1, 1, 2, 3), (3, 2, 5, 5), (4, 4, 4, 67)]
TILES = [(5, 2, 3, 3),      # 1×1 tile, padded
         (16, 16, 3, 2),    # 1×1 exact
         (17, 5, 3, 3),     # 2×1 padded
         (24, 18, 3, 2),    # 2×2 padded
         (33, 17, 3, 2),    # 4×2 padded
         (63, 31, 3, 2),    # 4×2 padded by one
         (64, 32, 3, 2)]    # 4×2 full: fp64 four-wave kernel (plain, linear), one-wave (affine, cross, value)
BIG = [(65, 33, 3, 2), (130, 5, 3, 2)]      # dp_big_kernel
SHAPES = SMALL + TILES + BIG
# kind → the optional inputs it passes, in the order the kinds nest
KINDS = {"plain": (), "linear": ("q", "r", "qf"), "affine": ("q", "r", "qf", "c"),
         "cross": ("q", "r", "qf", "c", "M"), "value": ("q", "r", "qf", "c", "M")}
OPTIONAL = ("q", "r", "qf", "c", "M")


def family(shape):
    return "small" if shape in SMALL else "tiles" if shape in TILES else "big"


def _modes(shape, kind, tv):
    """LQRX_DP_SMALL settings worth running for an n ≤ 4 shape: the lane kernel always, the quad
    kernel where it serves (plain, linear; time-invariant), the hex kernel (plain only)."""
    if shape not in SMALL:
        return ("",)
    if tv or kind not in ("plain", "linear"):
        return ("lane",)
    return ("lane", "quad", "hex") if kind == "plain" else ("lane", "quad")


def _cases():
    out = []
    for sh in SHAPES:
        for kind in KINDS:                                     # every kind, fp64, layout 0
            for pm, tv in ((0, 0), (1, 1)):
                out += [(sh, kind, 0, pm, tv, "f64", mode) for mode in _modes(sh, kind, tv)]
        for kind in ("plain", "value"):                        # layout 1
            for pm in (0, 1):
                out += [(sh, kind, 1, pm, 0, "f64", mode) for mode in _modes(sh, kind, 0)]
        out.append((sh, "value", 0, 1, 1, "f32", _modes(sh, "value", 1)[0]))
    return out


CASES = _cases()


def _id(c):
    sh, kind, lay, pm, tv, prec, mode = c
    return f"{'x'.join(map(str, sh))}-{kind}-l{lay}-p{pm}-tv{tv}-{prec}" + (f"-{mode}" if mode else "")


@functools.lru_cache(maxsize=None)
def problem(shape, tv):
    """One cross problem per (shape, time-varying): computed once, shared, never modified."""
    import lqrx

    n, m, N, bt = shape
    d = cross_problem(lqrx, n, m, N, bt, 9300 + 17 * n + m, tv_QR=bool(tv), tv_AB=bool(tv))
    d["tv_AB"] = d["tv_QR"] = int(tv)
    return d


@functools.lru_cache(maxsize=None)
def truth(shape, tv, kind, pm):
    """The checker's result for a kind: the inputs the kind does not pass are zeros."""
    d = dict(problem(shape, tv))
    for k in OPTIONAL:
        if k not in KINDS[kind]:
            d[k] = np.zeros_like(d[k])
    N = shape[2]
    return dp_solve_abi_np(d, N, "value", all_P=bool(pm)) if kind == "value" else dp_solve_abi_np(d, N, "cross", all_P=bool(pm))


def out_sizes(shape, kind, pm):
    """Elements of every output of a kind (include/lqrx.h); info is int32."""
    n, m, N, bt = shape
    kP = N if pm else 1
    sz = dict(K=bt * (N - 1) * m * n, P=bt * n * n * kP, X=bt * N * n, U=bt * (N - 1) * m, info=bt)
    if kind != "plain":
        sz.update(d=bt * (N - 1) * m, p=bt * n * kP)
    if kind == "value":
        sz.update(s=bt * kP, dV=bt, J=bt)
    return sz


def upload(d, shape, kind, layout, npdt):
    """The kind's inputs as exact-size device tensors in the given layout, plus n, m, batch, tv."""
    import torch
    from lqrx.dp import to_soa

    n, m, N, bt = shape
    lay = (lambda a: to_soa(a, bt)) if layout == 1 else (lambda a: a)
    t = {k: torch.from_numpy(np.ascontiguousarray(lay(np.ascontiguousarray(d[k], npdt))).reshape(-1)).to("cuda:0")
         for k in ("A", "B", "Q", "R", "Qf", "x0") + KINDS[kind]}
    t.update(n=n, m=m, batch=bt, tv_AB=d["tv_AB"], tv_QR=d["tv_QR"])
    return t


def plain_outputs(t, sizes):
    """Exact-size outputs holding the fill pattern."""
    import torch

    like_i = torch.empty(1, dtype=torch.int32, device="cuda:0")
    return {k: pattern_filled(like_i if k == "info" else t["A"], sz) for k, sz in sizes.items()}


def bits(x):
    import torch

    return x.view({8: torch.int64, 4: torch.int32}[x.element_size()])


def same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def parity(o, ref, shape, kind, pm, layout, tol, what):
    """The measures of test_dp_affine_gpu.check (K, P per knot; d, p on the trajectory's scale; X, U
    on max(1, max|ref|)) and of dp_truth.value_errors; prints every figure, then asserts."""
    from lqrx.dp import from_soa

    n, m, N, bt = shape
    unlay = (lambda a: from_soa(a, bt)) if layout == 1 else (lambda a: a)
    host = {k: unlay(np.asarray(v.cpu().numpy(), np.float64)) for k, v in o.items() if k not in ("info", "rc")}
    if kind == "plain":
        host.update(d=ref["d"], p=ref["p"])
    host["info"] = o["info"].cpu().numpy()
    got, want = logical(host, n, m, N, bt, bool(pm)), logical(ref, n, m, N, bt, bool(pm))
    pk = (lambda a: a) if pm else (lambda a: a[:, None])
    e = dict(K=relerr_per_knot(got["K"], want["K"]), P=relerr_per_knot(pk(got["P"]), pk(want["P"])))
    if kind != "plain":
        e.update(d=relerr_traj(got["d"], want["d"]), p=relerr_traj(got["p"], want["p"]))
    for k in ("X", "U"):
        e[k] = float(np.abs(got[k] - want[k]).max() / max(1.0, np.abs(want[k]).max()))
    if kind == "value":
        ve = value_errors({k: host[k] for k in ("s", "dV", "J")}, ref)
        e.update({k: float(v.max()) for k, v in ve.items()})
    print(f"PARITY dp {family(shape)} {what} worst {max(e.values()):.2e} :", " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert (ref["info"] == 0).all()
    for k, v in e.items():
        assert v <= tol, (k, v, what)


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_dp_solve_touches_only_its_buffers(lqrx, gpu_ok, monkeypatch, case):
    shape, kind, layout, pm, tv, prec, mode = case
    if mode:
        monkeypatch.setenv("LQRX_DP_SMALL", mode)
    n, m, N, bt = shape
    npdt = np.float64 if prec == "f64" else np.float32
    d = problem(shape, tv)
    value = kind == "value"
    sizes = out_sizes(shape, kind, pm)

    t = upload(d, shape, kind, layout, npdt)
    plain = lqrx.dp_solve_device(t, N, p_mode=pm, layout=layout, value=value, out=plain_outputs(t, sizes))
    assert plain["rc"] == 0

    hs = []
    tg = guard_all(t, "in", bt, hs)
    og = guard_all(plain_outputs(t, sizes), "out", bt, hs)
    assert sorted(h.name for h in hs) == sorted(list(sizes) + [k for k in t if hasattr(t[k], "shape")])
    got = lqrx.dp_solve_device(tg, N, p_mode=pm, layout=layout, value=value, out=og)
    assert got["rc"] == 0
    guard_check(hs)
    for k in sizes:
        assert got[k].data_ptr() == og[k].data_ptr() and plain[k].numel() == sizes[k]
        assert same_bits(got[k], plain[k]), (k, _id(case))
    assert (plain["info"] == 0).all().item()
    parity({k: plain[k] for k in sizes}, truth(shape, tv, kind, pm), shape, kind, pm, layout,
           TOL64 if prec == "f64" else TOL32, _id(case))


@pytest.mark.parametrize("shape", [(4, 4, 4, 67), (17, 5, 3, 3), (65, 33, 3, 2)], ids=lambda s: "x".join(map(str, s)))
def test_dp_value_null_dV_and_J_touch_nothing_else(lqrx, gpu_ok, shape):
    """val->dV = val->J = NULL: s and every other output are the bits of the full call, every guard
    is intact (s is guarded; a store of dV or J through a stale pointer has nowhere to hide)."""
    n, m, N, bt = shape
    d = problem(shape, 0)
    sizes = out_sizes(shape, "value", 0)
    t = upload(d, shape, "value", 0, np.float64)
    plain = lqrx.dp_solve_device(t, N, value=True, out=plain_outputs(t, sizes))
    hs = []
    tg = guard_all(t, "in", bt, hs)
    part = {k: v for k, v in sizes.items() if k not in ("dV", "J")}
    og = guard_all(plain_outputs(t, part), "out", bt, hs)
    og.update(dV=None, J=None)
    got = lqrx.dp_solve_device(tg, N, value=True, out=og)
    assert got["rc"] == 0 and got["dV"] is None and got["J"] is None
    guard_check(hs)
    for k in part:
        assert same_bits(got[k], plain[k]), k
    assert (plain["info"] == 0).all().item()
    parity({k: plain[k] for k in sizes}, truth(shape, 0, "value", 0), shape, "value", 0, 0, TOL64,
           "null-dV-J " + "x".join(map(str, shape)))


@pytest.mark.parametrize("with_P_", [True, False], ids=["P_", "gain-only"])
@pytest.mark.parametrize("n,m", [(3, 1), (12, 5), (32, 16), (80, 40)])
def test_dp_compute_ctg_touches_only_its_buffers(lqrx, gpu_ok, n, m, with_P_):
    """lqrx_dp_compute_ctg, batch 3, from a random SPD P: K (and P_, or P_ = NULL) against the
    formulas in fp64 numpy, as tests/test_dp_gpu.py::test_per_knot_compute_gain_ctg does
    (K = (R + BᵀPB)⁻¹BᵀPA, P_ = Q + AᵀPA − AᵀPB·K, 1e-10 of max(1, the largest entry))."""
    import torch
    from lqrx import _lib
    from lqrx.dp import abi_to_batch, from_abi, to_abi

    bt = 3
    raw = lqrx.random_batch(n, m, 3, bt, seed=5 + n)
    b = abi_to_batch(raw)
    G = np.random.default_rng(n).standard_normal((bt, n, n))
    P = G @ np.swapaxes(G, 1, 2) / n + np.eye(n)
    P = (P + np.swapaxes(P, 1, 2)) / 2
    t = {k: torch.from_numpy(np.ascontiguousarray(raw[k])).to("cuda:0") for k in ("A", "B", "Q", "R")}
    t["P"] = torch.from_numpy(to_abi(P).reshape(-1)).to("cuda:0")
    sizes = dict(K=bt * m * n, info=bt, **(dict(P_=bt * n * n) if with_P_ else {}))
    like_i = torch.empty(1, dtype=torch.int32, device="cuda:0")
    outs = lambda: {k: pattern_filled(like_i if k == "info" else t["A"], sz) for k, sz in sizes.items()}
    desc = _lib.DpDesc(n, m, 2, _lib.F64, bt, 0, 0, 0, 0)
    p = lambda x: C.c_void_p(x.data_ptr())

    def call(i, o):
        rc = lqrx.load().lqrx_dp_compute_ctg(C.byref(desc), p(i["A"]), p(i["B"]), p(i["Q"]), p(i["R"]), p(i["P"]),
                                             p(o["K"]), p(o["P_"]) if with_P_ else None, p(o["info"]), None)
        assert rc == 0, lqrx.load().lqrx_last_error().decode()
        torch.cuda.synchronize()

    plain = outs()
    call(t, plain)
    hs = []
    tg = guard_all(t, "in", bt, hs)
    og = guard_all(outs(), "out", bt, hs)
    call(tg, og)
    guard_check(hs)
    for k in sizes:
        assert same_bits(og[k], plain[k]), k
    assert (plain["info"] == 0).all().item()
    PB, PA = P @ b.B, P @ b.A
    E = b.R + np.swapaxes(b.B, 1, 2) @ PB
    K = np.linalg.solve(E, np.swapaxes(b.B, 1, 2) @ PA)
    eK = np.abs(from_abi(plain["K"].cpu().numpy(), (bt, m, n)) - K).max() / max(1.0, np.abs(K).max())
    eP = 0.0
    if with_P_:
        Pn = b.Q + np.swapaxes(b.A, 1, 2) @ PA - np.swapaxes(b.A, 1, 2) @ PB @ K
        eP = np.abs(from_abi(plain["P_"].cpu().numpy(), (bt, n, n)) - Pn).max() / max(1.0, np.abs(Pn).max())
    print(f"PARITY dp ctg {n}x{m} worst {max(eK, eP):.2e} : K {eK:.2e} P_ {eP:.2e}")
    assert eK <= 1e-10 and eP <= 1e-10


# ---------------------------------------------------------------------------------------------
# Host outputs: the D2H extents of the `_host` entries' buffer table
HOST_SHAPES = [(3, 2, 5, 5), (6, 3, 5, 3)]      # lane kernel (native layout 1); MFMA kernel (staged)
HOST_CASES = [(k, lay, sh, 0) for k in KINDS for lay in (0, 1) for sh in HOST_SHAPES] + \
             [("value", lay, sh, 1) for lay in (0, 1) for sh in HOST_SHAPES]


@pytest.mark.parametrize("kind,layout,shape,pm", HOST_CASES,
                         ids=[f"{k}-l{lay}-n{sh[0]}-p{pm}" for k, lay, sh, pm in HOST_CASES])
def test_dp_host_entries_write_exactly_their_outputs(lqrx, gpu_ok, kind, layout, shape, pm):
    """Each `_host` entry on numpy buffers from guarded(): guards of every input and output intact,
    every output element written, and the values those of lqrx.solve_batch bit for bit (which hands
    the same bytes to the same entry on plain np.zeros buffers)."""
    from lqrx import _lib
    from lqrx.dp import from_soa, to_soa

    n, m, N, bt = shape
    d = problem(shape, 0)
    value = kind == "value"
    b = to_batch(d, N)
    for k in OPTIONAL:
        if k not in KINDS[kind]:
            setattr(b, k, None)
    want = lqrx.solve_batch(b, all_P=bool(pm), layout=layout, value=value)
    assert want["rc"] == 0 and (want["info"] == 0).all()

    lay = (lambda a: to_soa(a, bt)) if layout == 1 else (lambda a: a)
    ins = {k: np.ascontiguousarray(lay(np.ascontiguousarray(d[k], np.float64))).reshape(-1)
           for k in ("A", "B", "Q", "R", "Qf", "x0") + KINDS[kind]}
    sizes = out_sizes(shape, kind, pm)
    hs = []
    ig = guard_all(ins, "in", bt, hs)
    og = guard_all({k: np.empty(sz, np.int32 if k == "info" else np.float64) for k, sz in sizes.items()}, "out", bt, hs)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    args = {k: ptr(a) for k, a in {**ig, **og}.items()}
    if kind != "plain":
        ln = _lib.DpLinear(*[args[k].value for k in ("q", "r", "qf", "d", "p")])
        args["lin"] = C.byref(ln)
    if value:
        vl = _lib.DpValue(*[args[k].value for k in ("s", "dV", "J")])
        args["val"] = C.byref(vl)
    entry = "lqrx_dp_solve" + ("" if kind == "plain" else "_" + kind) + "_host"
    desc = _lib.DpDesc(n, m, N, _lib.F64, bt, layout, pm, 0, 0)
    rc = _lib.dp_call(entry, desc, args)
    assert rc == 0, lqrx.load().lqrx_last_error().decode()
    guard_check(hs)

    unlay = (lambda a: from_soa(a, bt)) if layout == 1 else (lambda a: a)
    host = {k: (og[k] if k == "info" else unlay(og[k])) for k in sizes}
    if kind == "plain":
        z = truth(shape, 0, "plain", pm)
        host.update(d=z["d"], p=z["p"])
    got = logical(host, n, m, N, bt, bool(pm))
    if value:
        got.update(s=host["s"].reshape(bt, N) if pm else host["s"], dV=host["dV"], J=host["J"])
    for k in (x for x in want if x != "rc"):
        assert np.array_equal(np.asarray(got[k]).reshape(want[k].shape), want[k]), (k, kind, layout, shape, pm)
