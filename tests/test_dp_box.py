"""CPU tests of the input-bounds entry (lqrx_dp_resolve_box, include/lqrx.h): the numpy checker
tests/dp_box_truth.py against the re-solve's checker and against an independent truth (the QP condensed
over U, solved by scipy's BVLS), the checker's own properties, and everything the entries and the Python
layer decide before they touch a device (the library loads without one).  Every figure is printed before
it is asserted.

Measured here (float64 numpy, ρ = 1, relax 1.6, eps 1e-10, two random instances per plant): 4.2 %, 6.2 % and
14.5 % of the truth's entries active on (4, 1, 40), (6, 3, 30) and (17, 5, 12), the stop after 50 – 1046
iterations, |Z − U_truth|∞ 2.3e-10 – 3.6e-10 absolute on controls of size 4 – 57 (limit 1e-8 · that size),
2.4 – 4.0 × the larger residual at the stop; without bounds and from the unconstrained U one iteration and U 2.4e-14 from
the cross solve; the slow plant at ρ = 10 stops after 1580 iterations 6.5e-10 from the truth; natural residual
3e-8 – 3e-5 at the checker's Z against 20 – 7500 at the clipped unconstrained control.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from dp_box_truth import (SLOW_PLANT, TRUTH_SHAPES, active_share, box_np, bvls_truth, factors_np, half_peak_bounds,
                          natural_residual, own_rhs)
from dp_resolve_truth import random_rhs, xu_error
from dp_truth import cross_problem, dp_solve_abi_np

IDS = ["x".join(map(str, s)) for s in TRUTH_SHAPES]
RHO, RELAX = 1.0, 1.6
S_CPU = 2


@functools.lru_cache(maxsize=None)
def problem(lqrx, shape):
    """cross_problem (M ≠ 0, c ≠ 0), its factors with R + ρI, and the unconstrained U of its own right-hand side"""
    n, m, N, bt, tv = shape
    d = cross_problem(lqrx, n, m, N, bt, 3, tv_QR=tv, tv_AB=tv)
    return d, factors_np(d, N, RHO), dp_solve_abi_np(d, N, "cross")


@functools.lru_cache(maxsize=None)
def bounded(lqrx, shape):
    """S_CPU random instances per problem, bounds at half their unconstrained peak with one side of one input
    left open, the BVLS truth and the checker's run"""
    n, m, N, bt, tv = shape
    d, fac, unc = problem(lqrx, shape)
    rhs = random_rhs(n, m, N, bt, S_CPU, seed=5, tv_QR=tv)
    U_unc = bvls_truth(d, N, S_CPU, None, None, tv_QR=int(tv), **rhs)
    lo, hi = half_peak_bounds(U_unc, bt, m)
    truth = bvls_truth(d, N, S_CPU, lo, hi, tv_QR=int(tv), **rhs)
    got = box_np(d, N, fac["K"], fac["Einv"], fac["Pc"], S_CPU, tv_QR=int(tv), u_lo=lo, u_hi=hi, rho=RHO, relax=RELAX,
                 eps_prim=1e-10, eps_dual=1e-10, max_iter=2000, **rhs)
    return d, fac, rhs, lo, hi, U_unc, truth, got


@pytest.mark.parametrize("shape", TRUTH_SHAPES, ids=IDS)
def test_checker_without_bounds_is_the_unconstrained_solve(lqrx, shape):
    """u_lo = u_hi = None and Z = the unconstrained U: one iteration, and U is the cross solve's."""
    n, m, N, bt, tv = shape
    d, fac, unc = problem(lqrx, shape)
    got = box_np(d, N, fac["K"], fac["Einv"], fac["Pc"], 1, tv_QR=int(tv), rho=RHO, relax=RELAX, eps_prim=1e-9,
                 eps_dual=1e-9, max_iter=50, Z=unc["U"], **own_rhs(d, N))
    eU, eX, eZ = xu_error(got["U"], unc["U"]), xu_error(got["X"], unc["X"]), xu_error(got["Z"], unc["U"])
    print(f"CHECKER box no bounds {shape}: iters {got['iters'].ravel().tolist()} U {eU:.2e} X {eX:.2e} Z {eZ:.2e} "
          f"res {got['res'].max():.2e}")
    assert (got["iters"] == 1).all()
    assert eU <= 1e-12 and eX <= 1e-12 and eZ <= 1e-12


@pytest.mark.parametrize("shape", TRUTH_SHAPES, ids=IDS)
def test_checker_against_bvls(lqrx, shape):
    n, m, N, bt, tv = shape
    d, fac, rhs, lo, hi, U_unc, truth, got = bounded(lqrx, shape)
    share = active_share(truth, lo, hi, bt, m)
    scale = max(1.0, np.abs(truth).max())
    dist = np.abs(got["Z"] - truth).max(axis=(2, 3))
    ratio = (dist / np.maximum(got["res"].max(axis=2), 1e-300)).max()
    print(f"TRUTH box {shape}: active {100 * share:.1f} % iters {got['iters'].min()} .. {got['iters'].max()} "
          f"|Z - truth| {dist.max():.2e} (scale {scale:.2e}) worst distance / residual {ratio:.2f}")
    assert 0.02 <= share <= 0.60, share                       # otherwise the test tests nothing
    assert (got["iters"] < 2000).all()
    assert (got["res"] <= 1e-10).all()
    assert ((got["Z"] >= lo[:, None, None]) & (got["Z"] <= hi[:, None, None])).all()
    assert dist.max() <= 1e-8 * scale


def test_checker_against_bvls_on_the_slow_plant(lqrx):
    """The plant that ρ = 1 does not finish in 3000 iterations (dp_box_truth.TRUTH_SHAPES), with its own right-hand
    side at ρ = 10: every plant of the batch stops and meets the same truth."""
    shape, rho = SLOW_PLANT
    n, m, N, bt, tv = shape
    d = cross_problem(lqrx, n, m, N, bt, 3, tv_QR=tv, tv_AB=tv)
    fac = factors_np(d, N, rho)
    lo, hi = half_peak_bounds(dp_solve_abi_np(d, N, "cross")["U"], bt, m)
    truth = bvls_truth(d, N, 1, lo, hi, tv_QR=int(tv), **own_rhs(d, N))
    got = box_np(d, N, fac["K"], fac["Einv"], fac["Pc"], 1, tv_QR=int(tv), u_lo=lo, u_hi=hi, rho=rho, relax=RELAX,
                 eps_prim=1e-10, eps_dual=1e-10, max_iter=2000, **own_rhs(d, N))
    dist = np.abs(got["Z"] - truth).max(axis=(1, 2, 3))
    print(f"TRUTH box slow plant rho {rho}: iters {got['iters'].ravel().tolist()} |Z - truth| {dist.max():.2e} "
          f"active {100 * active_share(truth, lo, hi, bt, m):.1f} %")
    assert (got["iters"] < 2000).all() and got["iters"][5, 0] == got["iters"].max()
    assert dist.max() <= 1e-8 * max(1.0, np.abs(truth).max())


@pytest.mark.parametrize("shape", TRUTH_SHAPES, ids=IDS)
def test_natural_residual_and_multiplier_signs(lqrx, shape):
    """The reference-free measure the GPU tests use: small at the checker's Z, zero-ish at the truth, large at the
    clipped unconstrained optimum; Y = ρW is ≥ 0 at the upper bound, ≤ 0 at the lower one, 0 inside."""
    n, m, N, bt, tv = shape
    d, fac, rhs, lo, hi, U_unc, truth, got = bounded(lqrx, shape)
    nat, g = natural_residual(d, N, S_CPU, got["Z"], lo, hi, tv_QR=int(tv), **rhs)
    nat_truth, _ = natural_residual(d, N, S_CPU, truth, lo, hi, tv_QR=int(tv), **rhs)
    nat_clip, _ = natural_residual(d, N, S_CPU, np.clip(U_unc, lo[:, None, None], hi[:, None, None]), lo, hi,
                                   tv_QR=int(tv), **rhs)
    Y = RHO * got["W"]
    upper, lower = got["Z"] == hi[:, None, None], got["Z"] == lo[:, None, None]
    inside = ~upper & ~lower
    print(f"NATURAL box {shape}: checker {nat.max():.2e} truth {nat_truth.max():.2e} clipped {nat_clip.max():.2e} "
          f"|Y + g| {np.abs(Y + g).max():.2e} |Y| inside {np.abs(Y[inside]).max():.2e}")
    # g = HU + g₀ carries the conditioning of the condensed Hessian (its own rounding at the truth is 2e-8 on
    # (4, 1, 40)), so the measure is held against that of the clipped control, the scale of the gradient: six
    # orders below it, where a clipped control is no optimum at all
    assert nat.max() <= 1e-6 * nat_clip.max() and nat_truth.max() <= 1e-6 * nat_clip.max()
    assert (Y[upper] >= -1e-9).all() and (Y[lower] <= 1e-9).all() and np.abs(Y[inside]).max() <= 1e-9
    assert upper.any() and np.abs(Y + g).max() <= 1e-6 * nat_clip.max()   # y = −g: the multiplier of the bounds


def test_checker_continuation_and_relaxation(lqrx):
    """7 then 23 iterations on the returned Z, W are 30 (eps = 0: no early stop, bit for bit); relax = 1 and 1.6
    stop at the same Z."""
    shape = (6, 3, 30, 5, False)
    n, m, N, bt, tv = shape
    d, fac, rhs, lo, hi, U_unc, truth, got = bounded(lqrx, shape)
    run = lambda **kw: box_np(d, N, fac["K"], fac["Einv"], fac["Pc"], S_CPU, tv_QR=int(tv), u_lo=lo, u_hi=hi, rho=RHO,
                              **{**dict(relax=RELAX, eps_prim=0.0, eps_dual=0.0), **kw}, **rhs)
    a = run(max_iter=7)
    ab = run(max_iter=23, Z=a["Z"], W=a["W"])
    full = run(max_iter=30)
    assert (a["iters"] == 7).all() and (ab["iters"] == 23).all() and (full["iters"] == 30).all()
    for k in ("Z", "W", "d", "X", "U", "res"):
        assert np.array_equal(ab[k], full[k]), k
    plain = run(relax=1.0, eps_prim=1e-10, eps_dual=1e-10, max_iter=4000)
    e = np.abs(plain["Z"] - got["Z"]).max() / max(1.0, np.abs(got["Z"]).max())
    print(f"CHECKER box relax 1 against 1.6: iters {plain['iters'].max()} against {got['iters'].max()}, |dZ| {e:.2e}")
    assert (plain["iters"] < 4000).all() and e <= 2e-8       # each within 1e-8 of the truth


def test_checker_nan_never_converges(lqrx):
    shape = (6, 3, 30, 5, False)
    n, m, N, bt, tv = shape
    d, fac, rhs, lo, hi, U_unc, truth, got = bounded(lqrx, shape)
    x0 = np.array(rhs["x0"], np.float64).reshape(bt, S_CPU, n).copy()
    x0[2, 1, 0] = np.nan
    run = lambda x: box_np(d, N, fac["K"], fac["Einv"], fac["Pc"], S_CPU, tv_QR=int(tv), u_lo=lo, u_hi=hi, rho=RHO,
                           relax=RELAX, eps_prim=1e-3, eps_dual=1e-3, max_iter=400, **dict(rhs, x0=x))
    r, clean = run(x0.ravel()), run(rhs["x0"])
    assert r["iters"][2, 1] == 400 and np.isnan(r["res"][2, 1]).all() and clean["iters"].max() < 400
    others = np.ones((bt, S_CPU), bool)
    others[2, 1] = False
    for k in ("Z", "W", "d", "X", "U", "iters", "res"):       # the other instances stop as they do without it
        assert np.array_equal(r[k][others], clean[k][others]), k


# ---- argument codes: decided before the device is touched ----
def _desc(**kw):
    from lqrx import _lib

    return _lib.DpDesc(**{**dict(n=8, m=4, N=10, dtype=_lib.F64, batch=4, layout=0, p_mode=0,
                                 knot_stride_AB=0, knot_stride_QR=0), **kw})


def _box_call(lqrx, host, desc, A, B, c, fac, rhs, box):
    lib = lqrx.load()
    vp = lambda x: None if x is None else C.c_void_p(x)
    args = [C.byref(desc) if desc is not None else None, vp(A), vp(B), vp(c),
            C.byref(fac) if fac is not None else None, C.byref(rhs) if rhs is not None else None,
            C.byref(box) if box is not None else None]
    rc = lib.lqrx_dp_resolve_box_host(*args) if host else lib.lqrx_dp_resolve_box(*args, None)
    return rc, lib.lqrx_last_error().decode()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_box_argument_codes(lqrx, host):
    from lqrx import _lib

    p = np.zeros(4096).ctypes.data
    fac = lambda **kw: _lib.DpFactors(**{**dict(K=p, Einv=p, Pc=p), **kw})
    rhs = lambda **kw: _lib.DpRhs(**{**dict(S=5, q=p, r=p, qf=p, x0=p, d=p, p=None, X=p, U=p), **kw})
    box = lambda **kw: _lib.DpBox(**{**dict(rho=1.0, relax=1.6, eps_prim=1e-6, eps_dual=1e-6, max_iter=100, u_lo=p, u_hi=p,
                                            Z=p, W=p, iters=p, res=p), **kw})
    call = lambda **kw: _box_call(lqrx, host, **{**dict(desc=_desc(), A=p, B=p, c=p, fac=fac(), rhs=rhs(), box=box()), **kw})
    for name, code in (("A", -2), ("B", -3), ("fac", -5), ("rhs", -6), ("box", -7)):
        rc, msg = call(**{name: None})
        assert rc == code and name in msg, (name, rc, msg)
    for member in ("K", "Einv", "Pc"):
        rc, msg = call(fac=fac(**{member: None}))
        assert rc == -5 and "fac->" + member in msg, (member, rc, msg)
    rc, msg = call(c=None)                                       # Pc without c
    assert rc == -5 and "fac->Pc" in msg, (rc, msg)
    for kw, text in ((dict(S=0), "rhs->S"), (dict(S=-2), "rhs->S"), (dict(d=None), "rhs->d"), (dict(p=p), "rhs->p")):
        rc, msg = call(rhs=rhs(**kw))
        assert rc == -6 and text in msg, (kw, rc, msg)
    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(rho=0.0), "box->rho"), (dict(rho=-1.0), "box->rho"), (dict(rho=nan), "box->rho"),
                     (dict(rho=inf), "box->rho"), (dict(relax=0.99), "box->relax"), (dict(relax=2.0), "box->relax"),
                     (dict(relax=nan), "box->relax"), (dict(eps_prim=-1e-9), "box->eps_prim"),
                     (dict(eps_prim=nan), "box->eps_prim"), (dict(eps_dual=-1.0), "box->eps_dual"),
                     (dict(eps_dual=nan), "box->eps_dual"), (dict(max_iter=0), "box->max_iter"),
                     (dict(max_iter=10001), "box->max_iter"), (dict(Z=None), "box->Z"), (dict(W=None), "box->W")):
        rc, msg = call(box=box(**kw))
        assert rc == -7 and text in msg, (kw, rc, msg)
    # the optional members, the ends of the ranges and eps = 0 pass: what answers is the next check
    ok = box(u_lo=None, u_hi=None, iters=None, res=None, relax=1.0, eps_prim=0.0, eps_dual=0.0, max_iter=10000)
    assert call(box=ok, rhs=rhs(q=None, r=None, qf=None, x0=None, X=None, U=None), A=None)[0] == -2
    assert call(box=box(max_iter=1), A=None)[0] == -2
    assert call(desc=None)[0] == -1
    assert call(desc=_desc(n=0))[0] == -1
    assert call(desc=_desc(p_mode=2))[0] == -1
    for tv in (dict(knot_stride_AB=1), dict(knot_stride_QR=1), dict(dtype=_lib.F32), dict(n=64, m=32), dict(p_mode=1)):
        assert call(desc=_desc(**tv), A=None)[0] == -2, tv       # the whole support of the re-solve
    for bad in (dict(layout=1), dict(n=65), dict(m=33)):
        rc, msg = call(desc=_desc(**bad))
        assert rc == _lib.ERR_UNSUPPORTED and "lqrx_dp_resolve_box" in msg, (bad, rc, msg)
    assert call(desc=_desc(batch=0), A=None, B=None, c=None, fac=None, rhs=None, box=None)[0] == 0


def test_wrappers_raise(lqrx):
    from dp_truth import to_batch

    n, m, N, bt = 6, 3, 8, 2
    d = cross_problem(lqrx, n, m, N, bt, 3)
    b = to_batch(d, N)
    x0 = np.zeros((bt, 4, n))
    with pytest.raises(ValueError, match="u_lo is"):
        lqrx.box_batch(b, np.zeros((bt, m + 1)), None, x0=x0)
    with pytest.raises(ValueError, match="u_hi is"):
        lqrx.box_batch(b, None, np.zeros((bt + 1, m)), x0=x0)
    with pytest.raises(ValueError, match="qf is"):
        lqrx.box_batch(b, None, None, x0=x0, qf=np.zeros((bt, 3, n)))
    with pytest.raises(ValueError, match="both or neither"):
        lqrx.box_batch(b, None, None, x0=x0, q=np.zeros((bt, 4, N - 1, n)), r=np.zeros((bt, 4, m)))
    with pytest.raises(ValueError, match="r is"):
        lqrx.box_batch(b, None, None, x0=x0, r=np.zeros((bt, 4, m + 1)))
    with pytest.raises(ValueError, match="Z is"):
        lqrx.box_batch(b, None, None, x0=x0, Z=np.zeros((bt, 4, N - 1, m + 1)))
    with pytest.raises(ValueError, match="W is"):
        lqrx.box_batch(b, None, None, x0=x0, W=np.zeros((bt, 3, N - 1, m)))
    with pytest.raises(ValueError, match="rho"):
        lqrx.box_batch(b, None, None, x0=x0, rho=0.0)
    with pytest.raises(ValueError, match="eps is the pair"):
        lqrx.box_batch(b, None, None, x0=x0, eps=1e-6)

    class T:   # the little of a tensor that the checks read
        def __init__(self, numel, dtype="f"):
            self._n, self.dtype, self.device = numel, dtype, None

        def numel(self):
            return self._n

    t = dict(n=n, m=m, batch=bt, A=T(1))
    full = bt * 4 * (N - 1) * m
    with pytest.raises(ValueError, match="rhs outputs"):
        lqrx.dp_box_device(t, N, {}, dict(S=4, outputs=("X",)), dict(rho=1.0, Z=T(full), W=T(full)))
    with pytest.raises(ValueError, match="rhs outputs"):
        lqrx.dp_box_device(t, N, {}, dict(S=4, outputs=("d", "p")), dict(rho=1.0, Z=T(full), W=T(full)))
    with pytest.raises(ValueError, match="box outputs"):
        lqrx.dp_box_device(t, N, {}, dict(S=4), dict(rho=1.0, Z=T(full), W=T(full), outputs=("J",)))
    with pytest.raises(ValueError, match="needs rho"):
        lqrx.dp_box_device(t, N, {}, dict(S=4), dict(Z=T(full), W=T(full)))
    with pytest.raises(ValueError, match=r"box\['Z'\]"):
        lqrx.dp_box_device(t, N, {}, dict(S=4), dict(rho=1.0, W=T(full)))
    with pytest.raises(ValueError, match=r"box\['W'\]"):
        lqrx.dp_box_device(t, N, {}, dict(S=4), dict(rho=1.0, Z=T(full), W=T(full - 1)))
    with pytest.raises(ValueError, match=r"box\['u_hi'\]"):
        lqrx.dp_box_device(t, N, {}, dict(S=4), dict(rho=1.0, Z=T(full), W=T(full), u_hi=T(bt * m + 1)))


def test_box_symbols_and_mirrors(lqrx):
    """The entries are additive to ABI 5 (detect by symbol), stay out of the solve-entry table, and the ctypes
    signatures and the DpBox mirror follow the prototypes and the struct of include/lqrx.h."""
    from lqrx import _lib

    lib = lqrx.load()
    assert lib.lqrx_abi_version() == 5
    hdr = open(_lib.HEADER_PATH).read()
    for sym in ("lqrx_dp_resolve_box", "lqrx_dp_resolve_box_host"):
        assert hasattr(lib, sym) and sym in _lib.header_functions(), sym
        proto = re.search(r"\bint\s+" + sym + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        params = [re.sub(r"\s+", " ", x).strip() for x in proto.split(",")]
        want = []
        for x in params:
            kind = re.match(r"const (lqrx_\w+) \*", x)
            want.append({"lqrx_dp_desc": C.POINTER(_lib.DpDesc), "lqrx_dp_factors": C.POINTER(_lib.DpFactors),
                         "lqrx_dp_rhs": C.POINTER(_lib.DpRhs), "lqrx_dp_box": C.POINTER(_lib.DpBox)}[kind.group(1)]
                        if kind else C.c_void_p)
        res, args = _lib._SIGS[sym]
        assert res is C.c_int and args == want, (sym, params)
    assert not any("box" in k for k in _lib.DP_ENTRY_ARGS) and len(_lib.DP_ENTRY_ARGS) == 12
    body = hdr[hdr.index("typedef struct lqrx_dp_box {"):hdr.index("} lqrx_dp_box;")]
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = [nm for decl in body.split("{")[1].split(";") for nm in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.DpBox._fields_], names
    assert C.sizeof(_lib.DpBox) == 4 * 8 + 8 + 6 * C.sizeof(C.c_void_p)
    assert _lib.DpBox.max_iter.offset == 32 and _lib.DpBox.u_lo.offset == 40
    for f in ("box_batch", "dp_box_device"):
        assert callable(getattr(lqrx, f)), f
