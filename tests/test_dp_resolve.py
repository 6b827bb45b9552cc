"""CPU tests of the re-solve (lqrx_dp_factor / lqrx_dp_resolve, include/lqrx.h): the numpy checker
tests/dp_resolve_truth.py against the full solve's checker, and everything the entries decide
before they touch a device (the library loads without one).

The checker is compared with dp_truth.dp_solve_abi_np(kind="cross", all_P=True) on cross_problem, one
full solve per right-hand side, to 1e-12 in float64: d and p with relerr_traj, X and U as
max|a − b| / max(1, max|b|), E⁻¹ per knot against the float64 inverse.  Every figure is printed before
it is asserted.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from dp_adjoint_truth import dense_adjoint_truth, per_knot_problem
from dp_resolve_truth import SHAPES, factor_np, random_rhs, resolve_np, xu_error
from dp_truth import cross_problem, dp_solve_abi_np, relerr_per_knot, relerr_traj

TOL = 1e-12
IDS = ["x".join(map(str, s)) for s in SHAPES]
S_CPU = 3


@functools.lru_cache(maxsize=None)
def solved(lqrx, shape):
    n, m, N, bt, tv = shape
    d = cross_problem(lqrx, n, m, N, bt, 3, tv_QR=tv, tv_AB=tv)
    ref = dp_solve_abi_np(d, N, "cross", all_P=True)
    fac = factor_np(d, N, ref["P"])
    return d, ref, fac


def errors(got, ref_d, ref_p, ref_X, ref_U):
    bt = ref_d.shape[0]
    flat = lambda a: np.asarray(a, np.float64).reshape(bt, -1)
    return dict(d=relerr_traj(flat(got["d"]), flat(ref_d)), p=relerr_traj(flat(got["p"]), flat(ref_p)),
                X=xu_error(got["X"], ref_X), U=xu_error(got["U"], ref_U))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_checker_against_the_full_solve(lqrx, shape):
    """S_CPU right-hand sides per problem: each one's d, p_k, X, U are those of a full cross solve of
    the problem with that q, r, qf, x0; info = 0 and E·E⁻¹ = I."""
    n, m, N, bt, tv = shape
    d, ref, fac = solved(lqrx, shape)
    assert (fac["info"] == 0).all() and (ref["info"] == 0).all()
    rhs = random_rhs(n, m, N, bt, S_CPU, seed=21, tv_QR=tv)
    got = resolve_np(d, N, ref["K"], fac["Einv"], fac["Pc"], S_CPU, tv_QR=int(tv), **rhs)
    kq = N - 1 if tv else 1
    worst = dict(d=0.0, p=0.0, X=0.0, U=0.0)
    for j in range(S_CPU):
        dj = dict(d)
        pick = lambda a, per: np.asarray(a).reshape(bt, S_CPU, per)[:, j].ravel()
        dj.update(q=pick(rhs["q"], kq * n), r=pick(rhs["r"], kq * m), qf=pick(rhs["qf"], n), x0=pick(rhs["x0"], n))
        full = dp_solve_abi_np(dj, N, "cross", all_P=True)
        e = errors({k: got[k][:, j] for k in got}, full["d"].reshape(bt, -1), full["p"].reshape(bt, -1),
                   full["X"].reshape(bt, N, n), full["U"].reshape(bt, N - 1, m))
        worst = {k: max(worst[k], e[k]) for k in e}
    print(f"CHECKER resolve {shape}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (k, v)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_checker_reproduces_the_solve(lqrx, shape):
    """S = 1 and the problem's own q, r, qf, x0: the solve's d, p, X, U."""
    n, m, N, bt, tv = shape
    d, ref, fac = solved(lqrx, shape)
    got = resolve_np(d, N, ref["K"], fac["Einv"], fac["Pc"], 1, q=d["q"], r=d["r"], qf=d["qf"], x0=d["x0"],
                     tv_QR=int(tv))
    e = errors({k: got[k][:, 0] for k in got}, ref["d"].reshape(bt, -1), ref["p"].reshape(bt, -1),
               ref["X"].reshape(bt, N, n), ref["U"].reshape(bt, N - 1, m))
    print(f"CHECKER resolve own rhs {shape}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v <= TOL, (k, v)


def test_checker_is_the_adjoint_solve(lqrx):
    """c = NULL, x0 = 0, q = gX, qf = gX_N, r = gU: X' and U' of the adjoint — the gradients with
    respect to q, qf and r of ℓ = Σ gX·X + Σ gU·U by autograd through the dense KKT solve."""
    shape = (6, 3, 9, 2, True)
    n, m, N, bt, tv = shape
    d = cross_problem(lqrx, n, m, N, bt, 5, tv_QR=tv, tv_AB=tv)
    ref = dp_solve_abi_np(d, N, "cross", all_P=True)
    d0 = dict(d, c=None)
    fac = factor_np(d0, N, ref["P"])
    assert fac["Pc"] is None
    rng = np.random.default_rng(31)
    gX, gU = rng.standard_normal((bt, N, n)), rng.standard_normal((bt, N - 1, m))
    got = resolve_np(d0, N, ref["K"], fac["Einv"], None, 1, q=gX[:, :N - 1].ravel(), r=gU.ravel(),
                     qf=gX[:, N - 1].ravel(), x0=None, tv_QR=1)
    for b in range(bt):
        t = dense_adjoint_truth(per_knot_problem(d, N, b), N, gX[b], gU[b])
        want_X = np.concatenate([t["g"]["q"], t["g"]["qf"][None]], axis=0)
        eX, eU = xu_error(got["X"][b, 0], want_X), xu_error(got["U"][b, 0], t["g"]["r"])
        print(f"CHECKER resolve adjoint problem {b}: X' {eX:.2e} U' {eU:.2e}")
        assert eX <= 1e-10 and eU <= 1e-10


def test_checker_inverse(lqrx):
    d, ref, fac = solved(lqrx, (24, 18, 10, 3, False))
    n, m, N, bt = 24, 18, 10, 3
    from dp_truth import _mats

    Ei = _mats(fac["Einv"], bt, N - 1, m, m, np.float64)
    B = _mats(d["B"], bt, 1, n, m, np.float64)[:, 0]
    R = _mats(d["R"], bt, 1, m, m, np.float64)[:, 0]
    P = _mats(ref["P"], bt, N, n, n, np.float64)
    E = R[:, None] + np.swapaxes(B, -1, -2)[:, None] @ P[:, 1:] @ B[:, None]
    e = relerr_per_knot(E @ Ei, np.broadcast_to(np.eye(m), E.shape).copy())
    print(f"CHECKER factor E·Einv − I: {e:.2e}")
    assert e <= TOL


# ---- argument codes: decided before the device is touched ----
def _desc(**kw):
    from lqrx import _lib

    return _lib.DpDesc(**{**dict(n=8, m=4, N=10, dtype=_lib.F64, batch=4, layout=0, p_mode=1,
                                 knot_stride_AB=0, knot_stride_QR=0), **kw})


def _factor(lqrx, host, desc, B, R, c, P, Einv, Pc, info):
    lib = lqrx.load()
    vp = lambda x: None if x is None else C.c_void_p(x)
    args = [C.byref(desc) if desc is not None else None] + [vp(x) for x in (B, R, c, P, Einv, Pc, info)]
    rc = lib.lqrx_dp_factor_host(*args) if host else lib.lqrx_dp_factor(*args, None)
    return rc, lib.lqrx_last_error().decode()


def _resolve(lqrx, host, desc, A, B, c, fac, rhs):
    lib = lqrx.load()
    vp = lambda x: None if x is None else C.c_void_p(x)
    args = [C.byref(desc) if desc is not None else None, vp(A), vp(B), vp(c),
            C.byref(fac) if fac is not None else None, C.byref(rhs) if rhs is not None else None]
    rc = lib.lqrx_dp_resolve_host(*args) if host else lib.lqrx_dp_resolve(*args, None)
    return rc, lib.lqrx_last_error().decode()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_factor_argument_codes(lqrx, host):
    from lqrx import _lib

    p = np.zeros(4096).ctypes.data
    call = lambda **kw: _factor(lqrx, host, **{**dict(desc=_desc(), B=p, R=p, c=p, P=p, Einv=p, Pc=p, info=p), **kw})
    for name, code in (("B", -2), ("R", -3), ("P", -5), ("Einv", -6), ("Pc", -7)):
        rc, msg = call(**{name: None})
        assert rc == code and name in msg, (name, rc, msg)
    rc, msg = call(c=None)                                       # Pc without c
    assert rc == -7 and "Pc" in msg, (rc, msg)
    assert call(desc=None)[0] == -1
    assert call(desc=_desc(n=0))[0] == -1
    assert call(desc=_desc(N=1))[0] == -1
    assert call(desc=_desc(dtype=7))[0] == -1
    assert call(desc=_desc(p_mode=2))[0] == -1
    for bad in (dict(p_mode=0), dict(layout=1), dict(n=65), dict(m=33)):
        assert call(desc=_desc(**bad))[0] == _lib.ERR_UNSUPPORTED, bad
    assert call(desc=_desc(n=64, m=32), B=None)[0] == -2        # the largest supported shape passes the descriptor
    assert call(desc=_desc(batch=0), B=None, R=None, c=None, P=None, Einv=None, Pc=None, info=None)[0] == 0


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_resolve_argument_codes(lqrx, host):
    from lqrx import _lib

    p = np.zeros(4096).ctypes.data
    fac = lambda **kw: _lib.DpFactors(**{**dict(K=p, Einv=p, Pc=p), **kw})
    rhs = lambda **kw: _lib.DpRhs(**{**dict(S=5, q=p, r=p, qf=p, x0=p, d=p, p=p, X=p, U=p), **kw})
    call = lambda **kw: _resolve(lqrx, host, **{**dict(desc=_desc(), A=p, B=p, c=p, fac=fac(), rhs=rhs()), **kw})
    for name, code in (("A", -2), ("B", -3), ("fac", -5), ("rhs", -6)):
        rc, msg = call(**{name: None})
        assert rc == code and name in msg, (name, rc, msg)
    for member in ("K", "Einv", "Pc"):
        rc, msg = call(fac=fac(**{member: None}))
        assert rc == -5 and "fac->" + member in msg, (member, rc, msg)
    rc, msg = call(c=None)                                       # Pc without c
    assert rc == -5 and "fac->Pc" in msg, (rc, msg)
    for kw, text in ((dict(S=0), "rhs->S"), (dict(S=-2), "rhs->S"), (dict(d=None, p=None, X=None, U=None), "rhs->d"),
                     (dict(d=None), "rhs->X"), (dict(d=None, X=None), "rhs->U")):
        rc, msg = call(rhs=rhs(**kw))
        assert rc == -6 and text in msg, (kw, rc, msg)
    # q, r, qf, x0 are optional, and so is every output but one: what answers is the next check
    assert call(rhs=rhs(q=None, r=None, qf=None, x0=None, X=None, U=None, p=None), A=None)[0] == -2
    assert call(desc=None)[0] == -1
    assert call(desc=_desc(n=0))[0] == -1
    assert call(desc=_desc(p_mode=2))[0] == -1
    assert call(desc=_desc(p_mode=0), A=None)[0] == -2          # both p modes are served
    for bad in (dict(layout=1), dict(n=65), dict(m=33)):
        assert call(desc=_desc(**bad))[0] == _lib.ERR_UNSUPPORTED, bad
    assert call(desc=_desc(batch=0), A=None, B=None, c=None, fac=None, rhs=None)[0] == 0


def test_wrappers_raise(lqrx):
    from dp_truth import to_batch
    from lqrx.dp import from_abi

    n, m, N, bt = 6, 3, 8, 2
    d = cross_problem(lqrx, n, m, N, bt, 3)
    b = to_batch(d, N)
    P = np.zeros((bt, N, n, n))
    K = np.zeros((bt, N - 1, m, n))
    fac = dict(Einv=np.zeros((bt, N - 1, m, m)), Pc=np.zeros((bt, N - 1, n)))
    x0 = np.zeros((bt, 4, n))
    with pytest.raises(ValueError, match="P is"):
        lqrx.factor_batch(b, P[:, 0])
    with pytest.raises(ValueError, match="outputs"):
        lqrx.resolve_batch(b, K, fac, x0=x0, outputs=())
    with pytest.raises(ValueError, match="outputs"):
        lqrx.resolve_batch(b, K, fac, x0=x0, outputs=("J",))
    with pytest.raises(ValueError, match="need d"):
        lqrx.resolve_batch(b, K, fac, x0=x0, outputs=("X",))
    with pytest.raises(ValueError, match="sets S"):
        lqrx.resolve_batch(b, K, fac)
    with pytest.raises(ValueError, match="qf is"):
        lqrx.resolve_batch(b, K, fac, x0=x0, qf=np.zeros((bt, 3, n)))
    with pytest.raises(ValueError, match="both or neither"):
        lqrx.resolve_batch(b, K, fac, x0=x0, q=np.zeros((bt, 4, N - 1, n)), r=np.zeros((bt, 4, m)))
    with pytest.raises(ValueError, match="r is"):
        lqrx.resolve_batch(b, K, fac, x0=x0, r=np.zeros((bt, 4, m + 1)))
    with pytest.raises(ValueError, match="K has"):
        lqrx.resolve_batch(b, K[:, 1:], fac, x0=x0)
    with pytest.raises(ValueError, match="Pc"):
        lqrx.resolve_batch(b, K, dict(Einv=fac["Einv"], Pc=None), x0=x0)
    with pytest.raises(ValueError, match="Einv"):
        lqrx.resolve_batch(b, K, dict(Pc=fac["Pc"]), x0=x0)
    with pytest.raises(ValueError, match="outputs"):
        lqrx.dp_resolve_device(dict(n=n, m=m, batch=bt, A=np.zeros(1)), N, {}, dict(S=1, outputs=("U",)))


def test_resolve_symbols_and_mirrors(lqrx):
    """The entries are additive to ABI 5 (detect by symbol) and stay out of the solve-entry table."""
    from lqrx import _lib

    lib = lqrx.load()
    assert lib.lqrx_abi_version() == 5
    for sym in ("lqrx_dp_factor", "lqrx_dp_factor_host", "lqrx_dp_resolve", "lqrx_dp_resolve_host"):
        assert hasattr(lib, sym), sym
    assert not any("resolve" in k or "factor" in k for k in _lib.DP_ENTRY_ARGS)
    assert len(_lib.DP_ENTRY_ARGS) == 12                       # five kinds, device and _host, two _host_devices
    assert C.sizeof(_lib.DpFactors) == 3 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.DpRhs) == 8 + 8 * C.sizeof(C.c_void_p)
    for f in ("factor_batch", "resolve_batch", "dp_factor_device", "dp_resolve_device"):
        assert callable(getattr(lqrx, f)), f
