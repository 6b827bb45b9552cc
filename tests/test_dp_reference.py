"""oracle.dp_reference — the DP recursion in one precision (float32, float64 or longdouble) with
its own Cholesky — pinned against the checkers the suite already trusts.  No device is needed.

On one benign problem (n = 6, m = 3, N = 12, three trajectories of dp_truth.affine_problem),
time-invariant and with every field per knot:
  1. float64, with q, r, qf, c: K, P, d, p, X, U of dp_truth.dp_solve_abi_np (affine) within 1e-12;
  2. float64, plain: K, P, X, U of oracle.dp_solve_abi (the C oracle) within 1e-12;
  3. longdouble against float64 within 1e-11 — the precisions run the same code;
and dp_extended is the longdouble run, an indefinite E is reported at its knot, float32 stays
float32.  Errors are max|a − b| / max|b| over the whole array.
"""
import numpy as np
import pytest

from dp_truth import affine_problem, dp_solve_abi_np

n, m, N, BT = 6, 3, 12, 3


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _logical(d):
    from lqrx.dp import from_abi

    kab = (N - 1,) if d.get("tv_AB") else ()
    kqr = (N - 1,) if d.get("tv_QR") else ()
    return dict(A=from_abi(d["A"], (BT, *kab, n, n)), B=from_abi(d["B"], (BT, *kab, n, m)),
                Q=from_abi(d["Q"], (BT, *kqr, n, n)), R=from_abi(d["R"], (BT, *kqr, m, m)),
                Qf=from_abi(d["Qf"], (BT, n, n)), x0=d["x0"].reshape(BT, n),
                q=d["q"].reshape(BT, *kqr, n), r=d["r"].reshape(BT, *kqr, m), qf=d["qf"].reshape(BT, n),
                c=d["c"].reshape(BT, *kab, n))


def _run(oracle, L, dtype, lin=True):
    kw = dict(q=L["q"], r=L["r"], qf=L["qf"], c=L["c"]) if lin else {}
    return oracle.dp_reference(L["A"], L["B"], L["Q"], L["R"], L["Qf"], N, x0=L["x0"], dtype=dtype, **kw)


@pytest.mark.parametrize("tv", [False, True])
def test_reference_f64_equals_checkers(lqrx, oracle, tv):
    from lqrx.dp import from_abi

    d = affine_problem(lqrx, n, m, N, BT, 501, tv_QR=tv, tv_AB=tv)
    L = _logical(d)
    got = _run(oracle, L, np.float64)
    ref = dp_solve_abi_np(d, N, "affine", all_P=True)
    assert (got["info"] == 0).all() and (ref["info"] == 0).all()
    want = dict(K=from_abi(ref["K"], (BT, N - 1, m, n)), P=from_abi(ref["P"], (BT, N, n, n)),
                d=ref["d"].reshape(BT, N - 1, m), p=ref["p"].reshape(BT, N, n),
                X=ref["X"].reshape(BT, N, n), U=ref["U"].reshape(BT, N - 1, m))
    for k, w in want.items():
        e = _rel(got[k], w)
        print(f"tv={tv} affine checker {k}: {e:.2e}")
        assert e <= 1e-12, k
    plain = _run(oracle, L, np.float64, lin=False)
    c = oracle.dp_solve_abi(d, N, all_P=True)
    want = dict(K=from_abi(c["K"], (BT, N - 1, m, n)), P=from_abi(c["P"], (BT, N, n, n)),
                X=c["X"].reshape(BT, N, n), U=c["U"].reshape(BT, N - 1, m))
    assert "d" not in plain and "p" not in plain
    for k, w in want.items():
        e = _rel(plain[k], w)
        print(f"tv={tv} C oracle {k}: {e:.2e}")
        assert e <= 1e-12, k
    # K, P do not depend on the linear terms
    assert np.array_equal(plain["K"], got["K"]) and np.array_equal(plain["P"], got["P"])


@pytest.mark.parametrize("tv", [False, True])
def test_reference_longdouble_equals_f64(lqrx, oracle, tv):
    assert np.finfo(np.longdouble).eps < 1e-18, "needs x87 extended precision"
    L = _logical(affine_problem(lqrx, n, m, N, BT, 501, tv_QR=tv, tv_AB=tv))
    a, b = _run(oracle, L, np.longdouble), _run(oracle, L, np.float64)
    for k in ("K", "P", "d", "p", "X", "U"):
        assert a[k].dtype == np.longdouble and b[k].dtype == np.float64
        e = _rel(b[k], a[k])
        print(f"tv={tv} {k}: float64 vs longdouble {e:.2e}")
        assert e <= 1e-11, k
    f = _run(oracle, L, np.float32)
    for k in ("K", "P", "d", "p", "X", "U"):
        assert f[k].dtype == np.float32
        assert _rel(f[k], a[k]) <= 1e-3, k           # float32 ran (eps 6e-8), nothing was promoted


def test_dp_extended_is_the_longdouble_run(lqrx, oracle):
    L = _logical(affine_problem(lqrx, n, m, N, BT, 501))
    Kx, Px = oracle.dp_extended(L["A"], L["B"], L["Q"], L["R"], L["Qf"], N)
    a = _run(oracle, L, np.longdouble, lin=False)
    assert Kx.dtype == np.longdouble and Kx.shape == (BT, N - 1, m, n) and Px.shape == (BT, N, n, n)
    assert np.array_equal(Kx, a["K"]) and np.array_equal(Px, a["P"])


def test_reference_reports_indefinite_knot(lqrx, oracle):
    """R_k = −100·I, B_k ≈ 0 at knot 5 of trajectory 1: info = 5 there, 0 elsewhere (potrf's info,
    as oracle.dp_solve_abi reports it)."""
    from lqrx.dp import to_abi

    d = affine_problem(lqrx, n, m, N, BT, 501, tv_QR=True, tv_AB=True)
    L = _logical(d)
    L["R"] = np.array(L["R"]); L["B"] = np.array(L["B"])
    L["R"][1, 4] = -100.0 * np.eye(m)
    L["B"][1, 4] *= 1e-3
    got = _run(oracle, L, np.float64, lin=False)
    d2 = dict(d, R=to_abi(L["R"].reshape(-1, m, m)).ravel(), B=to_abi(L["B"].reshape(-1, n, m)).ravel())
    ref = oracle.dp_solve_abi(d2, N, all_P=True)
    assert list(got["info"]) == [0, 5, 0] == list(ref["info"])
