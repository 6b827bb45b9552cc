"""Affine dynamics x⁺ = A x + B u + c (lqrx_dp_solve_affine): the checker's identities, the
ABI's argument codes and the wrapper's shape rules.  No device is needed.

tests/dp_truth.py restates the recursion in numpy; here it is pinned by
  1. the dense equality-constrained QP with rows x_{k+1} − A x_k − B u_k = c_k: X, U within
     1e-10 and P_k x_k + p_k = −(dynamics multiplier) within 1e-9 at every knot (the
     tolerances of tests/test_oracle.py::test_dp_oracle_linear_equals_dense_kkt);
  2. c = 0: K, P, d, p, X, U of oracle.dp_solve_lin_abi within 1e-10.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from dp_truth import affine_problem, dense_kkt, dp_solve_abi_np


@pytest.mark.parametrize("n,m,N", [(5, 2, 9), (3, 1, 6)])
def test_checker_equals_dense_qp(lqrx, n, m, N):
    """Identity 1, time-varying: rollout = QP optimum, P_k x_k + p_k = −multiplier."""
    from lqrx.dp import from_abi

    bt = 3
    d = affine_problem(lqrx, n, m, N, bt, 61 + n, tv_QR=True, tv_AB=True)
    out = dp_solve_abi_np(d, N, "affine", all_P=True)
    assert (out["info"] == 0).all()
    X = out["X"].reshape(bt, N, n)
    U = out["U"].reshape(bt, N - 1, m)
    P = from_abi(out["P"], (bt, N, n, n))
    p = out["p"].reshape(bt, N, n)
    A = from_abi(d["A"], (bt, N - 1, n, n)); B = from_abi(d["B"], (bt, N - 1, n, m))
    Q = from_abi(d["Q"], (bt, N - 1, n, n)); R = from_abi(d["R"], (bt, N - 1, m, m))
    Qf = from_abi(d["Qf"], (bt, n, n)); x0 = d["x0"].reshape(bt, n)
    q = d["q"].reshape(bt, N - 1, n); r = d["r"].reshape(bt, N - 1, m); qf = d["qf"].reshape(bt, n)
    c = d["c"].reshape(bt, N - 1, n)
    for t in range(bt):
        Xd, Ud, lam = dense_kkt(A[t], B[t], c[t], Q[t], R[t], None, Qf[t], x0[t], N, q[t], r[t], qf[t])
        sc = max(1.0, np.abs(Xd).max(), np.abs(Ud).max())
        eX, eU = np.abs(X[t] - Xd).max() / sc, np.abs(U[t] - Ud).max() / sc
        grad = np.einsum("kij,kj->ki", P[t], X[t]) + p[t]
        eL = np.abs(grad + lam).max() / max(1.0, np.abs(lam).max())
        print(f"n={n} m={m} N={N} traj {t}: X {eX:.2e} U {eU:.2e} costate {eL:.2e}")
        assert eX <= 1e-10 and eU <= 1e-10
        assert eL <= 1e-9


@pytest.mark.parametrize("n,m,N", [(6, 3, 20), (4, 1, 30)])
def test_checker_zero_offset_equals_linear_oracle(lqrx, n, m, N):
    """Identity 2: c = 0 is the linear-terms recursion of the committed oracle."""
    bt = 3
    d = affine_problem(lqrx, n, m, N, bt, 83 + n)
    d["c"] = np.zeros_like(d["c"])
    a = dp_solve_abi_np(d, N, "affine", all_P=True)
    b = orc.dp_solve_lin_abi(d, N, all_P=True)
    assert (a["info"] == 0).all() and (b["info"] == 0).all()
    for k in ("K", "P", "d", "p", "X", "U"):
        e = np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max())
        print(f"n={n} m={m} N={N} {k}: {e:.2e}")
        assert e <= 1e-10, k


def test_dp_affine_argument_codes(lqrx):
    """lqrx_dp_solve_affine[_host]: codes follow the argument position — desc 1, c 4, lin 9
    (and each of its members), K … U 10 … 13 — and are decided before the device is touched;
    batch = 0 is a valid no-op."""
    from lqrx import _lib

    lib = lqrx.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.c_void_p)
    full = lambda: _lib.DpLinear(p.value, p.value, p.value, p.value, p.value)
    for host in (False, True):
        fn = lib.lqrx_dp_solve_affine_host if host else lib.lqrx_dp_solve_affine
        tail = (None,) if host else (None, None)       # info[, stream]
        d = _lib.DpDesc(8, 4, 10, 0, 4, 0, 0, 0, 0)
        ln = full()
        call = lambda desc, ins, lin, outs: fn(desc, *ins, lin, *outs, *tail)
        ok_in, ok_out = [p] * 7, [p] * 4
        assert call(None, ok_in, C.byref(ln), ok_out) == -1
        for i in range(7):                              # A, B, c, Q, R, Qf, x0 = arguments 2 … 8
            ins = list(ok_in)
            ins[i] = None
            assert call(C.byref(d), ins, C.byref(ln), ok_out) == -(i + 2)
        assert call(C.byref(d), ok_in, None, ok_out) == -9
        for k in ("q", "r", "qf", "d", "p"):
            l2 = full()
            setattr(l2, k, None)
            assert call(C.byref(d), ok_in, C.byref(l2), ok_out) == -9
            assert k in lib.lqrx_last_error().decode()
        for i in range(4):                              # K, P, X, U = arguments 10 … 13
            outs = list(ok_out)
            outs[i] = None
            assert call(C.byref(d), ok_in, C.byref(ln), outs) == -(i + 10)
        d0 = _lib.DpDesc(8, 4, 10, 0, 0, 0, 0, 0, 0)
        assert call(C.byref(d0), [None] * 7, None, [None] * 4) == 0     # batch = 0
        d.n = 0
        assert call(C.byref(d), ok_in, C.byref(ln), ok_out) == -1


def test_header_declares_affine_entries(lqrx):
    from lqrx import _lib

    names = _lib.header_functions()
    assert "lqrx_dp_solve_affine" in names and "lqrx_dp_solve_affine_host" in names
    assert lqrx.load().lqrx_abi_version() == 5          # additive: detected by symbol


def _problem(n, m, N, c, tv):
    from lqrx.dp import LQRProblem

    rng = np.random.default_rng(5)
    A = rng.standard_normal((N - 1, n, n) if tv else (n, n)) * 0.3
    B = rng.standard_normal((N - 1, n, m) if tv else (n, m))
    return LQRProblem(Qf=np.eye(n), Q=np.eye(n), R=np.eye(m), A=A, B=B, x0=np.ones(n), N=N, c=c)


def test_wrapper_rejects_knot_axis_mismatch(lqrx):
    """A knot axis on c needs one on A and B, and vice versa (no device is reached)."""
    from lqrx.dp import LQRBatch, solve_batch

    n, m, N = 3, 1, 6
    with pytest.raises(ValueError):
        LQRBatch.of([_problem(n, m, N, np.zeros((N - 1, n)), tv=False)])
    with pytest.raises(ValueError):
        LQRBatch.of([_problem(n, m, N, np.zeros(n), tv=True)])
    b = LQRBatch.of([_problem(n, m, N, np.zeros(n), tv=False)])
    b.c = np.zeros((1, N - 1, n))
    with pytest.raises(ValueError):
        solve_batch(b)


def test_wrapper_rejects_devices_with_offset(lqrx):
    from lqrx.dp import LQRBatch, solve_batch

    b = LQRBatch.of([_problem(3, 1, 6, np.zeros(3), tv=False)])
    with pytest.raises(ValueError):
        solve_batch(b, devices=[0])
