"""Cost cross term uᵀMx (lqrx_dp_solve_cross): the checker's identities, the ABI's argument codes
and the wrapper's shape rules.  No device is needed.

tests/dp_truth.py restates the recursion (G = BᵀPA + M_k) in numpy; here it is pinned by
  1. the dense equality-constrained QP with H[u_k, x_k] = M_k and its transpose: X, U within
     1e-10 and P_k x_k + p_k = −(dynamics multiplier) within 1e-9 at every knot (the tolerances of
     tests/test_dp_affine.py);
  2. M = 0: K, P, d, p, X, U of the affine kind, which ignores M, within 1e-10;
  3. the feedback-shift identity against the committed oracle alone: with u = ũ − F x the
     linear-terms problem (A, B, Q, R, q, r, qf) becomes the cross problem (A + BF, B, Q + FᵀRF, R,
     M = RF, q + Fᵀr, r, qf), c = 0, with the same P, p, d, X, and K = K̃ + F, U = Ũ − F X̃; 1e-10.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from dp_truth import (affine_problem, cross_problem, dense_kkt, dp_solve_abi_np, feedback_shift,
                      feedback_shift_reference)


@pytest.mark.parametrize("n,m,N", [(5, 2, 9), (3, 1, 6)])
def test_checker_equals_dense_qp(lqrx, n, m, N):
    """Identity 1, time-varying everything: rollout = QP optimum, P_k x_k + p_k = −multiplier."""
    from lqrx.dp import from_abi

    bt = 3
    d = cross_problem(lqrx, n, m, N, bt, 61 + n, tv_QR=True, tv_AB=True)
    out = dp_solve_abi_np(d, N, "cross", all_P=True)
    assert (out["info"] == 0).all()
    X = out["X"].reshape(bt, N, n)
    U = out["U"].reshape(bt, N - 1, m)
    P = from_abi(out["P"], (bt, N, n, n))
    p = out["p"].reshape(bt, N, n)
    A = from_abi(d["A"], (bt, N - 1, n, n)); B = from_abi(d["B"], (bt, N - 1, n, m))
    Q = from_abi(d["Q"], (bt, N - 1, n, n)); R = from_abi(d["R"], (bt, N - 1, m, m))
    M = from_abi(d["M"], (bt, N - 1, m, n))
    Qf = from_abi(d["Qf"], (bt, n, n)); x0 = d["x0"].reshape(bt, n)
    q = d["q"].reshape(bt, N - 1, n); r = d["r"].reshape(bt, N - 1, m); qf = d["qf"].reshape(bt, n)
    c = d["c"].reshape(bt, N - 1, n)
    assert np.abs(M).max() > 0.05                       # the term is there
    for t in range(bt):
        Xd, Ud, lam = dense_kkt(A[t], B[t], c[t], Q[t], R[t], M[t], Qf[t], x0[t], N, q[t], r[t], qf[t])
        sc = max(1.0, np.abs(Xd).max(), np.abs(Ud).max())
        eX, eU = np.abs(X[t] - Xd).max() / sc, np.abs(U[t] - Ud).max() / sc
        grad = np.einsum("kij,kj->ki", P[t], X[t]) + p[t]
        eL = np.abs(grad + lam).max() / max(1.0, np.abs(lam).max())
        print(f"n={n} m={m} N={N} traj {t}: X {eX:.2e} U {eU:.2e} costate {eL:.2e}")
        assert eX <= 1e-10 and eU <= 1e-10
        assert eL <= 1e-9


@pytest.mark.parametrize("n,m,N", [(6, 3, 20), (4, 1, 30)])
def test_checker_zero_cross_equals_affine_checker(lqrx, n, m, N):
    """Identity 2: M = 0 is the affine recursion."""
    bt = 3
    d = affine_problem(lqrx, n, m, N, bt, 83 + n)
    d["M"] = np.zeros(bt * m * n)
    a = dp_solve_abi_np(d, N, "cross", all_P=True)
    b = dp_solve_abi_np(d, N, "affine", all_P=True)
    assert (a["info"] == 0).all() and (b["info"] == 0).all()
    for k in ("K", "P", "d", "p", "X", "U"):
        e = np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max())
        print(f"n={n} m={m} N={N} {k}: {e:.2e}")
        assert e <= 1e-10, k


@pytest.mark.parametrize("n,m,N", [(6, 3, 20), (4, 1, 30)])
def test_checker_feedback_shift_identity(lqrx, n, m, N):
    """Identity 3: the committed oracle's linear-terms solve is the only reference."""
    from lqrx.dp import from_abi

    bt = 3
    d, dx, F = feedback_shift(lqrx, n, m, N, bt, 300 + n)
    ref = feedback_shift_reference(orc.dp_solve_lin_abi(d, N, all_P=True), F, n, m, N, bt)
    out = dp_solve_abi_np(dx, N, "cross", all_P=True)
    got = dict(K=from_abi(out["K"], (bt, N - 1, m, n)), P=from_abi(out["P"], (bt, N, n, n)),
               X=out["X"].reshape(bt, N, n), U=out["U"].reshape(bt, N - 1, m),
               d=out["d"].reshape(bt, N - 1, m), p=out["p"].reshape(bt, N, n))
    assert (out["info"] == 0).all() and (ref["info"] == 0).all()
    for k in ("K", "P", "d", "p", "X", "U"):
        e = np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())
        print(f"n={n} m={m} N={N} {k}: {e:.2e}")
        assert e <= 1e-10, k


def test_dp_cross_argument_codes(lqrx):
    """lqrx_dp_solve_cross[_host]: codes follow the argument position — desc 1, A 2, B 3, c 4, Q 5,
    R 6, M 7, Qf 8, x0 9, lin 10 (and each of its members), K … U 11 … 14 — and are decided
    before the device is touched; batch = 0 is a valid no-op; n = 0 is a descriptor error."""
    from lqrx import _lib

    lib = lqrx.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.c_void_p)
    full = lambda: _lib.DpLinear(p.value, p.value, p.value, p.value, p.value)
    for host in (False, True):
        fn = lib.lqrx_dp_solve_cross_host if host else lib.lqrx_dp_solve_cross
        tail = (None,) if host else (None, None)       # info[, stream]
        d = _lib.DpDesc(8, 4, 10, 0, 4, 0, 0, 0, 0)
        ln = full()
        call = lambda desc, ins, lin, outs: fn(desc, *ins, lin, *outs, *tail)
        ok_in, ok_out = [p] * 8, [p] * 4
        assert call(None, ok_in, C.byref(ln), ok_out) == -1
        for i in range(8):                              # A, B, c, Q, R, M, Qf, x0 = arguments 2 … 9
            ins = list(ok_in)
            ins[i] = None
            assert call(C.byref(d), ins, C.byref(ln), ok_out) == -(i + 2)
        ins = list(ok_in)
        ins[5] = None
        assert call(C.byref(d), ins, C.byref(ln), ok_out) == -7
        assert "(M)" in lib.lqrx_last_error().decode()
        assert call(C.byref(d), ok_in, None, ok_out) == -10
        for k in ("q", "r", "qf", "d", "p"):
            l2 = full()
            setattr(l2, k, None)
            assert call(C.byref(d), ok_in, C.byref(l2), ok_out) == -10
            assert k in lib.lqrx_last_error().decode()
        for i in range(4):                              # K, P, X, U = arguments 11 … 14
            outs = list(ok_out)
            outs[i] = None
            assert call(C.byref(d), ok_in, C.byref(ln), outs) == -(i + 11)
        d0 = _lib.DpDesc(8, 4, 10, 0, 0, 0, 0, 0, 0)
        assert call(C.byref(d0), [None] * 8, None, [None] * 4) == 0     # batch = 0
        d.n = 0
        assert call(C.byref(d), ok_in, C.byref(ln), ok_out) == -1


def test_header_declares_cross_entries(lqrx):
    from lqrx import _lib

    names = _lib.header_functions()
    assert "lqrx_dp_solve_cross" in names and "lqrx_dp_solve_cross_host" in names
    assert lqrx.load().lqrx_abi_version() == 5          # additive: detected by symbol


def _problem(n, m, N, M, tv):
    from lqrx.dp import LQRProblem

    rng = np.random.default_rng(5)
    A = rng.standard_normal((n, n)) * 0.3
    B = rng.standard_normal((n, m))
    Q = np.broadcast_to(np.eye(n), (N - 1, n, n)).copy() if tv else np.eye(n)
    R = np.broadcast_to(np.eye(m), (N - 1, m, m)).copy() if tv else np.eye(m)
    return LQRProblem(Qf=np.eye(n), Q=Q, R=R, A=A, B=B, x0=np.ones(n), N=N, M=M)


def test_wrapper_rejects_knot_axis_mismatch(lqrx):
    """A knot axis on M needs one on Q and R, and vice versa (no device is reached)."""
    from lqrx.dp import LQRBatch, solve_batch

    n, m, N = 3, 1, 6
    with pytest.raises(ValueError):
        LQRBatch.of([_problem(n, m, N, np.zeros((N - 1, m, n)), tv=False)])
    with pytest.raises(ValueError):
        LQRBatch.of([_problem(n, m, N, np.zeros((m, n)), tv=True)])
    b = LQRBatch.of([_problem(n, m, N, np.zeros((m, n)), tv=False)])
    b.M = np.zeros((1, N - 1, m, n))
    with pytest.raises(ValueError):
        solve_batch(b)
    b.M = np.zeros((1, n, m))                           # the shape of Kᵀ, not of K
    with pytest.raises(ValueError):
        solve_batch(b)


def test_wrapper_rejects_devices_with_cross_term(lqrx):
    from lqrx.dp import LQRBatch, solve_batch

    b = LQRBatch.of([_problem(3, 1, 6, np.zeros((1, 3)), tv=False)])
    with pytest.raises(ValueError):
        solve_batch(b, devices=[0])
