"""Value-function constant (lqrx_dp_solve_value): the checker's identities, the ABI's argument codes
and the wrapper's rules.  No device is needed.

tests/dp_truth.py extends the cross recursion with s_k, dV = Σ h_kᵀd_k and
J = V_1(x0); here it is pinned by
  1. the dense equality-constrained QP of dp_truth.dense_kkt: J equals the cost of the
     QP's optimum, evaluated term by term by cost_of(), within 1e-10 of max(1, S + |J|);
  2. c = 0 ⇒ s_1 = −½dV;
  3. s_N = 0, and the all-P s_1 equals the P_1-only s.
"""
import ctypes as C

import numpy as np
import pytest

from dp_truth import cost_of, cross_problem, dense_kkt, dp_solve_abi_np


def _per_knot(a, bt, k, N, *shape):
    """(bt, k, …) logical blocks of a flat ABI array, broadcast to N−1 knots."""
    from lqrx.dp import from_abi

    a = from_abi(a, (bt, k) + shape) if len(shape) == 2 else np.asarray(a).reshape((bt, k) + shape)
    return np.broadcast_to(a, (bt, N - 1) + shape) if k == 1 else a


@pytest.mark.parametrize("n,m,N,tv", [(4, 2, 8, False), (6, 3, 10, True)])
def test_checker_cost_equals_dense_qp(lqrx, n, m, N, tv):
    """Identity 1: J of the recursion = the cost of the QP optimum; and = the cost of the
    checker's own rollout."""
    from lqrx.dp import from_abi

    bt = 3
    d = cross_problem(lqrx, n, m, N, bt, 900 + n, tv_QR=tv, tv_AB=tv)
    out = dp_solve_abi_np(d, N, "value")
    assert (out["info"] == 0).all()
    k = N - 1 if tv else 1
    A = _per_knot(d["A"], bt, k, N, n, n); B = _per_knot(d["B"], bt, k, N, n, m)
    Q = _per_knot(d["Q"], bt, k, N, n, n); R = _per_knot(d["R"], bt, k, N, m, m)
    M = _per_knot(d["M"], bt, k, N, m, n)
    c = _per_knot(d["c"], bt, k, N, n); q = _per_knot(d["q"], bt, k, N, n); r = _per_knot(d["r"], bt, k, N, m)
    Qf = from_abi(d["Qf"], (bt, n, n)); x0 = d["x0"].reshape(bt, n); qf = d["qf"].reshape(bt, n)
    assert np.abs(c).max() > 0.01 and np.abs(q).max() > 0.01      # the constant is not −½dV here
    Xd = np.zeros((bt, N, n)); Ud = np.zeros((bt, N - 1, m))
    for t in range(bt):
        Xd[t], Ud[t], _ = dense_kkt(A[t], B[t], c[t], Q[t], R[t], M[t], Qf[t], x0[t], N, q[t], r[t], qf[t])
    Jqp = cost_of(d, Xd, Ud)
    Jro = cost_of(d, out["X"], out["U"])
    sc = np.maximum(1, out["S"] + np.abs(Jqp))
    e1, e2 = np.abs(out["J"] - Jqp) / sc, np.abs(out["J"] - Jro) / sc
    print(f"n={n} m={m} N={N} tv={tv}: J {out['J']}  vs QP {e1.max():.2e}  vs rollout {e2.max():.2e}  S {out['S']}")
    assert np.abs(out["s"] + 0.5 * out["dV"]).min() > 1e-3         # s_1 carries the c terms
    assert e1.max() <= 1e-10 and e2.max() <= 1e-10


def test_checker_zero_offset_constant_is_minus_half_dV(lqrx):
    """Identity 2: c = 0 ⇒ s_1 = −½dV, and dV ≥ 0."""
    n, m, N, bt = 6, 3, 20, 3
    d = cross_problem(lqrx, n, m, N, bt, 77)
    d["c"] = np.zeros_like(d["c"])
    out = dp_solve_abi_np(d, N, "value")
    e = np.abs(out["s"] + 0.5 * out["dV"]) / np.maximum(1, out["S"])
    print("s_1 + dV/2:", e, "dV", out["dV"])
    assert (out["dV"] > 0).all() and e.max() <= 1e-14


def test_checker_p_modes_agree(lqrx):
    """Identity 3: s_N = 0; the all-P s_1 is the P_1-only s."""
    n, m, N, bt = 5, 2, 9, 3
    d = cross_problem(lqrx, n, m, N, bt, 78, tv_QR=True, tv_AB=True)
    a = dp_solve_abi_np(d, N, "value", all_P=True)
    b = dp_solve_abi_np(d, N, "value")
    sa = a["s"].reshape(bt, N)
    assert (sa[:, N - 1] == 0).all()
    assert np.array_equal(sa[:, 0], b["s"]) and np.array_equal(a["dV"], b["dV"]) and np.array_equal(a["J"], b["J"])


def test_dp_value_argument_codes(lqrx):
    """lqrx_dp_solve_value[_host]: codes follow the argument position — desc 1, A 2, B 3, c 4, Q 5,
    R 6, M 7, Qf 8, x0 9, lin 10 (and each of its members), val 11 (and its member s), K … U
    12 … 15 — and are decided before the device is touched; NULL dV and J are accepted; batch = 0
    is a valid no-op; n = 0 is a descriptor error."""
    from lqrx import _lib

    lib = lqrx.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.c_void_p)
    full = lambda: _lib.DpLinear(p.value, p.value, p.value, p.value, p.value)
    for host in (False, True):
        fn = lib.lqrx_dp_solve_value_host if host else lib.lqrx_dp_solve_value
        tail = (None,) if host else (None, None)       # info[, stream]
        d = _lib.DpDesc(8, 4, 10, 0, 4, 0, 0, 0, 0)
        ln = full()
        vl = _lib.DpValue(p.value, p.value, p.value)
        call = lambda desc, ins, lin, val, outs: fn(desc, *ins, lin, val, *outs, *tail)
        ok_in, ok_out = [p] * 8, [p] * 4
        assert call(None, ok_in, C.byref(ln), C.byref(vl), ok_out) == -1
        for i in range(8):                              # A, B, c, Q, R, M, Qf, x0 = arguments 2 … 9
            ins = list(ok_in)
            ins[i] = None
            assert call(C.byref(d), ins, C.byref(ln), C.byref(vl), ok_out) == -(i + 2)
        assert call(C.byref(d), ok_in, None, C.byref(vl), ok_out) == -10
        for k in ("q", "r", "qf", "d", "p"):
            l2 = full()
            setattr(l2, k, None)
            assert call(C.byref(d), ok_in, C.byref(l2), C.byref(vl), ok_out) == -10
            assert k in lib.lqrx_last_error().decode()
        assert call(C.byref(d), ok_in, C.byref(ln), None, ok_out) == -11
        assert "val" in lib.lqrx_last_error().decode()
        v2 = _lib.DpValue(None, p.value, p.value)
        assert call(C.byref(d), ok_in, C.byref(ln), C.byref(v2), ok_out) == -11
        assert "s" in lib.lqrx_last_error().decode() and "val->s" in lib.lqrx_last_error().decode()
        v3 = _lib.DpValue(p.value, None, None)          # dV, J optional: validation goes on to K … U
        for i in range(4):                              # K, P, X, U = arguments 12 … 15
            outs = list(ok_out)
            outs[i] = None
            assert call(C.byref(d), ok_in, C.byref(ln), C.byref(vl), outs) == -(i + 12)
            assert call(C.byref(d), ok_in, C.byref(ln), C.byref(v3), outs) == -(i + 12)
        d0 = _lib.DpDesc(8, 4, 10, 0, 0, 0, 0, 0, 0)
        assert call(C.byref(d0), [None] * 8, None, None, [None] * 4) == 0     # batch = 0
        d.n = 0
        assert call(C.byref(d), ok_in, C.byref(ln), C.byref(vl), ok_out) == -1


def test_header_declares_value_entries(lqrx):
    from lqrx import _lib

    names = _lib.header_functions()
    assert "lqrx_dp_solve_value" in names and "lqrx_dp_solve_value_host" in names
    assert "lqrx_dp_value" in open(_lib.HEADER_PATH).read()
    assert lqrx.load().lqrx_abi_version() == 5          # additive: detected by symbol


def _problem(n, m, N):
    from lqrx.dp import LQRProblem

    rng = np.random.default_rng(5)
    return LQRProblem(Qf=np.eye(n), Q=np.eye(n), R=np.eye(m), A=rng.standard_normal((n, n)) * 0.3,
                      B=rng.standard_normal((n, m)), x0=np.ones(n), N=N)


def test_wrapper_value_defaults_and_devices(lqrx):
    """LQRSolution carries s, dV, J only when asked; value=True has no devices= form (no device
    is reached)."""
    from lqrx.dp import LQRBatch, LQRSolution, solve_batch

    prob = _problem(3, 1, 6)
    sol = LQRSolution.of(prob)
    assert sol.s is None and sol.dV is None and sol.J is None and sol.d is None
    sol = LQRSolution.of(prob, all_P=True, value=True)
    assert sol.s.shape == (6,) and sol.dV is not None and sol.J is not None
    assert sol.d is not None and sol.p.shape == (6, 3)
    assert LQRSolution.of(prob, value=True).s.shape == ()
    with pytest.raises(ValueError):
        solve_batch(LQRBatch.of([prob]), devices=[0], value=True)
