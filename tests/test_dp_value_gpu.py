"""GPU parity: the value function's constant (lqrx_dp_solve_value) — s_k, dV = Σ h_kᵀd_k and
J = V_1(x0) on top of the cross solve.

Checker: tests/dp_truth.py (numpy float64; pinned to the dense QP in tests/test_dp_value.py).
Independently of it, J is compared with the cost of the GPU's own X, U, evaluated term by term.
Error measures (dp_truth.value_errors): s and dV relative to max(1, S), J relative to
max(1, S + |J|), S = Σ_k (|c_kᵀ(p + ½Pc_k)| + ½|h_kᵀd_k|) per trajectory.  Tolerances are the
project's: fp64 1e-10, fp32 1e-4.
The fp32 bound: the checker run in float32 against float64 on the CPU at the three fp32 shapes
below, on the same error measures, is worst at 5.0e-7 (s at (6, 3, 30, 7); per shape the worst of
s, dV, J is 5.0e-7, 1.1e-7, 1.0e-7), so 1e-4 leaves the kernels more than two decades.
Kernels: n ≤ 4 dp_lane_kernel<…, LIN, AFF, CROSS, VALUE>, n ≥ 5 dp_riccati_kernel<…, VAR_LIN |
VAR_AFF | VAR_CROSS | VAR_VALUE [| VAR_TV]> (fp64 n = 64 too — never dp_wg4_kernel), past the
register tiles dp_big_kernel; J from dp_value_cost_kernel behind each of them.
"""
import ctypes as C

import numpy as np
import pytest

from dp_truth import (F32_SHAPES, PARITY, check, cost_of, cross_problem, dp_solve_abi_np, logical, to_batch,
                      value_errors)

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL32 = 1e-4
OUT = ("K", "P", "X", "U", "d", "p", "info")


def check_value(got, ref, tol, what="", keep=None):
    """Prints the worst s, dV, J error over the trajectories `keep` (all by default), then asserts."""
    e = value_errors(got, ref)
    if keep is not None:
        e = {k: v[keep] for k, v in e.items()}
    print(what, " ".join(f"{k} {v.max():.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v.max() <= tol, (k, v)


@pytest.mark.parametrize("n,m,N,bt,tvq,tvab,all_P", PARITY)
def test_dp_value_parity_f64(lqrx, gpu_ok, n, m, N, bt, tvq, tvab, all_P):
    d = cross_problem(lqrx, n, m, N, bt, 5100 + 11 * n + m, tvq, tvab)
    got = lqrx.solve_batch(to_batch(d, N), all_P=all_P, value=True)
    assert got["rc"] == 0
    ref = dp_solve_abi_np(d, N, "value", all_P=all_P)
    assert got["s"].shape == ((bt, N) if all_P else (bt,))
    check(got, logical(ref, n, m, N, bt, all_P), all_P, TOL64, f"f64 {n},{m},{N},{bt}")
    check_value(got, ref, TOL64, f"f64 {n},{m},{N},{bt}")


@pytest.mark.parametrize("n,m,N,bt,tv", F32_SHAPES)
def test_dp_value_parity_f32(lqrx, gpu_ok, n, m, N, bt, tv):
    d = cross_problem(lqrx, n, m, N, bt, 700 + n, tv, tv)
    got = lqrx.solve_batch(to_batch(d, N), dtype=1, all_P=True, value=True)
    ref = dp_solve_abi_np(d, N, "value", all_P=True)
    assert got["s"].dtype == np.float32 and got["J"].dtype == np.float32
    check_value(got, ref, TOL32, f"f32 {n},{m},{N},{bt}")


@pytest.mark.parametrize("n,m,N,bt", [(4, 2, 30, 5), (6, 3, 30, 7), (32, 16, 40, 3), (65, 4, 8, 2)])
def test_dp_value_cost_of_own_rollout(lqrx, gpu_ok, n, m, N, bt):
    """No checker: J is the cost of the X, U the same call returned, evaluated term by term.  (S,
    the scale, is the only thing taken from the checker.)"""
    d = cross_problem(lqrx, n, m, N, bt, 6100 + n)
    got = lqrx.solve_batch(to_batch(d, N), value=True)
    assert (got["info"] == 0).all()
    J = cost_of(d, got["X"], got["U"])
    S = dp_solve_abi_np(d, N, "value")["S"]
    e = np.abs(got["J"] - J) / np.maximum(1, S + np.abs(J))
    print(f"{n},{m},{N},{bt}: J {got['J']} cost {J} err {e.max():.2e}")
    assert e.max() <= TOL64


@pytest.mark.parametrize("n,m,N,bt,tv", [(4, 1, 30, 5, False), (32, 16, 40, 3, False), (70, 8, 9, 3, True)])
def test_dp_value_same_solve_as_cross(lqrx, gpu_ok, n, m, N, bt, tv):
    """K, P, X, U, d, p, info: the bits of lqrx_dp_solve_cross on the same data."""
    d = cross_problem(lqrx, n, m, N, bt, 41 + n, tv, tv)
    b = to_batch(d, N)
    a = lqrx.solve_batch(b, all_P=True, value=True)
    ref = lqrx.solve_batch(b, all_P=True)
    assert (ref["info"] == 0).all() and np.abs(ref["K"]).max() > 0
    for k in OUT:
        assert np.array_equal(a[k], ref[k]), k


def test_dp_value_zero_offset(lqrx, gpu_ok):
    """c = 0 ⇒ s_1 = −½dV (to rounding of the one subtraction; both sides are the GPU's)."""
    n, m, N, bt = 6, 3, 30, 7
    d = cross_problem(lqrx, n, m, N, bt, 515)
    d["c"] = np.zeros_like(d["c"])
    got = lqrx.solve_batch(to_batch(d, N), value=True)
    S = dp_solve_abi_np(d, N, "value")["S"]
    e = np.abs(got["s"] + 0.5 * got["dV"]) / np.maximum(1, S)
    print("s_1 + dV/2:", e)
    assert (got["dV"] > 0).all() and e.max() <= TOL64


@pytest.mark.parametrize("n,m,N,bt,tv", [(4, 2, 30, 5, False), (6, 3, 30, 7, False), (17, 5, 12, 3, True),
                                         (65, 4, 8, 2, False)])
def test_dp_value_p_modes(lqrx, gpu_ok, n, m, N, bt, tv):
    """p_mode 1 reduces the running sums, not the increments: its s_1 is the p_mode-0 s, bit for
    bit; s_N = 0; dV and J do not depend on the mode."""
    d = cross_problem(lqrx, n, m, N, bt, 333 + n, tv, tv)
    b = to_batch(d, N)
    a1 = lqrx.solve_batch(b, all_P=True, value=True)
    a0 = lqrx.solve_batch(b, all_P=False, value=True)
    assert np.array_equal(a1["s"][:, 0], a0["s"]) and np.abs(a0["s"]).min() > 0
    assert (a1["s"][:, N - 1] == 0).all()
    assert np.array_equal(a1["dV"], a0["dV"]) and np.array_equal(a1["J"], a0["J"])


@pytest.mark.parametrize("n,m,N,bt", [(4, 2, 50, 70), (32, 16, 40, 3)])   # native SoA lane kernel; staged
def test_dp_value_layout1(lqrx, gpu_ok, n, m, N, bt):
    """Layout 1 (SoA): bit-identical to layout 0, every s_k included.  Per-knot everything."""
    d = cross_problem(lqrx, n, m, N, bt, 177 + n, tv_QR=True, tv_AB=True)
    b = to_batch(d, N)
    a0 = lqrx.solve_batch(b, all_P=True, layout=0, value=True)
    a1 = lqrx.solve_batch(b, all_P=True, layout=1, value=True)
    assert (a0["info"] == 0).all() and np.abs(a0["s"][:, :-1]).min() > 0
    for k in OUT + ("s", "dV", "J"):
        assert np.array_equal(a0[k], a1[k]), k
    b0 = lqrx.solve_batch(b, layout=0, value=True)
    b1 = lqrx.solve_batch(b, layout=1, value=True)
    for k in ("s", "dV", "J"):
        assert np.array_equal(b0[k], b1[k]) and np.array_equal(b0[k], a0[k] if k != "s" else a0[k][:, 0]), k


def _value_host(lqrx, d, N, want_dV, want_J):
    """lqrx_dp_solve_value_host on the flat ABI arrays of d (layout 0, p_mode 0) → (s, dV, J)."""
    from lqrx import _lib

    lib = lqrx.load()
    n, m, bt = d["n"], d["m"], d["batch"]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ins = {k: np.ascontiguousarray(d[k], np.float64) for k in ("A", "B", "c", "Q", "R", "M", "Qf", "x0", "q", "r", "qf")}
    K = np.zeros(bt * (N - 1) * m * n); P = np.zeros(bt * n * n); X = np.zeros(bt * N * n)
    U = np.zeros(bt * (N - 1) * m); dd = np.zeros(bt * (N - 1) * m); pp = np.zeros(bt * n)
    s, dV, J = np.full(bt, np.nan), np.full(bt, np.nan), np.full(bt, np.nan)
    info = np.zeros(bt, np.int32)
    desc = _lib.DpDesc(n, m, N, 0, bt, 0, 0, 0, 0)
    ln = _lib.DpLinear(ptr(ins["q"]).value, ptr(ins["r"]).value, ptr(ins["qf"]).value, ptr(dd).value, ptr(pp).value)
    vl = _lib.DpValue(ptr(s).value, ptr(dV).value if want_dV else None, ptr(J).value if want_J else None)
    rc = lib.lqrx_dp_solve_value_host(C.byref(desc), *[ptr(ins[k]) for k in ("A", "B", "c", "Q", "R", "M", "Qf", "x0")],
                                      C.byref(ln), C.byref(vl), ptr(K), ptr(P), ptr(X), ptr(U), ptr(info))
    assert rc == 0, lib.lqrx_last_error().decode()
    return s, dV, J


@pytest.mark.parametrize("n,m,N,bt", [(4, 2, 30, 5), (32, 16, 40, 3), (65, 4, 8, 2)])
def test_dp_value_null_dV_and_J(lqrx, gpu_ok, n, m, N, bt):
    """val->dV and val->J may be NULL, each alone or both: s is the same bits, the other is still
    written, and a NULL one is not touched."""
    d = cross_problem(lqrx, n, m, N, bt, 271 + n)
    s, dV, J = _value_host(lqrx, d, N, True, True)
    assert np.isfinite(s).all() and np.isfinite(dV).all() and np.isfinite(J).all()
    for want_dV, want_J in ((False, False), (True, False), (False, True)):
        s2, dV2, J2 = _value_host(lqrx, d, N, want_dV, want_J)
        assert np.array_equal(s2, s)
        assert np.array_equal(dV2, dV) if want_dV else np.isnan(dV2).all()
        assert np.array_equal(J2, J) if want_J else np.isnan(J2).all()


def test_dp_value_device_stream(lqrx, gpu_ok):
    """Device-pointer entry on a created stream, synchronised before checking."""
    import torch

    n, m, N, bt = 32, 16, 40, 4
    d = cross_problem(lqrx, n, m, N, bt, 321)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.asarray(d[k])).to(dev)
         for k in ("A", "B", "Q", "R", "Qf", "x0", "q", "r", "qf", "c", "M")}
    t.update(n=n, m=m, batch=bt)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = lqrx.dp_solve_device(t, N, p_mode=1, stream=s.cuda_stream, value=True)
    s.synchronize()
    ref = dp_solve_abi_np(d, N, "value", all_P=True)
    got = logical({k: out[k].cpu().numpy() for k in OUT}, n, m, N, bt, True)
    check(got, logical(ref, n, m, N, bt, True), True, TOL64, "stream")
    check_value({k: out[k].cpu().numpy() for k in ("s", "dV", "J")}, ref, TOL64, "stream")


def test_dp_value_info_leaves_other_trajectories_alone(lqrx, gpu_ok):
    """R negated at one trajectory: info equals the checker's; s, dV, J of the other three pass
    parity (the bad trajectory's values are unspecified and not compared)."""
    from lqrx.dp import from_abi, to_abi

    n, m, N, bt = 6, 3, 12, 4
    d = cross_problem(lqrx, n, m, N, bt, 4242)
    R = from_abi(d["R"], (bt, m, m)).copy()
    R[2] = -R[2]
    d["R"] = to_abi(R).ravel()
    a = lqrx.solve_batch(to_batch(d, N), all_P=True, value=True)
    ref = dp_solve_abi_np(d, N, "value", all_P=True)
    print("info", a["info"], ref["info"])
    assert ref["info"][2] != 0 and (np.delete(ref["info"], 2) == 0).all()
    assert np.array_equal(a["info"], ref["info"])
    check_value(a, ref, TOL64, "info", keep=np.array([0, 1, 3]))


def test_dp_value_single_problem_api(lqrx, gpu_ok):
    """LQRSolution.of(prob, value=True) → solve(sol, DPSolver, prob) fills sol.s, sol.dV, sol.J
    (and d, p); the problem has no M, which is passed as zeros."""
    from lqrx.dp import DPSolver, LQRProblem, LQRSolution, from_abi

    n, m, N = 6, 2, 30
    d = cross_problem(lqrx, n, m, N, 1, 2025)
    d["M"] = np.zeros_like(d["M"])
    prob = LQRProblem(Qf=from_abi(d["Qf"], (1, n, n))[0], Q=from_abi(d["Q"], (1, n, n))[0],
                      R=from_abi(d["R"], (1, m, m))[0], A=from_abi(d["A"], (1, n, n))[0],
                      B=from_abi(d["B"], (1, n, m))[0], x0=d["x0"].copy(), N=N,
                      q=d["q"].copy(), r=d["r"].copy(), qf=d["qf"].copy(), c=d["c"].copy())
    sol = LQRSolution.of(prob, all_P=True, value=True)
    lqrx.solve(sol, DPSolver.of(prob), prob)
    ref = dp_solve_abi_np(d, N, "value", all_P=True)
    got = dict(K=sol.K[None], P=sol.P[None], X=sol.X[None], U=sol.U[None], d=sol.d[None], p=sol.p[None],
               info=np.array([sol.info]))
    check(got, logical(ref, n, m, N, 1, True), True, TOL64, "single")
    assert sol.s.shape == (N,) and sol.s[N - 1] == 0 and sol.dV > 0
    check_value(dict(s=sol.s[None], dV=np.array([sol.dV]), J=np.array([sol.J])), ref, TOL64, "single")
