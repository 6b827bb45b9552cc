"""GPU parity: DP with a cost cross term uᵀMx (lqrx_dp_solve_cross), G = BᵀPA + M_k.

Checker: tests/dp_truth.py (numpy float64; pinned to the dense QP, to the affine checker and
to the committed oracle in tests/test_dp_cross.py).  Independently of it, the feedback-shift
identity below compares against oracle.dp_solve_lin_abi alone.  Tolerances are those of
tests/test_dp_linear_gpu.py and tests/test_dp_affine_gpu.py, measured the same way: fp64 1e-10,
fp32 1e-4; K and P per knot, d, p, X, U on their trajectory's scale.
The fp32 bound: the checker run in float32 against float64 on the CPU at the three fp32 shapes
below, on the same error measures, is worst at 4.1e-6 (K at (64, 32, 12, 2); per shape the worst
of K, P, d, p, X, U is 2.5e-6, 2.8e-6, 4.1e-6), so 1e-4 leaves the kernels more than a decade.
Kernels: n ≤ 4 dp_lane_kernel<…, LIN, AFF, CROSS>, n ≥ 5 dp_riccati_kernel<…, VAR_LIN | VAR_AFF |
VAR_CROSS [| VAR_TV]> (fp64 n = 64 too — never dp_wg4_kernel), past the register tiles
dp_big_kernel.
"""
import numpy as np
import pytest

from dp_truth import (F32_SHAPES, PARITY, check, cross_problem, dp_solve_abi_np, feedback_shift,
                      feedback_shift_reference, logical, to_batch)

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL32 = 1e-4


@pytest.mark.parametrize("n,m,N,bt,tvq,tvab,all_P", PARITY)
def test_dp_cross_parity_f64(lqrx, gpu_ok, n, m, N, bt, tvq, tvab, all_P):
    d = cross_problem(lqrx, n, m, N, bt, 5100 + 11 * n + m, tvq, tvab)
    got = lqrx.solve_batch(to_batch(d, N), all_P=all_P)
    assert got["rc"] == 0
    ref = logical(dp_solve_abi_np(d, N, "cross", all_P=all_P), n, m, N, bt, all_P)
    check(got, ref, all_P, TOL64, f"f64 {n},{m},{N},{bt}")


@pytest.mark.parametrize("n,m,N,bt,tv", F32_SHAPES)
def test_dp_cross_parity_f32(lqrx, gpu_ok, n, m, N, bt, tv):
    d = cross_problem(lqrx, n, m, N, bt, 700 + n, tv, tv)
    got = lqrx.solve_batch(to_batch(d, N), dtype=1, all_P=True)
    ref = logical(dp_solve_abi_np(d, N, "cross", all_P=True), n, m, N, bt, True)
    check(got, ref, True, TOL32, f"f32 {n},{m},{N},{bt}")


@pytest.mark.parametrize("n,m,N,bt", [(4, 2, 30, 5), (6, 3, 30, 7), (32, 16, 40, 3)])
def test_dp_cross_feedback_shift_identity(lqrx, oracle, gpu_ok, n, m, N, bt):
    """u = ũ − F x turns the linear-terms problem (A, B, Q, R, q, r, qf) into the cross problem
    (A + BF, B, Q + FᵀRF, R, M = RF, q + Fᵀr, r, qf), c = 0: P, p, d, X are the linear-terms ones,
    K = K̃ + F, U = Ũ − F X̃.  Reference: the committed oracle's linear-terms solve only."""
    d, dx, F = feedback_shift(lqrx, n, m, N, bt, 8800 + n)
    got = lqrx.solve_batch(to_batch(dx, N), all_P=True)
    assert got["rc"] == 0
    ref = feedback_shift_reference(oracle.dp_solve_lin_abi(d, N, all_P=True), F, n, m, N, bt)
    check(got, ref, True, TOL64, f"feedback shift {n},{m},{N},{bt}")


@pytest.mark.parametrize("n,m,N,bt", [(4, 1, 30, 5), (32, 16, 40, 3)])
def test_dp_cross_zero_cross_equals_affine(lqrx, gpu_ok, n, m, N, bt):
    """M = 0: the results of lqrx_dp_solve_affine on the same data."""
    d = cross_problem(lqrx, n, m, N, bt, 19 + n)
    d["M"] = np.zeros_like(d["M"])
    a = lqrx.solve_batch(to_batch(d, N), all_P=True)
    ref = lqrx.solve_batch(to_batch(d, N, fields=("q", "r", "qf", "c")), all_P=True)
    check(a, ref, True, TOL64, f"M=0 {n},{m},{N},{bt}")


@pytest.mark.parametrize("n,m,N,bt", [(4, 2, 50, 70), (32, 16, 40, 3)])   # native SoA lane kernel; staged
def test_dp_cross_layout1(lqrx, gpu_ok, n, m, N, bt):
    """Layout 1 (SoA), M included: bit-identical to layout 0.  Per-knot M."""
    d = cross_problem(lqrx, n, m, N, bt, 177 + n, tv_QR=True, tv_AB=True)
    b = to_batch(d, N)
    a0 = lqrx.solve_batch(b, all_P=True, layout=0)
    a1 = lqrx.solve_batch(b, all_P=True, layout=1)
    assert (a0["info"] == 0).all() and np.abs(a0["K"]).max() > 0
    for k in ("K", "P", "X", "U", "d", "p", "info"):
        assert np.array_equal(a0[k], a1[k]), k


def test_dp_cross_device_stream(lqrx, gpu_ok):
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
        out = lqrx.dp_solve_device(t, N, p_mode=1, stream=s.cuda_stream)
    s.synchronize()
    got = logical({k: out[k].cpu().numpy() for k in ("K", "P", "X", "U", "d", "p", "info")}, n, m, N, bt, True)
    ref = logical(dp_solve_abi_np(d, N, "cross", all_P=True), n, m, N, bt, True)
    check(got, ref, True, TOL64, "stream")


def test_dp_cross_info_matches_checker(lqrx, gpu_ok):
    """R negated at one trajectory: info equals the checker's (the first knot whose E has a
    non-positive eigenvalue) and is 0 at the other trajectories."""
    from lqrx.dp import from_abi, to_abi

    n, m, N, bt = 6, 3, 12, 4
    d = cross_problem(lqrx, n, m, N, bt, 4242)
    R = from_abi(d["R"], (bt, m, m)).copy()
    R[2] = -R[2]
    d["R"] = to_abi(R).ravel()
    a = lqrx.solve_batch(to_batch(d, N))
    ref = dp_solve_abi_np(d, N, "cross")
    print("info", a["info"], ref["info"])
    assert ref["info"][2] != 0 and (np.delete(ref["info"], 2) == 0).all()
    assert np.array_equal(a["info"], ref["info"])


def test_dp_cross_single_problem_api(lqrx, gpu_ok):
    """LQRProblem(M=…) with no c and no cost vectors → solve(sol, DPSolver, prob): c, q, r, qf are
    filled with zeros, sol.d and sol.p come back beside K, X, U, P."""
    from lqrx.dp import DPSolver, LQRProblem, LQRSolution, from_abi

    n, m, N = 6, 2, 30
    d = cross_problem(lqrx, n, m, N, 1, 2025)
    for k in ("q", "r", "qf", "c"):
        d[k] = np.zeros_like(d[k])
    prob = LQRProblem(Qf=from_abi(d["Qf"], (1, n, n))[0], Q=from_abi(d["Q"], (1, n, n))[0],
                      R=from_abi(d["R"], (1, m, m))[0], A=from_abi(d["A"], (1, n, n))[0],
                      B=from_abi(d["B"], (1, n, m))[0], x0=d["x0"].copy(), N=N,
                      M=from_abi(d["M"], (1, m, n))[0])
    sol = LQRSolution.of(prob, all_P=True)
    lqrx.solve(sol, DPSolver.of(prob), prob)
    got = dict(K=sol.K[None], P=sol.P[None], X=sol.X[None], U=sol.U[None], d=sol.d[None], p=sol.p[None],
               info=np.array([sol.info]))
    ref = logical(dp_solve_abi_np(d, N, "cross", all_P=True), n, m, N, 1, True)
    check(got, ref, True, TOL64, "single")
