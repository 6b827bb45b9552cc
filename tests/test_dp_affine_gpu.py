"""GPU parity: DP with affine dynamics x⁺ = A x + B u + c (lqrx_dp_solve_affine).

Checker: tests/dp_truth.py (numpy float64; pinned to the dense QP and to the committed
oracle in tests/test_dp_affine.py).  Independently of it, the shift identity below compares
against oracle.dp_solve_abi alone.  Tolerances are those of tests/test_dp_linear_gpu.py,
measured the same way: fp64 1e-10, fp32 1e-4; K and P per knot, d, p, X, U on their
trajectory's scale.  (A float32 numpy recursion against float64 at these shapes stays at or
below 8e-6 on that scale, so the fp32 bound leaves the kernels more than a decade.)
Kernels: n ≤ 4 dp_lane_kernel<…, LIN, AFF> (always — never dp_quad_kernel), n ≥ 5
dp_riccati_kernel<…, VAR_LIN | VAR_AFF [| VAR_TV]> (fp64 n = 64 too — never dp_wg4_kernel),
past the register tiles dp_big_kernel.
"""
import numpy as np
import pytest

from dp_truth import PARITY, affine_problem, check, dp_solve_abi_np, logical, to_batch

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL32 = 1e-4


@pytest.mark.parametrize("n,m,N,bt,tvq,tvab,all_P", PARITY)
def test_dp_affine_parity_f64(lqrx, gpu_ok, n, m, N, bt, tvq, tvab, all_P):
    d = affine_problem(lqrx, n, m, N, bt, 5100 + 11 * n + m, tvq, tvab)
    got = lqrx.solve_batch(to_batch(d, N), all_P=all_P)
    assert got["rc"] == 0
    ref = logical(dp_solve_abi_np(d, N, "affine", all_P=all_P), n, m, N, bt, all_P)
    check(got, ref, all_P, TOL64, f"f64 {n},{m},{N},{bt}")


@pytest.mark.parametrize("n,m,N,bt,tv", [(6, 3, 30, 7, False), (32, 16, 40, 3, True), (64, 32, 12, 2, False)])
def test_dp_affine_parity_f32(lqrx, gpu_ok, n, m, N, bt, tv):
    d = affine_problem(lqrx, n, m, N, bt, 700 + n, tv, tv)
    got = lqrx.solve_batch(to_batch(d, N), dtype=1, all_P=True)
    ref = logical(dp_solve_abi_np(d, N, "affine", all_P=True), n, m, N, bt, True)
    check(got, ref, True, TOL32, f"f32 {n},{m},{N},{bt}")


@pytest.mark.parametrize("n,m,N,bt", [(4, 2, 30, 5), (6, 3, 30, 7), (32, 16, 40, 3)])
def test_dp_affine_shift_identity(lqrx, oracle, gpu_ok, n, m, N, bt):
    """x = x̃ + s, u = ũ + t turns the plain problem (A, B, Q, R, Qf, x̃0) into the affine one
    with c = s − As − Bt, q = −Qs, r = −Rt, qf = −Qf s, x0 = x̃0 + s: K and P are the plain
    ones, X − s = X̃, U − t = Ũ, d_k = −(K_k s + t), p_k = −P_k s.  Reference: the committed
    oracle's plain solve only."""
    from lqrx.dp import from_abi

    d = lqrx.random_batch(n, m, N, bt, 8800 + n)
    rng = np.random.default_rng(n * 31 + m)
    s = rng.standard_normal((bt, n))
    t = rng.standard_normal((bt, m))
    A = from_abi(d["A"], (bt, n, n)); B = from_abi(d["B"], (bt, n, m))
    Q = from_abi(d["Q"], (bt, n, n)); R = from_abi(d["R"], (bt, m, m)); Qf = from_abi(d["Qf"], (bt, n, n))
    mv = lambda M, v: np.einsum("bij,bj->bi", M, v)
    da = dict(d)
    da["c"] = (s - mv(A, s) - mv(B, t)).ravel()
    da["q"] = (-mv(Q, s)).ravel()
    da["r"] = (-mv(R, t)).ravel()
    da["qf"] = (-mv(Qf, s)).ravel()
    da["x0"] = (d["x0"].reshape(bt, n) + s).ravel()
    got = lqrx.solve_batch(to_batch(da, N), all_P=True)
    assert got["rc"] == 0
    plain = oracle.dp_solve_abi(d, N, all_P=True)
    K = from_abi(plain["K"], (bt, N - 1, m, n)); P = from_abi(plain["P"], (bt, N, n, n))
    ref = dict(K=K, P=P, X=plain["X"].reshape(bt, N, n) + s[:, None], U=plain["U"].reshape(bt, N - 1, m) + t[:, None],
               d=-(np.einsum("bkij,bj->bki", K, s) + t[:, None]), p=-np.einsum("bkij,bj->bki", P, s),
               info=plain["info"])
    check(got, ref, True, TOL64, f"shift {n},{m},{N},{bt}")


@pytest.mark.parametrize("n,m,N,bt", [(4, 1, 30, 5), (32, 16, 40, 3)])
def test_dp_affine_zero_offset_equals_linear(lqrx, gpu_ok, n, m, N, bt):
    """c = 0: the results of lqrx_dp_solve_linear on the same data."""
    d = affine_problem(lqrx, n, m, N, bt, 19 + n)
    d["c"] = np.zeros_like(d["c"])
    a = lqrx.solve_batch(to_batch(d, N), all_P=True)
    ref = lqrx.solve_batch(to_batch(d, N, fields=("q", "r", "qf")), all_P=True)
    check(a, ref, True, TOL64, f"c=0 {n},{m},{N},{bt}")


@pytest.mark.parametrize("n,m,N,bt", [(4, 2, 50, 70), (32, 16, 40, 3)])   # native SoA lane kernel; staged
def test_dp_affine_layout1(lqrx, gpu_ok, n, m, N, bt):
    """Layout 1 (SoA), c included: bit-identical to layout 0.  Per-knot c."""
    d = affine_problem(lqrx, n, m, N, bt, 177 + n, tv_QR=True, tv_AB=True)
    b = to_batch(d, N)
    a0 = lqrx.solve_batch(b, all_P=True, layout=0)
    a1 = lqrx.solve_batch(b, all_P=True, layout=1)
    for k in ("K", "P", "X", "U", "d", "p", "info"):
        assert np.array_equal(a0[k], a1[k]), k


def test_dp_affine_device_stream(lqrx, gpu_ok):
    """Device-pointer entry on a created stream, synchronised before checking."""
    import torch

    n, m, N, bt = 32, 16, 40, 4
    d = affine_problem(lqrx, n, m, N, bt, 321)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.asarray(d[k])).to(dev)
         for k in ("A", "B", "Q", "R", "Qf", "x0", "q", "r", "qf", "c")}
    t.update(n=n, m=m, batch=bt)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = lqrx.dp_solve_device(t, N, p_mode=1, stream=s.cuda_stream)
    s.synchronize()
    got = logical({k: out[k].cpu().numpy() for k in ("K", "P", "X", "U", "d", "p", "info")}, n, m, N, bt, True)
    ref = logical(dp_solve_abi_np(d, N, "affine", all_P=True), n, m, N, bt, True)
    check(got, ref, True, TOL64, "stream")


def test_dp_affine_info_matches_linear(lqrx, gpu_ok):
    """A non-SPD R at one trajectory: info names the same knot as lqrx_dp_solve_linear."""
    from lqrx.dp import from_abi, to_abi

    n, m, N, bt = 6, 3, 12, 4
    d = affine_problem(lqrx, n, m, N, bt, 4242)
    R = from_abi(d["R"], (bt, m, m)).copy()
    R[2] = -R[2]
    d["R"] = to_abi(R).ravel()
    a = lqrx.solve_batch(to_batch(d, N))
    ref = lqrx.solve_batch(to_batch(d, N, fields=("q", "r", "qf")))
    assert ref["info"][2] != 0 and (np.delete(ref["info"], 2) == 0).all()
    assert np.array_equal(a["info"], ref["info"])


def test_dp_affine_single_problem_api(lqrx, gpu_ok):
    """LQRProblem(c=…) without cost terms → solve(sol, DPSolver, prob): q, r, qf are filled with
    zeros, sol.d and sol.p come back beside K, X, U, P."""
    from lqrx.dp import DPSolver, LQRProblem, LQRSolution, from_abi

    n, m, N = 6, 2, 30
    d = affine_problem(lqrx, n, m, N, 1, 2025)
    for k in ("q", "r", "qf"):
        d[k] = np.zeros_like(d[k])
    prob = LQRProblem(Qf=from_abi(d["Qf"], (1, n, n))[0], Q=from_abi(d["Q"], (1, n, n))[0],
                      R=from_abi(d["R"], (1, m, m))[0], A=from_abi(d["A"], (1, n, n))[0],
                      B=from_abi(d["B"], (1, n, m))[0], x0=d["x0"].copy(), N=N, c=d["c"].copy())
    sol = LQRSolution.of(prob, all_P=True)
    lqrx.solve(sol, DPSolver.of(prob), prob)
    got = dict(K=sol.K[None], P=sol.P[None], X=sol.X[None], U=sol.U[None], d=sol.d[None], p=sol.p[None],
               info=np.array([sol.info]))
    ref = logical(dp_solve_abi_np(d, N, "affine", all_P=True), n, m, N, 1, True)
    check(got, ref, True, TOL64, "single")
