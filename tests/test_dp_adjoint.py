"""CPU tests of the costates and the adjoint pass (no GPU needed).

The two checkers of tests/dp_adjoint_truth.py against each other — (b) the numpy restatement of
the recursion the kernels implement, (a) torch float64 autograd through the dense KKT solve — at
the shapes the GPU tests use, the sign of λ against dense_kkt, the stationarity residual, a
central finite difference of the loss, and the argument checks of lqrx_dp_costates[_host] and
lqrx_dp_solve_adjoint, which are decided before the device is touched.

Bounds: the project's TOL64 = 1e-10 / TOL32 = 1e-4 on the trajectory's scale for λ and the vector
gradients, 4·TOL on the scale of their two terms for the matrix gradients (dp_adjoint_truth.grad_errors).
Observed on the CPU: float64 worst 4.4e-14, float32 worst 3.8e-6 of the array's largest entry.
"""
import ctypes as C

import numpy as np
import pytest

from dp_adjoint_truth import (FIELDS, adjoint_abi, check_grads, dense_adjoint_truth, per_knot_problem,
                              sum_truth_like)
from dp_truth import cross_problem, dense_kkt

TOL64 = 1e-10
TOL32 = 1e-4
SHAPES = [(2, 1, 2), (4, 2, 6), (5, 2, 5), (16, 16, 4), (17, 3, 4), (33, 17, 3), (64, 32, 3), (65, 33, 3),
          (6, 3, 30), (32, 16, 40)]


def problem(lqrx, n, m, N, bt, seed, tv_AB):
    d = cross_problem(lqrx, n, m, N, bt, seed, tv_QR=True, tv_AB=bool(tv_AB))
    d["tv_QR"], d["tv_AB"] = 1, int(bool(tv_AB))   # N = 2 has one knot: the flags still say per knot
    rng = np.random.default_rng(seed + 99)
    return d, rng.standard_normal((bt, N, n)), rng.standard_normal((bt, N - 1, m))


def truth_of(d, N, gX, gU, b):
    """Checker (a) at trajectory b, in the shapes adjoint_abi returns (one trajectory)."""
    ta = dense_adjoint_truth(per_knot_problem(d, N, b), N, gX[b], gU[b])
    return ta, sum_truth_like(ta["g"], d)


@pytest.mark.parametrize("n,m,N", SHAPES)
@pytest.mark.parametrize("dtype,tol", [(np.float64, TOL64), (np.float32, TOL32)])
def test_recursion_matches_dense_autograd(lqrx, n, m, N, dtype, tol):
    """(b) against (a): λ and all eleven gradients, both knot strides of A."""
    seeds = (1, 2, 3) if N * (2 * n + m) <= 1000 else (1,)
    for seed in seeds:
        tv_AB = seed % 2
        d, gX, gU = problem(lqrx, n, m, N, 2, 4000 + 31 * n + seed, tv_AB)
        ref = adjoint_abi(d, N, gX, gU)
        got = ref if dtype is np.float64 else adjoint_abi(d, N, gX, gU, dtype=np.float32)
        assert (ref["info"] == 0).all() and (ref["info_adj"] == 0).all()
        for b in range(2):
            ta, ga = truth_of(d, N, gX, gU, b)
            # (a) in the place of the kernels' output, (b) float64 as the scale-giving reference
            one = lambda r: dict(X=r["X"][b:b + 1], U=r["U"][b:b + 1], lam=r["lam"][b:b + 1], Xa=r["Xa"][b:b + 1],
                                 Ua=r["Ua"][b:b + 1], lama=r["lama"][b:b + 1],
                                 g={k: v[b:b + 1] for k, v in r["g"].items()})
            truth = one(ref)
            truth["lam"] = ta["lam"][None]
            truth["g"] = {k: ga[k][None] for k in FIELDS}
            mine = {k: got["g"][k][b:b + 1] for k in FIELDS}
            mine["lam"] = got["lam"][b:b + 1]
            check_grads(mine, truth, tol, f"{dtype.__name__} {n},{m},{N} seed {seed} traj {b}")


@pytest.mark.parametrize("n,m,N", [(5, 2, 6), (2, 1, 4), (3, 2, 2)])
def test_costate_sign_and_stationarity(lqrx, n, m, N):
    """λ of (a) is −lam of dense_kkt; R u + M x + r + Bᵀλ_{k+1} = 0 with (b)'s λ; x'_1 = 0."""
    d, gX, gU = problem(lqrx, n, m, N, 2, 77 + n, 1)
    ref = adjoint_abi(d, N, gX, gU)
    for b in range(2):
        p = per_knot_problem(d, N, b)
        X, U, lam = dense_kkt(p["A"], p["B"], p["c"], p["Q"], p["R"], p["M"], p["Qf"], p["x0"], N,
                                    p["q"], p["r"], p["qf"])
        ta = dense_adjoint_truth(p, N, gX[b], gU[b])
        assert np.abs(ta["lam"] + lam).max() <= TOL64 * np.abs(lam).max()
        assert np.abs(ref["lam"][b] + lam).max() <= TOL64 * np.abs(lam).max()
        for k in range(N - 1):
            terms = [p["R"][k] @ ref["U"][b, k], p["M"][k] @ ref["X"][b, k], p["r"][k], p["B"][k].T @ ref["lam"][b, k + 1]]
            scale = sum(np.abs(t).max() for t in terms)
            assert np.abs(sum(terms)).max() <= TOL64 * scale, k
    assert (ref["Xa"][:, 0] == 0).all() and (ref["g"]["q"][:, 0] == 0).all() and (ref["g"]["Q"][:, 0] == 0).all()


def test_long_horizon_needs_the_closed_loop_sweep(lqrx):
    """n = 32, m = 16, N = 256, per-knot A with ρ(A) ≈ 1.14: (b)'s closed-loop sweep equals
    P_k x_k + p_k of the checker's own Riccati pass to TOL64 on the trajectory's scale (observed
    2.7e-15); the textbook open-loop sweep on the same X, U, equal in exact arithmetic, does not
    (observed 1.9e-5: ρ^(N−1) ≈ 2e14 times the rounding of X, U) — which is why the library and the
    checker add K_kᵀ·(stationarity)."""
    from dp_adjoint_truth import costates_textbook
    from dp_truth import _mats, dp_solve_abi_np

    n, m, N, bt = 32, 16, 256, 2
    d, gX, gU = problem(lqrx, n, m, N, bt, 6100 + 13 * n + m, 1)
    ref = adjoint_abi(d, N, gX, gU)
    full = dp_solve_abi_np(d, N, "cross", all_P=True)
    P, p = _mats(full["P"], bt, N, n, n, np.float64), full["p"].reshape(bt, N, n)
    lamP = (P @ ref["X"][..., None])[..., 0] + p
    mx = lambda a: np.abs(a).reshape(bt, -1).max(axis=1)
    e = (mx(ref["lam"] - lamP) / mx(lamP)).max()
    mats = lambda k, r, c: _mats(d[k], bt, N - 1, r, c, np.float64)
    text = costates_textbook(mats("A", n, n), mats("Q", n, n), mats("M", m, n), _mats(d["Qf"], bt, 1, n, n, np.float64)[:, 0],
                             d["q"].reshape(bt, N - 1, n), d["qf"].reshape(bt, n), ref["X"], ref["U"])
    et = (mx(text - lamP) / mx(lamP)).max()
    print("closed loop", e, "textbook", et)
    assert e <= TOL64
    assert et > 1e3 * TOL64   # the reason, pinned: if this ever holds no longer, the simpler sweep would do


def test_finite_difference_of_the_loss(lqrx):
    """ℓ(θ + εδ) − ℓ(θ − εδ) over 2ε against Σ ⟨gradient, δ⟩ in three random directions, symmetric
    in Q, R, Qf; ℓ from dense_kkt (numpy).  ε = 1e-6: the truncation error is O(ε²) = 1e-12 and
    the rounding error of ℓ about 1e-16·cond/ε ≈ 1e-10·cond relative, so 1e-6 of the sum of the terms'
    magnitudes holds with a wide margin for these well-conditioned problems."""
    n, m, N = 4, 2, 6
    d, gX, gU = problem(lqrx, n, m, N, 1, 909, 1)
    p = per_knot_problem(d, N, 0)
    g = adjoint_abi(d, N, gX, gU)["g"]

    def loss(q):
        X, U, _ = dense_kkt(q["A"], q["B"], q["c"], q["Q"], q["R"], q["M"], q["Qf"], q["x0"], N, q["q"],
                                  q["r"], q["qf"])
        return (X * gX[0]).sum() + (U * gU[0]).sum()

    rng = np.random.default_rng(5)
    eps = 1e-6
    for _ in range(3):
        dl = {k: rng.standard_normal(p[k].shape) for k in FIELDS}
        for k in ("Q", "R", "Qf"):
            dl[k] = 0.5 * (dl[k] + np.swapaxes(dl[k], -1, -2))
        fd = (loss({k: p[k] + eps * dl[k] for k in FIELDS}) - loss({k: p[k] - eps * dl[k] for k in FIELDS})) / (2 * eps)
        terms = [float((g[k][0] * dl[k]).sum()) for k in FIELDS]
        print("fd", fd, "adjoint", sum(terms))
        assert abs(fd - sum(terms)) <= 1e-6 * sum(abs(t) for t in terms)


# ---- ABI argument checks: every code is decided before the device is touched ----

def _desc(lqrx, **kw):
    from lqrx import _lib

    f = dict(n=3, m=2, N=4, dtype=0, batch=2, layout=0, p_mode=0, knot_stride_AB=1, knot_stride_QR=1)
    f.update(kw)
    return _lib.DpDesc(f["n"], f["m"], f["N"], f["dtype"], f["batch"], f["layout"], f["p_mode"],
                       f["knot_stride_AB"], f["knot_stride_QR"])


@pytest.fixture(scope="module")
def buf():
    return np.zeros(4096)


def _p(buf):
    return C.c_void_p(buf.ctypes.data)


@pytest.mark.parametrize("host", [False, True])
def test_costates_argument_codes(lqrx, buf, host):
    lib = lqrx.load()
    fn = lib.lqrx_dp_costates_host if host else lib.lqrx_dp_costates
    tail = () if host else (None,)
    ok = [_p(buf)] * 13   # A B Q R M Qf q r qf K X U lam
    assert fn(None, *ok, *tail) == -1
    # M (6), q (8), r (9), qf (10) may be NULL: with them NULL too the first complaint is the required one
    for pos in (0, 1, 2, 3, 5, 9, 10, 11, 12):
        a = list(ok)
        a[4] = a[6] = a[7] = a[8] = None
        a[pos] = None
        assert fn(C.byref(_desc(lqrx)), *a, *tail) == -(pos + 2), pos
    assert fn(C.byref(_desc(lqrx, layout=1)), *ok, *tail) == -101
    assert b"layout" in lib.lqrx_last_error()
    assert fn(C.byref(_desc(lqrx, p_mode=1)), *([None] * 13), *tail) == -2      # p_mode is ignored
    assert fn(C.byref(_desc(lqrx, n=0)), *ok, *tail) == -1
    assert fn(C.byref(_desc(lqrx, batch=0)), *([None] * 13), *tail) == 0
    assert fn(C.byref(_desc(lqrx, batch=0, knot_stride_QR=0, knot_stride_AB=0)), *([None] * 13), *tail) == 0


def test_adjoint_argument_codes(lqrx, buf):
    from lqrx import _lib

    lib = lqrx.load()
    fn = lib.lqrx_dp_solve_adjoint
    ok = [_p(buf)] * 9   # A B Q R M Qf X U lam
    g = _lib.DpGrad(buf.ctypes.data, buf.ctypes.data, *([None] * 11))
    assert fn(None, *ok, C.byref(g), None, None) == -1
    for pos in range(9):
        a = list(ok)
        a[pos] = None
        assert fn(C.byref(_desc(lqrx)), *a, C.byref(g), None, None) == -(pos + 2), pos
    assert fn(C.byref(_desc(lqrx)), *ok, None, None, None) == -11
    assert fn(C.byref(_desc(lqrx)), *ok, C.byref(_lib.DpGrad(None, buf.ctypes.data, *([None] * 11))), None, None) == -11
    assert fn(C.byref(_desc(lqrx)), *ok, C.byref(_lib.DpGrad(buf.ctypes.data, None, *([None] * 11))), None, None) == -11
    assert fn(C.byref(_desc(lqrx, layout=1)), *ok, C.byref(g), None, None) == -101
    assert b"layout" in lib.lqrx_last_error()
    assert fn(C.byref(_desc(lqrx, knot_stride_QR=0)), *ok, C.byref(g), None, None) == -101
    assert b"broadcast" in lib.lqrx_last_error()
    assert fn(C.byref(_desc(lqrx, batch=0)), *([None] * 9), None, None, None) == 0
    assert fn(C.byref(_desc(lqrx, N=1)), *ok, C.byref(g), None, None) == -1


def test_python_surface(lqrx):
    """The new names are exported, and the struct mirrors the header's field order."""
    from lqrx import _lib

    assert callable(lqrx.lqr_solve) and callable(lqrx.dp_adjoint_device)
    assert [f[0] for f in _lib.DpGrad._fields_] == ["gX", "gU", "gA", "gB", "gc", "gQ", "gR", "gM", "gQf", "gx0",
                                                   "gq", "gr", "gqf"]
    names = _lib.header_functions()
    for nm in ("lqrx_dp_costates", "lqrx_dp_costates_host", "lqrx_dp_solve_adjoint"):
        assert nm in names and hasattr(lqrx.load(), nm)
    assert "lqrx_dp_solve_adjoint_host" not in names
    sol = lqrx.LQRSolution.of(lqrx.LQRProblem(Qf=np.eye(2), Q=np.eye(2), R=np.eye(1), A=np.eye(2),
                                              B=np.ones((2, 1)), x0=np.ones(2), N=3), costates=True)
    assert sol.lam.shape == (3, 2)
