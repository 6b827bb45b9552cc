"""Checker for lqrx_dp_resolve_box (include/lqrx.h): the ADMM iteration for input bounds in numpy on
dp_resolve_truth.resolve_np, an independent truth for the constrained optimum (the QP condensed over U,
solved by scipy's BVLS), and a reference-free optimality measure.  Not a test file; pinned in
tests/test_dp_box.py.

Per problem b and instance j (trajectory t = b·S + j), with the factors K, E⁻¹, Pc of a solve made with
R + ρI, iteration i = 1 … max_iter:

    r̂_k  = r_{t,k} − ρ (z_k − w_k)
    (d, X, U) = resolve_np on (q_t, r̂, qf_t, x0_t)
    û_k  = α u_k + (1 − α) z_k
    z⁺_k = min(max(û_k + w_k, u_lo_b), u_hi_b)
    w⁺_k = w_k + û_k − z⁺_k
    r_prim = max_k ‖u_k − z⁺_k‖∞      r_dual = ρ · max_k ‖z⁺_k − z_k‖∞

An instance stops after the first iteration with r_prim ≤ eps_prim and r_dual ≤ eps_dual (both eps > 0: an
eps of 0 never stops early; a NaN residual fails the test) and is left alone from then on.
"""
import numpy as np

from dp_resolve_truth import factor_np, resolve_np
from dp_truth import _mats, dp_solve_abi_np

# (n, m, N, batch, tv): dp_resolve_truth.SHAPES without the full-horizon one
SHAPES = [(1, 1, 6, 3, False), (4, 1, 40, 8, False), (6, 3, 30, 7, False), (17, 5, 12, 3, True),
          (32, 16, 40, 4, False), (24, 18, 10, 3, False), (64, 32, 12, 2, False), (48, 16, 10, 2, True)]
# The shapes of the BVLS truth at ρ = 1.  The rate of ADMM at a fixed ρ depends on the plant: of the seven plants
# of cross_problem(6, 3, 30, 7, seed 3) the first five and the last stop at 1e-10 within 49 – 802 iterations at
# ρ = 1, while plant 5 is still 0.2 away from the truth after 3000 (it stops after 1580 at ρ = 10, where the
# others need 82 – 120).  The ρ = 1 cases therefore take the first five plants, and SLOW_PLANT, all seven at
# ρ = 10, keeps plant 5 under the same truth.
TRUTH_SHAPES = [(4, 1, 40, 8, False), (6, 3, 30, 5, False), (17, 5, 12, 3, True)]
SLOW_PLANT = ((6, 3, 30, 7, False), 10.0)
__all__ = ["SHAPES", "TRUTH_SHAPES", "SLOW_PLANT", "with_rho", "factors_np", "box_np", "half_peak_bounds", "own_rhs",
           "bvls_truth", "natural_residual", "active_share"]


def with_rho(d: dict, rho: float) -> dict:
    """the flat ABI problem d with R + ρI on every stored R knot"""
    m = d["m"]
    R = np.asarray(d["R"], np.float64).reshape(-1, m, m) + rho * np.eye(m)
    return dict(d, R=R.ravel())


def factors_np(d: dict, N: int, rho: float) -> dict:
    """K, Einv, Pc (flat ABI, float64) of the cross solve of d with R + ρI"""
    dr = with_rho(d, rho)
    ref = dp_solve_abi_np(dr, N, "cross", all_P=True)
    fac = factor_np(dr, N, ref["P"])
    assert (ref["info"] == 0).all() and (fac["info"] == 0).all()
    return dict(K=ref["K"], Einv=fac["Einv"], Pc=fac["Pc"])


def own_rhs(d: dict, N: int) -> dict:
    """the problem's own q, r, qf, x0 as one instance per problem (S = 1; the knot axis of q, r follows tv_QR)"""
    return {k: np.asarray(d[k], np.float64) for k in ("q", "r", "qf", "x0")}


def box_np(d: dict, N: int, K, Einv, Pc, S: int, q=None, r=None, qf=None, x0=None, tv_QR: int = 0, u_lo=None,
           u_hi=None, rho: float = 1.0, relax: float = 1.6, eps_prim: float = 1e-6, eps_dual: float = 1e-6,
           max_iter: int = 500, Z=None, W=None, dtype=np.float64) -> dict:
    """d, K, Einv, Pc, q, r, qf, x0, tv_QR as in resolve_np (the factors those of R + ρI).  u_lo, u_hi: m per
    problem (flat) or None.  Z, W: m·(N−1) per instance (flat or logical) or None for zeros; not modified.
    Returns logical d, U, Z, W (bt, S, N−1, m), X (bt, S, N, n), iters (bt, S) and res (bt, S, 2), every operation
    in `dtype`."""
    n, m, bt = d["n"], d["m"], d["batch"]
    dt = dtype
    kq = N - 1 if tv_QR else 1
    knots = lambda a, w: np.ascontiguousarray(np.broadcast_to(
        np.zeros((bt, S, 1, w), dt) if a is None else np.asarray(a, dt).reshape(bt, S, kq, w), (bt, S, N - 1, w)))
    qv, rv = knots(q, n), knots(r, m)
    lo = np.full((bt, 1, 1, m), -np.inf, dt) if u_lo is None else np.asarray(u_lo, dt).reshape(bt, 1, 1, m)
    hi = np.full((bt, 1, 1, m), np.inf, dt) if u_hi is None else np.asarray(u_hi, dt).reshape(bt, 1, 1, m)
    start = lambda a: np.zeros((bt, S, N - 1, m), dt) if a is None else np.array(a, dt).reshape(bt, S, N - 1, m)
    Z, W = start(Z), start(W)
    rho_, al = dt(rho), dt(relax)
    om = dt(1) - al
    eps_p, eps_d = dt(eps_prim), dt(eps_dual)
    stops = eps_prim > 0 and eps_dual > 0
    dd, U, X = np.zeros((bt, S, N - 1, m), dt), np.zeros((bt, S, N - 1, m), dt), np.zeros((bt, S, N, n), dt)
    iters = np.zeros((bt, S), np.int32)
    res = np.zeros((bt, S, 2), dt)
    active = np.ones((bt, S), bool)
    for it in range(int(max_iter)):
        rhat = rv - rho_ * (Z - W)
        s = resolve_np(d, N, K, Einv, Pc, S, q=qv.ravel(), r=rhat.ravel(), qf=qf, x0=x0, tv_QR=1, dtype=dt)
        u = s["U"]
        uh = al * u + om * Z
        v = uh + W
        zp = np.where(v < lo, lo, v)          # compares, as in the kernel: a NaN passes through
        zp = np.where(zp > hi, hi, zp)
        wp = W + uh - zp
        with np.errstate(invalid="ignore"):
            rp = np.abs(u - zp).max(axis=(2, 3))
            rd = rho_ * np.abs(zp - Z).max(axis=(2, 3))
            conv = stops & (rp <= eps_p) & (rd <= eps_d)
        a4 = active[:, :, None, None]
        Z, W = np.where(a4, zp, Z), np.where(a4, wp, W)
        dd, U, X = np.where(a4, s["d"], dd), np.where(a4, u, U), np.where(a4, s["X"], X)
        iters[active] = it + 1
        res[active, 0], res[active, 1] = rp[active], rd[active]
        active = active & ~conv
        if not active.any():
            break
    return dict(d=dd, X=X, U=U, Z=Z, W=W, iters=iters, res=res)


def half_peak_bounds(U_unc, bt: int, m: int, share: float = 0.5):
    """±share·max|U_unconstrained| per problem, the lower side of input 0 left unbounded: (u_lo, u_hi), (bt, m)"""
    peak = np.abs(np.asarray(U_unc, np.float64).reshape(bt, -1)).max(axis=1)
    hi = np.repeat(share * peak[:, None], m, axis=1)
    lo = -hi.copy()
    lo[:, 0] = -np.inf
    return lo, hi


def _logical(d: dict, N: int):
    n, m, bt = d["n"], d["m"], d["batch"]
    kab = N - 1 if d.get("tv_AB") else 1
    kqr = N - 1 if d.get("tv_QR") else 1
    f8 = np.float64
    per = lambda a, k: np.broadcast_to(a, (bt, N - 1) + a.shape[2:]) if k == 1 else a
    A, B = per(_mats(d["A"], bt, kab, n, n, f8), kab), per(_mats(d["B"], bt, kab, n, m, f8), kab)
    c = per(np.asarray(d["c"], f8).reshape(bt, kab, n), kab) if d.get("c") is not None else np.zeros((bt, N - 1, n))
    Q, R = per(_mats(d["Q"], bt, kqr, n, n, f8), kqr), per(_mats(d["R"], bt, kqr, m, m, f8), kqr)
    M = per(_mats(d["M"], bt, kqr, m, n, f8), kqr) if d.get("M") is not None else np.zeros((bt, N - 1, m, n))
    Qf = _mats(d["Qf"], bt, 1, n, n, f8)[:, 0]
    return A, B, c, Q, R, M, Qf


def _rhs_logical(d, N, S, q, r, qf, x0, tv_QR):
    n, m, bt = d["n"], d["m"], d["batch"]
    kq = N - 1 if tv_QR else 1
    vec = lambda a, k, w: np.zeros((bt, S, k, w)) if a is None else np.asarray(a, np.float64).reshape(bt, S, k, w)
    q = np.broadcast_to(vec(q, kq, n), (bt, S, N - 1, n))
    r = np.broadcast_to(vec(r, kq, m), (bt, S, N - 1, m))
    return q, r, vec(qf, 1, n)[:, :, 0], vec(x0, 1, n)[:, :, 0]


def bvls_truth(d: dict, N: int, S: int, u_lo, u_hi, q=None, r=None, qf=None, x0=None, tv_QR: int = 0):
    """The constrained optimum U (bt, S, N−1, m) in float64, independent of the Riccati recursion: with
    x_k = G_k U + o_k from the dynamics, the cost is ½UᵀHU + gᵀU + const; H = LLᵀ, and
    min ½‖LᵀU + L⁻¹g‖² under the bounds is solved by scipy.optimize.lsq_linear(method="bvls")."""
    from scipy.linalg import cholesky, solve_triangular
    from scipy.optimize import lsq_linear

    n, m, bt = d["n"], d["m"], d["batch"]
    A, B, c, Q, R, M, Qf = _logical(d, N)
    q, r, qf, x0 = _rhs_logical(d, N, S, q, r, qf, x0, tv_QR)
    nu = (N - 1) * m
    lo = np.full((bt, m), -np.inf) if u_lo is None else np.asarray(u_lo, np.float64).reshape(bt, m)
    hi = np.full((bt, m), np.inf) if u_hi is None else np.asarray(u_hi, np.float64).reshape(bt, m)
    out = np.zeros((bt, S, N - 1, m))
    for b in range(bt):
        # x_k = G[k] U + (F[k] x0 + o[k]): G, F and o do not depend on the instance
        G, F, o = [np.zeros((n, nu))], [np.eye(n)], [np.zeros(n)]
        for k in range(N - 1):
            Gn = A[b, k] @ G[k]
            Gn[:, k * m:(k + 1) * m] += B[b, k]
            G.append(Gn), F.append(A[b, k] @ F[k]), o.append(A[b, k] @ o[k] + c[b, k])
        H = G[N - 1].T @ Qf[b] @ G[N - 1]
        for k in range(N - 1):
            Sk = np.zeros((m, nu))
            Sk[:, k * m:(k + 1) * m] = np.eye(m)
            MG = Sk.T @ M[b, k] @ G[k]
            H += G[k].T @ Q[b, k] @ G[k] + MG + MG.T + Sk.T @ R[b, k] @ Sk
        H = (H + H.T) / 2
        L = cholesky(H, lower=True)
        for j in range(S):
            xo = [F[k] @ x0[b, j] + o[k] for k in range(N)]
            g = G[N - 1].T @ (Qf[b] @ xo[N - 1] + qf[b, j])
            for k in range(N - 1):
                g += G[k].T @ (Q[b, k] @ xo[k] + q[b, j, k])
                g[k * m:(k + 1) * m] += M[b, k] @ xo[k] + r[b, j, k]
            rhs = -solve_triangular(L, g, lower=True)
            sol = lsq_linear(L.T, rhs, bounds=(np.tile(lo[b], N - 1), np.tile(hi[b], N - 1)), method="bvls", tol=1e-14,
                             max_iter=20 * nu)
            assert sol.status > 0, sol.message
            out[b, j] = sol.x.reshape(N - 1, m)
    return out


def natural_residual(d: dict, N: int, S: int, Z, u_lo, u_hi, q=None, r=None, qf=None, x0=None, tv_QR: int = 0):
    """Reference-free optimality of Z (bt, S, N−1, m) in float64: X rolled out from Z, the costates
    λ_N = Qf x_N + qf, λ_k = Q x_k + Mᵀu_k + q + Aᵀλ_{k+1}, the gradient g_k = R u_k + M x_k + r + Bᵀλ_{k+1}.
    Returns (‖Z − clip(Z − g, lo, hi)‖∞ per instance (bt, S), g (bt, S, N−1, m))."""
    n, m, bt = d["n"], d["m"], d["batch"]
    A, B, c, Q, R, M, Qf = _logical(d, N)
    q, r, qf, x0 = _rhs_logical(d, N, S, q, r, qf, x0, tv_QR)
    Z = np.asarray(Z, np.float64).reshape(bt, S, N - 1, m)
    lo = np.full((bt, 1, 1, m), -np.inf) if u_lo is None else np.asarray(u_lo, np.float64).reshape(bt, 1, 1, m)
    hi = np.full((bt, 1, 1, m), np.inf) if u_hi is None else np.asarray(u_hi, np.float64).reshape(bt, 1, 1, m)
    mv = lambda Y, v: np.einsum("bij,bsj->bsi", Y, v)
    mtv = lambda Y, v: np.einsum("bji,bsj->bsi", Y, v)
    X = np.zeros((bt, S, N, n))
    X[:, :, 0] = x0
    for k in range(N - 1):
        X[:, :, k + 1] = mv(A[:, k], X[:, :, k]) + mv(B[:, k], Z[:, :, k]) + c[:, None, k]
    lam = mv(Qf, X[:, :, N - 1]) + qf
    g = np.zeros((bt, S, N - 1, m))
    for k in range(N - 2, -1, -1):
        g[:, :, k] = mv(R[:, k], Z[:, :, k]) + mv(M[:, k], X[:, :, k]) + r[:, :, k] + mtv(B[:, k], lam)
        lam = mv(Q[:, k], X[:, :, k]) + mtv(M[:, k], Z[:, :, k]) + q[:, :, k] + mtv(A[:, k], lam)
    nat = np.abs(Z - np.clip(Z - g, lo, hi)).max(axis=(2, 3))
    return nat, g


def active_share(U, u_lo, u_hi, bt: int, m: int) -> float:
    """the share of the entries of U (bt, S, N−1, m) that sit on a bound"""
    lo, hi = np.asarray(u_lo).reshape(bt, 1, 1, m), np.asarray(u_hi).reshape(bt, 1, 1, m)
    return float(((U == lo) | (U == hi)).mean())
