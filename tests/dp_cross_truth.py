"""Checker for the DP with a cost cross term (lqrx_dp_solve_cross): a numpy restatement of the
recursion of include/lqrx.h, batched over flat ABI arrays like dp_affine_truth.dp_solve_affine_abi.

Dynamics x_{k+1} = A_k x_k + B_k u_k + c_k, stage cost ½xᵀQx + uᵀMx + ½uᵀRu + qᵀx + rᵀu
(+ terminal ½xᵀQf x + qfᵀx).  With V_{k+1}(x) = ½xᵀP x + pᵀx:

    E   = R_k + BᵀPB
    G   = BᵀPA + M_k
    p̃   = p_{k+1} + P_{k+1} c_k
    K_k = E⁻¹G              d_k = E⁻¹(r_k + Bᵀp̃)
    P_k = Q_k + AᵀPA − GᵀK_k     p_k = q_k + Aᵀp̃ − Gᵀd_k
    rollout: u_k = −K_k x_k − d_k,  x_{k+1} = A_k x_k + B_k u_k + c_k

It is pinned in tests/test_dp_cross.py against the dense equality-constrained QP with the
off-diagonal Hessian blocks H[u_k, x_k] = M_k, with M = 0 against dp_solve_affine_abi, and through
the feedback-shift identity against oracle.dp_solve_lin_abi.
"""
import numpy as np

from dp_affine_truth import _flat, _mats, affine_problem


def dp_solve_cross_abi(d: dict, N: int, all_P: bool = False, dtype=np.float64) -> dict:
    """d: flat ABI arrays A, B, Q, R, M, Qf, x0, q, r, qf, c and n, m, batch, optional tv_AB /
    tv_QR (c follows A, B; M, q, r follow Q, R; M is m×n column-major per knot).  Returns flat
    ABI K, P (P_1, or every P_k with all_P), X, U, d, p (p_1 or every p_k), info (first knot
    whose E has a non-positive eigenvalue).  `dtype` is the precision every operation runs in."""
    n, m, bt = d["n"], d["m"], d["batch"]
    kab = N - 1 if d.get("tv_AB") else 1
    kqr = N - 1 if d.get("tv_QR") else 1
    dt = dtype
    A = _mats(d["A"], bt, kab, n, n, dt)
    B = _mats(d["B"], bt, kab, n, m, dt)
    Q = _mats(d["Q"], bt, kqr, n, n, dt)
    R = _mats(d["R"], bt, kqr, m, m, dt)
    M = _mats(d["M"], bt, kqr, m, n, dt)
    P = _mats(d["Qf"], bt, 1, n, n, dt)[:, 0].copy()
    c = np.asarray(d["c"], dtype=dt).reshape(bt, kab, n)
    q = np.asarray(d["q"], dtype=dt).reshape(bt, kqr, n)
    r = np.asarray(d["r"], dtype=dt).reshape(bt, kqr, m)
    p = np.asarray(d["qf"], dtype=dt).reshape(bt, n).copy()
    x0 = np.asarray(d["x0"], dtype=dt).reshape(bt, n)
    T = lambda Z: np.swapaxes(Z, -1, -2)
    mv = lambda Z, v: (Z @ v[..., None])[..., 0]
    Ks = np.zeros((bt, N - 1, m, n), dt)
    Ps = np.zeros((bt, N, n, n), dt)
    ds = np.zeros((bt, N - 1, m), dt)
    ps = np.zeros((bt, N, n), dt)
    info = np.zeros(bt, np.int32)
    Ps[:, N - 1] = P
    ps[:, N - 1] = p
    for k in range(N - 1, 0, -1):
        Ak, Bk, ck = A[:, (k - 1) % kab], B[:, (k - 1) % kab], c[:, (k - 1) % kab]
        Qk, Rk, Mk = Q[:, (k - 1) % kqr], R[:, (k - 1) % kqr], M[:, (k - 1) % kqr]
        qk, rk = q[:, (k - 1) % kqr], r[:, (k - 1) % kqr]
        pt = p + mv(P, ck)
        PA = P @ Ak
        E = Rk + T(Bk) @ (P @ Bk)
        G = T(Bk) @ PA + Mk
        for t in range(bt):
            if info[t] == 0:
                ev = np.linalg.eigvalsh(((E[t] + E[t].T) / 2).astype(np.float64))
                if not ev.min() > 0:
                    info[t] = k
        K = np.linalg.solve(E, G)
        dk = np.linalg.solve(E, (rk + mv(T(Bk), pt))[..., None])[..., 0]
        p = qk + mv(T(Ak), pt) - mv(T(G), dk)
        P = Qk + T(Ak) @ PA - T(G) @ K
        P = (P + T(P)) / 2
        Ks[:, k - 1], ds[:, k - 1], Ps[:, k - 1], ps[:, k - 1] = K, dk, P, p
    X = np.zeros((bt, N, n), dt)
    U = np.zeros((bt, N - 1, m), dt)
    X[:, 0] = x0
    for k in range(1, N):
        Ak, Bk, ck = A[:, (k - 1) % kab], B[:, (k - 1) % kab], c[:, (k - 1) % kab]
        U[:, k - 1] = -mv(Ks[:, k - 1], X[:, k - 1]) - ds[:, k - 1]
        X[:, k] = mv(Ak, X[:, k - 1]) + mv(Bk, U[:, k - 1]) + ck
    return dict(K=_flat(Ks), P=_flat(Ps if all_P else Ps[:, 0]), X=X.ravel(), U=U.ravel(),
                d=ds.ravel(), p=(ps if all_P else ps[:, 0]).ravel(), info=info)


def dense_cross_kkt(A, B, c, Q, R, M, Qf, x0, N, q, r, qf):
    """Dense equality-constrained QP optimum of one problem (logical matrices; every per-knot
    field shaped (N−1, …), M (N−1, m, n)): the Hessian carries H[u_k, x_k] = M_k and its
    transpose; rows x_1 = x0 and x_{k+1} − A_k x_k − B_k u_k = c_k.  Returns X (N, n), U (N−1, m)
    and the multipliers lam (N, n) with the sign convention of dense_affine_kkt, so that
    P_k x_k + p_k = −lam[k] at every knot."""
    n, m = B.shape[-2:]
    nz = N * n + (N - 1) * m
    H = np.zeros((nz, nz))
    g = np.zeros(nz)
    ix = lambda k: slice(k * (n + m), k * (n + m) + n)
    iu = lambda k: slice(k * (n + m) + n, k * (n + m) + n + m)
    for k in range(N - 1):
        H[ix(k), ix(k)] = Q[k]
        H[iu(k), iu(k)] = R[k]
        H[iu(k), ix(k)] = M[k]
        H[ix(k), iu(k)] = M[k].T
        g[ix(k)] = q[k]
        g[iu(k)] = r[k]
    H[ix(N - 1), ix(N - 1)] = Qf
    g[ix(N - 1)] = qf
    D = np.zeros((N * n, nz))
    rhs = np.zeros(N * n)
    D[0:n, ix(0)] = np.eye(n)
    rhs[0:n] = x0
    for k in range(N - 1):
        rows = slice((k + 1) * n, (k + 2) * n)
        D[rows, ix(k + 1)] = np.eye(n)
        D[rows, ix(k)] = -A[k]
        D[rows, iu(k)] = -B[k]
        rhs[rows] = c[k]
    Kkt = np.block([[H, D.T], [D, np.zeros((N * n, N * n))]])
    sol = np.linalg.solve(Kkt, np.concatenate([-g, rhs]))
    z = sol[:nz]
    X = np.stack([z[ix(k)] for k in range(N)])
    U = np.stack([z[iu(k)] for k in range(N - 1)])
    return X, U, sol[nz:].reshape(N, n)


def cross_problem(lqrx, n, m, N, bt, seed, tv_QR=False, tv_AB=False):
    """affine_problem + a cross term built so that every problem is strictly convex: one
    F_k ~ 0.3/√n · N(0, 1) per stored Q/R knot, M_k = R_k F_k and Q_k ← Q_k + F_kᵀR_kF_k.  The
    joint block [Q Mᵀ; M R] is then congruent to blkdiag(Q, R) ≻ 0 (u → u + F x), so info = 0."""
    from lqrx.dp import from_abi, to_abi

    d = affine_problem(lqrx, n, m, N, bt, seed, tv_QR, tv_AB)
    rng = np.random.default_rng(seed + 13)
    kq = N - 1 if tv_QR else 1
    F = 0.3 / np.sqrt(n) * rng.standard_normal((bt * kq, m, n))
    Q = from_abi(d["Q"], (bt * kq, n, n))
    R = from_abi(d["R"], (bt * kq, m, m))
    M = R @ F
    Q = Q + np.swapaxes(F, -1, -2) @ M
    d["Q"] = to_abi((Q + np.swapaxes(Q, -1, -2)) / 2).ravel()
    d["M"] = to_abi(M).ravel()
    return d
