"""Checker for the value function's constant (lqrx_dp_solve_value): dp_cross_truth's recursion with
the third part of V_k(x) = ½xᵀP_k x + p_kᵀx + s_k, batched over flat ABI arrays.

With E = R_k + BᵀPB, G = BᵀPA + M_k, p̃ = p_{k+1} + P_{k+1}c_k, h = r_k + Bᵀp̃, d_k = E⁻¹h:

    s_N = 0
    s_k = s_{k+1} + c_kᵀ(p_{k+1} + ½P_{k+1}c_k) − ½h_kᵀd_k
    dV  = Σ_k h_kᵀd_k
    J   = ½x0ᵀP_1x0 + p_1ᵀx0 + s_1          (= the cost of the rolled-out X, U)

s and dV are sums of terms of either sign, so their errors are measured on the scale of the terms,
S = Σ_k (|c_kᵀ(p + ½Pc_k)| + ½|h_kᵀd_k|) per trajectory: relative to max(1, S) for s and dV, to
max(1, S + |J|) for J.  Pinned in tests/test_dp_value.py against the dense QP of
dp_cross_truth.dense_cross_kkt through cost_of().
"""
import numpy as np

from dp_affine_truth import _flat, _mats


def dp_solve_value_abi(d: dict, N: int, all_P: bool = False, dtype=np.float64) -> dict:
    """dp_cross_truth.dp_solve_cross_abi (same arguments, same K, P, X, U, d, p, info) plus
    s (batch, or batch·N with all_P: s_k at k−1, s_N = 0), dV, J (batch) and the float64 scale
    S (batch).  `dtype` is the precision every operation runs in."""
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
    dot = lambda a, b: np.einsum("bi,bi->b", a, b)
    half = dt(0.5)
    Ks = np.zeros((bt, N - 1, m, n), dt)
    Ps = np.zeros((bt, N, n, n), dt)
    ds = np.zeros((bt, N - 1, m), dt)
    ps = np.zeros((bt, N, n), dt)
    ss = np.zeros((bt, N), dt)
    s = np.zeros(bt, dt)
    dV = np.zeros(bt, dt)
    S = np.zeros(bt, np.float64)
    info = np.zeros(bt, np.int32)
    Ps[:, N - 1] = P
    ps[:, N - 1] = p
    for k in range(N - 1, 0, -1):
        Ak, Bk, ck = A[:, (k - 1) % kab], B[:, (k - 1) % kab], c[:, (k - 1) % kab]
        Qk, Rk, Mk = Q[:, (k - 1) % kqr], R[:, (k - 1) % kqr], M[:, (k - 1) % kqr]
        qk, rk = q[:, (k - 1) % kqr], r[:, (k - 1) % kqr]
        Pc = mv(P, ck)
        sc = dot(ck, p + half * Pc)
        pt = p + Pc
        PA = P @ Ak
        E = Rk + T(Bk) @ (P @ Bk)
        G = T(Bk) @ PA + Mk
        for t in range(bt):
            if info[t] == 0:
                ev = np.linalg.eigvalsh(((E[t] + E[t].T) / 2).astype(np.float64))
                if not ev.min() > 0:
                    info[t] = k
        K = np.linalg.solve(E, G)
        h = rk + mv(T(Bk), pt)
        dk = np.linalg.solve(E, h[..., None])[..., 0]
        hd = dot(h, dk)
        s = s + sc - half * hd
        dV = dV + hd
        S += np.abs(sc.astype(np.float64)) + 0.5 * np.abs(hd.astype(np.float64))
        p = qk + mv(T(Ak), pt) - mv(T(G), dk)
        P = Qk + T(Ak) @ PA - T(G) @ K
        P = (P + T(P)) / 2
        Ks[:, k - 1], ds[:, k - 1], Ps[:, k - 1], ps[:, k - 1], ss[:, k - 1] = K, dk, P, p, s
    X = np.zeros((bt, N, n), dt)
    U = np.zeros((bt, N - 1, m), dt)
    X[:, 0] = x0
    for k in range(1, N):
        Ak, Bk, ck = A[:, (k - 1) % kab], B[:, (k - 1) % kab], c[:, (k - 1) % kab]
        U[:, k - 1] = -mv(Ks[:, k - 1], X[:, k - 1]) - ds[:, k - 1]
        X[:, k] = mv(Ak, X[:, k - 1]) + mv(Bk, U[:, k - 1]) + ck
    J = half * dot(x0, mv(P, x0)) + dot(p, x0) + s
    return dict(K=_flat(Ks), P=_flat(Ps if all_P else Ps[:, 0]), X=X.ravel(), U=U.ravel(),
                d=ds.ravel(), p=(ps if all_P else ps[:, 0]).ravel(), info=info,
                s=(ss.ravel() if all_P else ss[:, 0].copy()), dV=dV, J=J, S=S)


def cost_of(d: dict, X, U) -> np.ndarray:
    """Σ_k (½xᵀQ_k x + uᵀM_k x + ½uᵀR_k u + q_kᵀx + r_kᵀu) + ½x_NᵀQf x_N + qfᵀx_N of the
    trajectories X (batch, N, n), U (batch, N−1, m) of the flat ABI problem d, in float64; (batch,)."""
    n, m, bt = d["n"], d["m"], d["batch"]
    X = np.asarray(X, np.float64).reshape(bt, -1, n)
    N = X.shape[1]
    U = np.asarray(U, np.float64).reshape(bt, N - 1, m)
    kqr = N - 1 if d.get("tv_QR") else 1
    f8 = np.float64
    Q = _mats(d["Q"], bt, kqr, n, n, f8)
    R = _mats(d["R"], bt, kqr, m, m, f8)
    M = _mats(d["M"], bt, kqr, m, n, f8)
    Qf = _mats(d["Qf"], bt, 1, n, n, f8)[:, 0]
    q = np.asarray(d["q"], f8).reshape(bt, kqr, n)
    r = np.asarray(d["r"], f8).reshape(bt, kqr, m)
    qf = np.asarray(d["qf"], f8).reshape(bt, n)
    J = np.zeros(bt)
    for k in range(1, N):
        x, u, i = X[:, k - 1], U[:, k - 1], (k - 1) % kqr
        J += 0.5 * np.einsum("bi,bij,bj->b", x, Q[:, i], x) + np.einsum("bi,bij,bj->b", u, M[:, i], x)
        J += 0.5 * np.einsum("bi,bij,bj->b", u, R[:, i], u)
        J += np.einsum("bi,bi->b", q[:, i], x) + np.einsum("bi,bi->b", r[:, i], u)
    xN = X[:, N - 1]
    return J + 0.5 * np.einsum("bi,bij,bj->b", xN, Qf, xN) + np.einsum("bi,bi->b", qf, xN)


def value_errors(got: dict, ref: dict) -> dict:
    """Errors of s, dV, J (arrays shaped (batch, …)) against the checker's on its scales, per
    trajectory: s and dV relative to max(1, S), J to max(1, S + |J|)."""
    S = ref["S"]
    bt = S.shape[0]
    f8 = np.float64
    es = np.abs(np.asarray(got["s"], f8).reshape(bt, -1) - np.asarray(ref["s"], f8).reshape(bt, -1)).max(axis=1)
    edV = np.abs(np.asarray(got["dV"], f8) - np.asarray(ref["dV"], f8))
    Jr = np.asarray(ref["J"], f8)
    eJ = np.abs(np.asarray(got["J"], f8) - Jr)
    return dict(s=es / np.maximum(1, S), dV=edV / np.maximum(1, S), J=eJ / np.maximum(1, S + np.abs(Jr)))
