"""Checker for the DP solve kinds past the committed oracle — affine (lqrx_dp_solve_affine), cross
(lqrx_dp_solve_cross), value (lqrx_dp_solve_value) — and the helpers their tests share: one numpy
restatement of the recursion of include/lqrx.h, batched over flat ABI arrays like
oracle.dp_solve_lin_abi.  (The plain and linear kinds are checked against the oracle itself.)

Dynamics x_{k+1} = A_k x_k + B_k u_k + c_k, stage cost ½xᵀQx + uᵀMx + ½uᵀRu + qᵀx + rᵀu
(+ terminal ½xᵀQf x + qfᵀx).  With V_{k+1}(x) = ½xᵀP x + pᵀx + s:

    E   = R_k + BᵀPB
    G   = BᵀPA + M_k                      (cross, value; the affine kind has no M: G = BᵀPA)
    p̃   = p_{k+1} + P_{k+1} c_k           h_k = r_k + Bᵀp̃
    K_k = E⁻¹G              d_k = E⁻¹h_k
    P_k = Q_k + AᵀPA − GᵀK_k     p_k = q_k + Aᵀp̃ − Gᵀd_k
    s_N = 0,  s_k = s_{k+1} + c_kᵀ(p_{k+1} + ½P_{k+1}c_k) − ½h_kᵀd_k,  dV = Σ_k h_kᵀd_k      (value)
    J   = ½x0ᵀP_1x0 + p_1ᵀx0 + s_1        (= the cost of the rolled-out X, U)
    rollout: u_k = −K_k x_k − d_k,  x_{k+1} = A_k x_k + B_k u_k + c_k

s and dV are sums of terms of either sign, so their errors are measured on the scale of the terms,
S = Σ_k (|c_kᵀ(p + ½Pc_k)| + ½|h_kᵀd_k|) per trajectory: relative to max(1, S) for s and dV, to
max(1, S + |J|) for J.

Pinned on the CPU against the dense equality-constrained QP (optimum, dynamics multipliers, cost)
and the committed oracle: tests/test_dp_affine.py (c = 0 equals oracle.dp_solve_lin_abi),
tests/test_dp_cross.py (M = 0 equals the affine kind, the feedback-shift identity),
tests/test_dp_value.py (J through cost_of).
"""
import numpy as np

KINDS = ("affine", "cross", "value")


def _mats(a, bt, k, r, c, dt):
    """flat ABI (column-major per matrix, batch slowest) → logical (bt, k, r, c)"""
    return np.swapaxes(np.asarray(a, dtype=dt).reshape(bt, k, c, r), -1, -2)


def _flat(a):
    """logical (..., r, c) → flat ABI"""
    return np.ascontiguousarray(np.swapaxes(a, -1, -2)).ravel()


def dp_solve_abi_np(d: dict, N: int, kind: str, all_P: bool = False, dtype=np.float64) -> dict:
    """d: flat ABI arrays A, B, Q, R, Qf, x0, q, r, qf, c (and M past the affine kind, which
    ignores one that is present) and n, m, batch, optional tv_AB / tv_QR (c follows A, B; M, q, r
    follow Q, R; M is m×n column-major per knot).  Returns flat ABI K, P (P_1, or every P_k with
    all_P), X, U, d, p (p_1 or every p_k), info (first knot whose E has a non-positive eigenvalue);
    the value kind adds s (batch, or batch·N with all_P: s_k at k−1, s_N = 0), dV, J (batch) and
    the float64 scale S (batch).  `dtype` is the precision every operation runs in."""
    assert kind in KINDS, kind
    n, m, bt = d["n"], d["m"], d["batch"]
    kab = N - 1 if d.get("tv_AB") else 1
    kqr = N - 1 if d.get("tv_QR") else 1
    dt = dtype
    A = _mats(d["A"], bt, kab, n, n, dt)
    B = _mats(d["B"], bt, kab, n, m, dt)
    Q = _mats(d["Q"], bt, kqr, n, n, dt)
    R = _mats(d["R"], bt, kqr, m, m, dt)
    M = _mats(d["M"], bt, kqr, m, n, dt) if kind != "affine" else None
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
        Qk, Rk = Q[:, (k - 1) % kqr], R[:, (k - 1) % kqr]
        qk, rk = q[:, (k - 1) % kqr], r[:, (k - 1) % kqr]
        Pc = mv(P, ck)
        sc = dot(ck, p + half * Pc)
        pt = p + Pc
        PA = P @ Ak
        E = Rk + T(Bk) @ (P @ Bk)
        G = T(Bk) @ PA
        if M is not None:
            G = G + M[:, (k - 1) % kqr]
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
    out = dict(K=_flat(Ks), P=_flat(Ps if all_P else Ps[:, 0]), X=X.ravel(), U=U.ravel(),
               d=ds.ravel(), p=(ps if all_P else ps[:, 0]).ravel(), info=info)
    if kind == "value":
        J = half * dot(x0, mv(P, x0)) + dot(p, x0) + s
        out.update(s=(ss.ravel() if all_P else ss[:, 0].copy()), dV=dV, J=J, S=S)
    return out


def dense_kkt(A, B, c, Q, R, M, Qf, x0, N, q, r, qf):
    """Dense equality-constrained QP optimum of one problem (logical matrices; every per-knot
    field shaped (N−1, …), M (N−1, m, n) or None for no cross term): minimise the cost, whose
    Hessian carries H[u_k, x_k] = M_k and its transpose, subject to x_1 = x0 and
    x_{k+1} − A_k x_k − B_k u_k = c_k.  Returns X (N, n), U (N−1, m) and the multipliers lam
    (N, n): lam[0] of the initial condition, lam[k] of the dynamics row into knot k (0-based),
    for the Lagrangian cost + Σ lamᵀ(row), so that P_k x_k + p_k = −lam[k] at every knot."""
    n, m = B.shape[-2:]
    nz = N * n + (N - 1) * m
    H = np.zeros((nz, nz))
    g = np.zeros(nz)
    ix = lambda k: slice(k * (n + m), k * (n + m) + n)
    iu = lambda k: slice(k * (n + m) + n, k * (n + m) + n + m)
    for k in range(N - 1):
        H[ix(k), ix(k)] = Q[k]
        H[iu(k), iu(k)] = R[k]
        if M is not None:
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


def affine_problem(lqrx, n, m, N, bt, seed, tv_QR=False, tv_AB=False):
    """random_batch + q, r, qf, c ~ N(0, 1) (flat ABI arrays); per-knot fields perturbed as
    lin_problem of tests/test_dp_linear_gpu.py does.  c follows A, B."""
    from lqrx.dp import from_abi, to_abi

    d = lqrx.random_batch(n, m, N, bt, seed)
    rng = np.random.default_rng(seed + 7)
    kq = N - 1 if tv_QR else 1
    kab = N - 1 if tv_AB else 1
    d["q"] = rng.standard_normal(bt * kq * n)
    d["r"] = rng.standard_normal(bt * kq * m)
    d["qf"] = rng.standard_normal(bt * n)
    d["c"] = rng.standard_normal(bt * kab * n)
    if tv_QR:
        s = 1.0 + 0.5 * rng.random((bt, N - 1, 1, 1))
        Q = from_abi(d["Q"], (bt, n, n))[:, None] * s
        R = from_abi(d["R"], (bt, m, m))[:, None] * s
        d["Q"] = to_abi(Q.reshape(-1, n, n)).ravel()
        d["R"] = to_abi(R.reshape(-1, m, m)).ravel()
        d["tv_QR"] = 1
    if tv_AB:
        A = from_abi(d["A"], (bt, n, n))[:, None] + 0.02 * rng.standard_normal((bt, N - 1, n, n))
        B = from_abi(d["B"], (bt, n, m))[:, None] * (1.0 + 0.1 * rng.random((bt, N - 1, 1, 1)))
        d["A"] = to_abi(A.reshape(-1, n, n)).ravel()
        d["B"] = to_abi(B.reshape(-1, n, m)).ravel()
        d["tv_AB"] = 1
    return d


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


def relerr_per_knot(a, b):
    """max over knots of max|a−b| / max|b| (leading axes: batch, knot)."""
    a = a.reshape(a.shape[0], a.shape[1], -1)
    b = b.reshape(b.shape[0], b.shape[1], -1)
    num = np.abs(a - b).max(axis=2)
    den = np.abs(b).max(axis=2)
    den[den == 0] = 1.0
    return float((num / den).max())


def relerr_traj(a, b):
    """max over trajectories of max|a−b| / max|b| over the whole trajectory."""
    a = a.reshape(a.shape[0], -1)
    b = b.reshape(b.shape[0], -1)
    den = np.abs(b).max(axis=1)
    den[den == 0] = 1.0
    return float((np.abs(a - b).max(axis=1) / den).max())


def to_batch(d, N, fields=("q", "r", "qf", "c", "M")):
    """flat ABI problem → LQRBatch, with those of `fields` that d holds (the rest None)."""
    from lqrx.dp import LQRBatch, from_abi

    n, m, bt = d["n"], d["m"], d["batch"]
    kab = N - 1 if d.get("tv_AB") else 1
    kq = N - 1 if d.get("tv_QR") else 1
    sh = lambda a, r, c, k: from_abi(a, (bt, k, r, c)) if k > 1 else from_abi(a, (bt, r, c))
    vec = lambda a, w, k: a.reshape(bt, k, w) if k > 1 else a.reshape(bt, w)
    has = lambda f: f in fields and f in d
    return LQRBatch(sh(d["A"], n, n, kab), sh(d["B"], n, m, kab), sh(d["Q"], n, n, kq),
                    sh(d["R"], m, m, kq), from_abi(d["Qf"], (bt, n, n)), d["x0"].reshape(bt, n), N,
                    q=vec(d["q"], n, kq) if has("q") else None, r=vec(d["r"], m, kq) if has("r") else None,
                    qf=d["qf"].reshape(bt, n) if has("qf") else None,
                    c=vec(d["c"], n, kab) if has("c") else None, M=sh(d["M"], m, n, kq) if has("M") else None)


def logical(ref, n, m, N, bt, all_P):
    """flat ABI result arrays → the logical arrays solve_batch returns"""
    from lqrx.dp import from_abi

    return dict(K=from_abi(ref["K"], (bt, N - 1, m, n)),
                P=from_abi(ref["P"], (bt, N, n, n) if all_P else (bt, n, n)),
                X=ref["X"].reshape(bt, N, n), U=ref["U"].reshape(bt, N - 1, m),
                d=ref["d"].reshape(bt, N - 1, m),
                p=ref["p"].reshape(bt, N, n) if all_P else ref["p"].reshape(bt, n), info=ref["info"])


def check(got, ref, all_P, tol, what=""):
    """got, ref: logical arrays.  Prints every figure, then asserts."""
    e = dict(K=relerr_per_knot(got["K"], ref["K"]),
             P=relerr_per_knot(got["P"], ref["P"]) if all_P else relerr_per_knot(got["P"][:, None], ref["P"][:, None]),
             d=relerr_traj(got["d"], ref["d"]), p=relerr_traj(got["p"], ref["p"]))
    for k in ("X", "U"):
        e[k] = float(np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max()))
    print(what, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert (got["info"] == 0).all() and (ref["info"] == 0).all()
    for k, v in e.items():
        assert v <= tol, (k, v)


# the shapes every kind's GPU parity test runs: (n, m, N, batch, tv_QR, tv_AB, all_P), and the fp32 ones
# (n, m, N, batch, tv)
PARITY = [
    (1, 1, 6, 3, False, False, True),       # lane, degenerate
    (4, 1, 40, 67, False, False, True),     # lane, partial second wave (quad-sized batch: the detour)
    (3, 2, 40, 9, True, True, True),        # lane, time-varying
    (2, 2, 30, 5, True, True, False),       # lane, time-varying, p_1 only
    (6, 3, 30, 7, False, False, True),      # MFMA 1×1 padded
    (17, 5, 12, 3, True, True, True),       # 2×1 padded, time-varying
    (32, 16, 40, 4, False, False, True),    # 2×1 exact, time-invariant: dp_rollout_full
    (32, 16, 256, 3, True, True, False),    # 2×1 exact, time-varying, full horizon, p_1 only
    (24, 18, 10, 3, False, False, True),    # 2×2
    (64, 32, 12, 2, False, False, True),    # fp64 n = 64: one-wave 4×2 (the wg4 detour)
    (48, 16, 10, 2, True, True, True),      # 4×1 in the 4×2 grid, time-varying
    (65, 4, 8, 2, False, False, True),      # big kernel
    (70, 8, 9, 3, True, True, False),       # big kernel, time-varying
]
F32_SHAPES = [(6, 3, 30, 7, False), (32, 16, 40, 3, True), (64, 32, 12, 2, False)]


def feedback_shift(lqrx, n, m, N, bt, seed):
    """(d, F): d the linear-terms problem of affine_problem with c = 0 (flat ABI, time-invariant),
    dx the cross problem it becomes under u = ũ − F x, F ~ 0.3/√n · N(0, 1) per trajectory."""
    from lqrx.dp import from_abi, to_abi

    d = affine_problem(lqrx, n, m, N, bt, seed)
    d["c"] = np.zeros_like(d["c"])
    F = 0.3 / np.sqrt(n) * np.random.default_rng(seed + 1).standard_normal((bt, m, n))
    A = from_abi(d["A"], (bt, n, n)); B = from_abi(d["B"], (bt, n, m))
    Q = from_abi(d["Q"], (bt, n, n)); R = from_abi(d["R"], (bt, m, m))
    Ft = np.swapaxes(F, -1, -2)
    dx = dict(d)
    dx["A"] = to_abi(A + B @ F).ravel()
    Qx = Q + Ft @ R @ F
    dx["Q"] = to_abi((Qx + np.swapaxes(Qx, -1, -2)) / 2).ravel()
    dx["M"] = to_abi(R @ F).ravel()
    dx["q"] = (d["q"].reshape(bt, n) + np.einsum("bij,bj->bi", Ft, d["r"].reshape(bt, m))).ravel()
    return d, dx, F


def feedback_shift_reference(lin, F, n, m, N, bt):
    """What the cross problem of feedback_shift must return, from the linear-terms solution `lin`
    (flat ABI, all P): P, p, d, X unchanged, K = K̃ + F, U = Ũ − F X̃.  Logical arrays."""
    from lqrx.dp import from_abi

    K = from_abi(lin["K"], (bt, N - 1, m, n)) + F[:, None]
    X = lin["X"].reshape(bt, N, n)
    U = lin["U"].reshape(bt, N - 1, m) - np.einsum("bij,bkj->bki", F, X[:, :-1])
    return dict(K=K, P=from_abi(lin["P"], (bt, N, n, n)), X=X, U=U, d=lin["d"].reshape(bt, N - 1, m),
                p=lin["p"].reshape(bt, N, n), info=lin["info"])
