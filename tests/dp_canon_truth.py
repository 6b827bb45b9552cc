"""numpy model of the Riccati recursion in input-canonical coordinates (DESIGN §3.1;
lqrx_dp_canon.hip, dp_riccati_kernel's VAR_CANON), batched over logical arrays.

For a time-invariant problem take the Householder QR of B:  B = T·[B₁; 0], T orthogonal n×n, B₁
upper triangular m×m, S = B₁⁻¹.  In x̃ = Tᵀx, ũ = B₁u the problem is

    Ã = TᵀAT,  B̃ = [I_m; 0],  Q̃ = TᵀQT,  Q̃f = TᵀQfT,  R̃ = SᵀRS

and P̃_k = TᵀP_kT obeys the same recursion with three products gone:

    PA = P̃Ã      Ẽ = R̃ + P̃[0:m, 0:m]      G̃ = PA[0:m, :]      K̃ = Ẽ⁻¹G̃
    P̃ ← Q̃ + ÃᵀPA − G̃ᵀK̃                 K = S·K̃·Tᵀ             P_1 = T·P̃_1·Tᵀ

The set-up excludes a trajectory (it stays on the direct form) when a reflector meets an exactly
zero column, a value is not finite, or κ∞(B₁) = ‖B₁‖∞‖S‖∞ exceeds KAPPA_MAX — the library's
DP_CANON_KAPPA_F64 (lqrx_internal.h), derived by kappa_sweep() below.
"""
import numpy as np

KAPPA_MAX = 2.5e13   # = DP_CANON_KAPPA_F64


def _T(M):
    return np.swapaxes(M, -1, -2)


def canon_setup(A, B, Q, R, Qf):
    """A (bt, n, n), B (bt, n, m), Q, R (bt, m, m), Qf → dict of T, B1, S, kappa (bt,), deficient (bt,)
    and the transformed At, Qt, Qft, Rt, in the arrays' precision."""
    bt, n, m = B.shape
    T = np.zeros((bt, n, n), B.dtype)
    B1 = np.zeros((bt, m, m), B.dtype)
    for t in range(bt):
        q, r = np.linalg.qr(B[t].astype(np.float64), mode="complete")
        T[t], B1[t] = q, np.triu(r[:m])
    dg = np.abs(np.einsum("bii->bi", B1))
    deficient = ~(dg > 0).all(axis=1)
    with np.errstate(all="ignore"):
        S = np.zeros_like(B1)
        for t in range(bt):
            S[t] = np.nan if deficient[t] else np.linalg.solve(B1[t].astype(np.float64), np.eye(m))
        kappa = np.abs(B1).sum(axis=2).max(axis=1) * np.abs(S).sum(axis=2).max(axis=1)
    sym = lambda M: (M + _T(M)) / 2
    return dict(T=T, B1=B1, S=S, kappa=kappa, deficient=deficient,
                At=_T(T) @ A @ T, Qt=sym(_T(T) @ Q @ T), Qft=sym(_T(T) @ Qf @ T), Rt=sym(_T(S) @ R @ S))


def canon_applies(B, kappa_max=KAPPA_MAX):
    """(bt,) bool: the set-up's verdict — full column rank, finite, κ∞(B₁) ≤ kappa_max."""
    z = np.zeros((B.shape[0], B.shape[1], B.shape[1]))
    s = canon_setup(z, B, z, np.zeros((B.shape[0], B.shape[2], B.shape[2])), z)
    with np.errstate(invalid="ignore"):
        return ~s["deficient"] & (s["kappa"] <= kappa_max)


class NsInverse:
    """The kernels' inverse of E in float64 (lqrx_dp.hip ns_refine): Newton–Schulz X ← X + X(I − EX)
    from the extrapolated warm start 2X_{k+1} − X_{k+2}, accepted at ρ = 16·MT·max|I − EX| ≤ 1e-11, or
    after the step taken at ρ ≤ 1e-9; the first knot, no contraction (ρ ≥ 1) or six rounds without
    acceptance take the exact inverse.  What the acceptance leaves of I − EX reaches the gain as
    δK = −(I − EX)ᵀK in the direct form and as −S(I − EX)ᵀB₁·K in the canonical one — the term of
    the conditioning sweep that grows with κ(B₁)."""

    def __init__(self):
        self.Xi = self.Xp = None

    def __call__(self, E):
        m = E.shape[-1]
        I = np.eye(m)
        X = np.linalg.inv(E)
        if self.Xi is not None:
            W = 2 * self.Xi - self.Xp
            for t in range(E.shape[0]):
                Y = W[t]
                for _ in range(6):
                    rho = 16 * (m // 16) * np.abs(I - E[t] @ Y).max()
                    if rho <= 1e-11:
                        X[t] = Y
                        break
                    if not rho < 1:
                        break
                    Y = Y + Y @ (I - E[t] @ Y)
                    if rho <= 1e-9:
                        X[t] = Y
                        break
        self.Xp = self.Xi if self.Xi is not None else X
        self.Xi = X
        return X


def dp_canon(A, B, Q, R, Qf, N, dtype=np.float64, ns=False):
    """The canonical recursion in `dtype` (ns: float64 with the kernels' Newton–Schulz inverse).  Returns K (bt, N−1, m, n) and P1 (bt, n, n) in original
    coordinates, and the canonical Kt (bt, N−1, m, n), Et (bt, N−1, m, m), with the set-up `setup`."""
    dt = np.dtype(dtype).type
    A, B, Q, R, Qf = (np.asarray(x, dtype=dt) for x in (A, B, Q, R, Qf))
    bt, n, m = B.shape
    s = canon_setup(A, B, Q, R, Qf)
    At, Qt, Rt, T, S = s["At"], s["Qt"], s["Rt"], s["T"], s["S"]
    P = s["Qft"].copy()
    K = np.zeros((bt, N - 1, m, n), dt)
    Kt = np.zeros((bt, N - 1, m, n), dt)
    Et = np.zeros((bt, N - 1, m, m), dt)
    solve = (lambda E, G: np.linalg.solve(E, G)) if dt is not np.longdouble else \
        (lambda E, G: np.stack([_ld_solve(E[t], G[t]) for t in range(bt)]))
    if ns:
        inv = NsInverse()
        solve = lambda E, G: _T(inv(E)) @ G
    for k in range(N - 1, 0, -1):
        PA = P @ At
        E = Rt + P[:, :m, :m]
        G = PA[:, :m, :]
        Kc = solve(E, G)
        P = Qt + _T(At) @ PA - _T(G) @ Kc
        P = (P + _T(P)) / 2
        Kt[:, k - 1], Et[:, k - 1] = Kc, E
        K[:, k - 1] = S @ Kc @ _T(T)
    return dict(K=K, P1=T @ P @ _T(T), Kt=Kt, Et=Et, setup=s)


def dp_direct(A, B, Q, R, Qf, N, ns=False):
    """The direct fast form of the generic kernel in float64 (ns: with the Newton–Schulz inverse): E = R + BᵀPB, G = BᵀPA, P ← Q + AᵀPA − GᵀK.
    Returns K (bt, N−1, m, n), P1, E (bt, N−1, m, m)."""
    bt, n, m = B.shape
    P = Qf.copy()
    K = np.zeros((bt, N - 1, m, n))
    Es = np.zeros((bt, N - 1, m, m))
    inv = NsInverse()
    for k in range(N - 1, 0, -1):
        PA = P @ A
        E = R + _T(B) @ (P @ B)
        G = _T(B) @ PA
        Kk = _T(inv(E)) @ G if ns else np.linalg.solve(E, G)
        P = Q + _T(A) @ PA - _T(G) @ Kk
        P = (P + _T(P)) / 2
        K[:, k - 1], Es[:, k - 1] = Kk, E
    return dict(K=K, P1=P, E=Es)


def _ld_solve(E, G):
    """Gaussian elimination with partial pivoting in the arrays' own precision (longdouble)."""
    E, G = E.copy(), G.copy()
    m = E.shape[0]
    for i in range(m):
        p = i + int(np.argmax(np.abs(E[i:, i])))
        if p != i:
            E[[i, p]], G[[i, p]] = E[[p, i]], G[[p, i]]
        f = E[i + 1:, i] / E[i, i]
        E[i + 1:] -= f[:, None] * E[i]
        G[i + 1:] -= f[:, None] * G[i]
    for i in range(m - 1, -1, -1):
        G[i] = (G[i] - E[i, i + 1:] @ G[i + 1:]) / E[i, i]
    return G


def with_cond(B, cond):
    """B (bt, n, m) with its singular values respaced geometrically from σ_max down to σ_max/cond."""
    out = np.empty_like(B)
    for t in range(B.shape[0]):
        u, s, vt = np.linalg.svd(B[t], full_matrices=False)
        out[t] = (u * (s[0] * cond ** (-np.arange(s.size) / (s.size - 1.0)))) @ vt
    return out


def kappa_sweep(family, conds, N, ns=True):
    """The conditioning sweep behind KAPPA_MAX.  family: logical float64 A, B, Q, R, Qf of one batch.
    For each cond(B) in conds: worst per-knot relative K error of the canonical and the direct float64
    recursions (ns: with the kernels' Newton–Schulz inverse, NsInverse) against the longdouble reference recursion (oracle.dp_reference), and the largest
    κ∞(B₁) of the batch.  Returns rows (cond, kappa, err_canon, err_direct)."""
    from dp_truth import relerr_per_knot
    from oracle import oracle as orc

    A, B, Q, R, Qf = family
    rows = []
    for c in conds:
        Bc = with_cond(B, c)
        ref = orc.dp_reference(A, Bc, Q, R, Qf, N, dtype=np.longdouble)["K"]
        cn = dp_canon(A, Bc, Q, R, Qf, N, ns=ns)
        dr = dp_direct(A, Bc, Q, R, Qf, N, ns=ns)
        rows.append((c, float(cn["setup"]["kappa"].max()),
                     relerr_per_knot(cn["K"].astype(np.longdouble), ref),
                     relerr_per_knot(dr["K"].astype(np.longdouble), ref)))
    return rows
