"""numpy model of the pre-feedback recursion with a diagonal A₂₁ (dp_riccati_kernel's
VAR_DIAG, the set-up's flag 3), on top of tests/dp_canon_pf_truth.py.

The pre-feedback form leaves the dynamics [0; A₂], A₂ = [A₂₁ | A₂₂] the rows m … of Ã.  The orthogonal
freedom that keeps B̃ = [I; 0] is x̃ → diag(U₁, U₂)ᵀx̃, ũ → U₁ᵀũ.  With the SVD A₂₁ = U₂ΣU₁ᵀ (n = 2m, so
that A₂₁ is square) the rotated A₂ is [Σ | A₂₂′], and every product that meets its first column tile is
a scaling:

    T′ = T·diag(U₁, U₂)      S′ = S·U₁       (all congruences of the set-up with T′, S′ for T, S)
    PA[:, 0:m] = P̃[:, m:]·Σ  (columns scaled)          PA[:, m:] = P̃[:, m:]·A₂₂
    (A₂ᵀPA₂)[0:m, 0:m] = Σ·PA₂[:, 0:m]  (rows scaled)   the other lower blocks A₂₂ᵀPA₂

The SVD is a one-sided (Hestenes) Jacobi in the set-up kernel's pair order (jacobi_svd); σ is the
diagonal of the recomputed T′ᵀAT′'s lower-left block and what is left beside that diagonal is dropped —
a backward error in A — so the tier is admitted only when that is at rounding level (OFFDIAG_MULT), the
Jacobi converged, σ_min above that same level (and every σ within [SIGMA_LO, SIGMA_HI]) and κ∞(B₁) ≤ KAPPA_DG_MAX, the library's DP_DIAG_KAPPA_F64
(lqrx_internal.h), derived by kappa_sweep() below.
"""
import numpy as np

import dp_canon_pf_truth as pt
import dp_canon_truth as ct

KAPPA_DG_MAX = 1.4e2   # = DP_DIAG_KAPPA_F64
JACOBI_SWEEPS = 12     # the set-up's cap on sweeps (a counted loop)
JACOBI_TOL = 16 * np.finfo(np.float64).eps      # rotate while (w_p·w_q)² > (tol·‖w_p‖‖w_q‖)²
SIGMA_LO, SIGMA_HI = 1e-60, 1e60                # the range of σ in which those products stay normal
# Admission: max |off-diagonal| of the recomputed block ≤ OFFDIAG_MULT·ε·σ_max.  The block comes out of
# two chained n-term products with orthogonal factors, worst case 2·n·ε·‖A‖₂ per entry, and ‖A‖₂ is allowed
# to be twice σ_max(A₂₁): 4n.  What is dropped is then a relative backward error in A of 4nε = 2.8e-14,
# a four-hundredth of the 1e-11 the tier's bound is derived against.
OFFDIAG_MULT = 128

_T = ct._T


def partner(j, t, m=16):
    """Round-robin partner of column j in step t (0 … m−2) of a sweep: column m−1 meets t, the others
    pair up with i + j ≡ 2t (mod m−1)."""
    if j == m - 1:
        return t
    k = (2 * t - j) % (m - 1)
    return m - 1 if k == j else k


def jacobi_svd(A21, sweeps=JACOBI_SWEEPS, tol=JACOBI_TOL):
    """One-sided Jacobi on the columns of W = A21·V (bt, m, m), the kernel's order: every step rotates
    m/2 disjoint pairs, each column by own ← c·own − c·t·other with the tangent of its own view (the two
    views differ by the sign of t alone; at equal norms the lower column takes +1).  Returns U1 = V, U2 = W·diag(1/σ), σ = ‖w_j‖ and converged
    (a sweep went by without a rotation)."""
    W = A21.astype(np.float64).copy()
    bt, m, _ = W.shape
    V = np.broadcast_to(np.eye(m), W.shape).copy()
    conv = np.zeros(bt, bool)
    for _ in range(sweeps):
        rotated = np.zeros(bt, bool)
        for t in range(m - 1):
            idx = np.array([partner(j, t, m) for j in range(m)])
            Wo, Vo = W[:, :, idx], V[:, :, idx]
            a, g = (W * W).sum(1), (W * Wo).sum(1)
            b = a[:, idx]                       # the kernel's two views of a pair hold the same bits
            g = np.where(np.arange(m) < idx, g, g[:, idx])
            with np.errstate(all="ignore"):
                rot = g * g > (tol * tol) * (a * b)
                # division-free, as the kernel: d = ‖other‖² − ‖own‖², D = |d| + √(d² + (2γ)²), t = sign(d)·2γ/D,
                # c = D/√(D² + (2γ)²); d = 0: the lower column takes +1
                d, g2 = b - a, 2 * g
                D = np.abs(d) + np.sqrt(d * d + g2 * g2)
                q = 1 / np.sqrt(D * D + g2 * g2)
                sgn = np.where(d != 0, np.sign(d), np.where(np.arange(m) < idx, 1.0, -1.0))
                c, ctn = np.where(rot, D * q, 1.0), np.where(rot, sgn * g2 * q, 0.0)
            W = c[:, None, :] * W - ctn[:, None, :] * Wo
            V = c[:, None, :] * V - ctn[:, None, :] * Vo
            rotated |= rot.any(axis=1)
        conv |= ~rotated
        if conv.all():
            break
    sig = np.sqrt((W * W).sum(1))
    with np.errstate(all="ignore"):
        U2 = W / sig[:, None, :]
    return V, U2, sig, conv


def diag_setup(s, A, m):
    """What the set-up does for a flag-3 candidate, from canon_setup()'s dict s and the logical A, Q, …:
    the rotation and the dict of the rotated set-up (canon_setup's keys), with sigma, offdiag (bt,),
    converged (bt,)."""
    U1, U2, sig_j, conv = jacobi_svd(s["At"][:, m:, :m])
    bt, n, _ = s["T"].shape
    D = np.zeros_like(s["T"])
    D[:, :m, :m], D[:, m:, m:] = U1, U2
    with np.errstate(all="ignore"):
        Tp, Sp = s["T"] @ D, s["S"] @ U1
        blk = (_T(Tp) @ A @ Tp)[:, m:, :m]
    sig = np.einsum("bii->bi", blk).copy()
    off = np.abs(blk - sig[:, :, None] * np.eye(m)).max(axis=(1, 2))
    return dict(Tp=Tp, Sp=Sp, U1=U1, U2=U2, sigma=sig, sigma_jacobi=sig_j, offdiag=off, converged=conv)


def admitted(r, kappa, kappa_dg=KAPPA_DG_MAX):
    """(bt,) bool: the flag-3 verdict on diag_setup()'s dict r and κ∞(B₁)."""
    eps = np.finfo(np.float64).eps
    with np.errstate(invalid="ignore"):
        smin, smax = np.abs(r["sigma"]).min(axis=1), np.abs(r["sigma"]).max(axis=1)
        sj = r["sigma_jacobi"]
        return (kappa <= kappa_dg) & r["converged"] & ((sj >= SIGMA_LO) & (sj <= SIGMA_HI)).all(axis=1) \
            & (r["sigma"] > (OFFDIAG_MULT * eps * smax)[:, None]).all(axis=1) & (r["offdiag"] <= OFFDIAG_MULT * eps * smax)


def rotated_setup(A, B, Q, R, Qf):
    """canon_setup() in the rotated basis: the same dict with T′, S′ for T, S and every congruence redone,
    plus `diag` (diag_setup's dict) and the un-rotated `plain` set-up."""
    s = ct.canon_setup(A, B, Q, R, Qf)
    bt, n, m = B.shape
    r = diag_setup(s, A, m)
    Tp, Sp = r["Tp"], r["Sp"]
    sym = lambda M: (M + _T(M)) / 2
    return dict(T=Tp, B1=s["B1"], S=Sp, kappa=s["kappa"], deficient=s["deficient"],
                At=_T(Tp) @ A @ Tp, Qt=sym(_T(Tp) @ Q @ Tp), Qft=sym(_T(Tp) @ Qf @ Tp), Rt=sym(_T(Sp) @ R @ Sp),
                diag=r, plain=s)


def tier(A, B, kappa_max=ct.KAPPA_MAX, kappa_pf=pt.KAPPA_PF_MAX, kappa_dg=KAPPA_DG_MAX):
    """(bt,) int: the set-up's flag — 0, 1, 2 as pt.tier() from B alone; 3 for a flag-2 trajectory that
    admitted() takes.  kappa_dg = 0 (LQRX_DP_DIAG=0) admits nobody."""
    f = pt.tier(B, kappa_max, kappa_pf)
    if not (f == 2).any():
        return f
    z = np.zeros_like(A)
    s = ct.canon_setup(A, B, z, np.zeros((B.shape[0], B.shape[2], B.shape[2])), z)
    r = diag_setup(s, A, B.shape[2])
    return np.where((f == 2) & admitted(r, s["kappa"], kappa_dg), 3, f)


def dp_canon_dg(A, B, Q, R, Qf, N, ns=False):
    """The flag-3 recursion in float64 (ns: with the kernels' Newton–Schulz inverse).  Returns K
    (bt, N−1, m, n) and P1 in original coordinates, the rotated canonical Kt = K_v + A₁, Et, Pt
    (bt, N, n, n), with `setup` (rotated_setup) and `pf` (prefb_setup in the rotated basis)."""
    A, B, Q, R, Qf = (np.asarray(x, dtype=np.float64) for x in (A, B, Q, R, Qf))
    bt, n, m = B.shape
    assert n == 2 * m
    s = rotated_setup(A, B, Q, R, Qf)
    f = pt.prefb_setup(s, A, m)
    Rt, T, S = s["Rt"], s["T"], s["S"]
    sig = s["diag"]["sigma"]
    A22 = f["A2"][:, :, m:]
    P = s["Qft"].copy()
    K = np.zeros((bt, N - 1, m, n))
    Kt = np.zeros((bt, N - 1, m, n))
    Et = np.zeros((bt, N - 1, m, m))
    Pt = np.zeros((bt, N, n, n))
    Pt[:, N - 1] = P
    solve = np.linalg.solve
    if ns:
        inv = ct.NsInverse()
        solve = lambda E, G: _T(inv(E)) @ G
    for k in range(N - 1, 0, -1):
        PA = np.concatenate([P[:, :, m:] * sig[:, None, :], P[:, :, m:] @ A22], axis=2)
        E = Rt + P[:, :m, :m]
        G = f["Mp"] + PA[:, :m]
        Kv = solve(E, G)
        PA2 = PA[:, m:]
        lo = _T(A22) @ PA2                                   # blocks (1, 0) and (1, 1)
        AP = np.zeros_like(P)
        AP[:, :m, :m] = sig[:, :, None] * PA2[:, :, :m]
        AP[:, m:, :m], AP[:, m:, m:] = lo[:, :, :m], lo[:, :, m:]
        AP[:, :m, m:] = _T(lo[:, :, :m])                     # the kernel forms the lower tiles and mirrors
        P = f["Qp"] + AP - _T(G) @ Kv
        P = (P + _T(P)) / 2
        Kt[:, k - 1], Et[:, k - 1], Pt[:, k - 1] = Kv + f["A1"], E, P
        K[:, k - 1] = S @ Kv @ _T(T) + f["C"]
    return dict(K=K, P1=T @ P @ _T(T), Kt=Kt, Et=Et, Pt=Pt, setup=s, pf=f)


def kappa_sweep(family, conds, N, ns=True):
    """The conditioning sweep behind KAPPA_DG_MAX, pt.kappa_sweep's protocol: for each cond(B) in conds
    the worst per-knot relative K error of the Σ-form and of the pre-feedback float64 recursions (ns:
    with the kernels' Newton–Schulz acceptance) against the longdouble reference recursion, and the
    largest κ∞(B₁) of the batch.  Returns rows (cond, kappa, err_diag, err_prefb)."""
    from dp_truth import relerr_per_knot
    from oracle import oracle as orc

    A, B, Q, R, Qf = family
    rows = []
    for c in conds:
        Bc = ct.with_cond(B, c)
        ref = orc.dp_reference(A, Bc, Q, R, Qf, N, dtype=np.longdouble)["K"]
        dg = dp_canon_dg(A, Bc, Q, R, Qf, N, ns=ns)
        pf = pt.dp_canon_pf(A, Bc, Q, R, Qf, N, ns=ns)
        rows.append((c, float(dg["setup"]["kappa"].max()),
                     relerr_per_knot(dg["K"].astype(np.longdouble), ref),
                     relerr_per_knot(pf["K"].astype(np.longdouble), ref)))
    return rows
