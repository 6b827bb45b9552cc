"""numpy model of the canonical recursion with the deadbeat pre-feedback (DESIGN §3.1;
dp_riccati_kernel's VAR_PREFB, the set-up's flag 2), on top of tests/dp_canon_truth.py.

In canonical coordinates B̃ = [I_m; 0], so the input writes the first m state rows directly.  With
A₁ = Ã[0:m, :], A₂ = Ã[m:, :] substitute ũ = v − A₁x̃: the same problem with dynamics [0; A₂] and cost

    Q′ = Q̃ + A₁ᵀR̃A₁      M′ = −R̃A₁      R̃

and the same value function, so P̃_k and Ẽ = R̃ + P̃[0:m, 0:m] are VAR_CANON's.  Per knot

    [G_v; PA₂] = [M′; 0] + P̃[:, m:]·A₂      K_v = Ẽ⁻¹G_v      P̃ ← Q′ + A₂ᵀPA₂ − G_vᵀK_v
    K̃ = K_v + A₁, so K = S·K_v·Tᵀ + C with C = S·A₁·Tᵀ = S·(T₁ᵀA), T₁ the first m columns of T

Q′ carries A₁ᵀR̃A₁, which −G_vᵀK_v cancels again; R̃ = SᵀRS grows like κ(B₁)², so digits are lost in
proportion and the tier is admitted only up to KAPPA_PF_MAX on κ∞(B₁) — the library's
DP_PREFB_KAPPA_F64 (lqrx_internal.h), derived by kappa_sweep() below.
"""
import numpy as np

import dp_canon_truth as ct

KAPPA_PF_MAX = 4.7e2   # = DP_PREFB_KAPPA_F64

_T = ct._T


def prefb_setup(s, A, m):
    """What the set-up adds for a flag-2 trajectory, from canon_setup()'s dict s and the logical A."""
    A1, A2 = s["At"][:, :m], s["At"][:, m:]
    RA = s["Rt"] @ A1
    Qp = s["Qt"] + _T(A1) @ RA
    return dict(A1=A1, A2=A2, Qp=(Qp + _T(Qp)) / 2, Mp=-RA, C=s["S"] @ (_T(s["T"][:, :, :m]) @ A))


def tier(B, kappa_max=ct.KAPPA_MAX, kappa_pf=KAPPA_PF_MAX):
    """(bt,) int: the set-up's flag — 0 generic (rank-deficient, non-finite, κ∞(B₁) past kappa_max),
    2 pre-feedback (κ∞(B₁) ≤ kappa_pf), else 1."""
    z = np.zeros((B.shape[0], B.shape[1], B.shape[1]))
    s = ct.canon_setup(z, B, z, np.zeros((B.shape[0], B.shape[2], B.shape[2])), z)
    with np.errstate(invalid="ignore"):
        ok = ~s["deficient"] & (s["kappa"] <= kappa_max)
        return np.where(ok, np.where(s["kappa"] <= kappa_pf, 2, 1), 0)


def dp_canon_pf(A, B, Q, R, Qf, N, dtype=np.float64, ns=False):
    """The pre-feedback recursion in `dtype` (ns: float64 with the kernels' Newton–Schulz inverse).
    Returns K (bt, N−1, m, n) and P1 in original coordinates, the canonical Kt = K_v + A₁, Et, the
    canonical P̃ of every knot Pt (bt, N, n, n), with `setup` and `pf` (prefb_setup)."""
    dt = np.dtype(dtype).type
    A, B, Q, R, Qf = (np.asarray(x, dtype=dt) for x in (A, B, Q, R, Qf))
    bt, n, m = B.shape
    s = ct.canon_setup(A, B, Q, R, Qf)
    f = prefb_setup(s, A, m)
    Rt, T, S = s["Rt"], s["T"], s["S"]
    P = s["Qft"].copy()
    K = np.zeros((bt, N - 1, m, n), dt)
    Kt = np.zeros((bt, N - 1, m, n), dt)
    Et = np.zeros((bt, N - 1, m, m), dt)
    Pt = np.zeros((bt, N, n, n), dt)
    Pt[:, N - 1] = P
    solve = (lambda E, G: np.linalg.solve(E, G)) if dt is not np.longdouble else \
        (lambda E, G: np.stack([ct._ld_solve(E[t], G[t]) for t in range(bt)]))
    if ns:
        inv = ct.NsInverse()
        solve = lambda E, G: _T(inv(E)) @ G
    for k in range(N - 1, 0, -1):
        PA = P[:, :, m:] @ f["A2"]
        E = Rt + P[:, :m, :m]
        G = f["Mp"] + PA[:, :m]
        Kv = solve(E, G)
        P = f["Qp"] + _T(f["A2"]) @ PA[:, m:] - _T(G) @ Kv
        P = (P + _T(P)) / 2
        Kt[:, k - 1], Et[:, k - 1], Pt[:, k - 1] = Kv + f["A1"], E, P
        K[:, k - 1] = S @ Kv @ _T(T) + f["C"]
    return dict(K=K, P1=T @ P @ _T(T), Kt=Kt, Et=Et, Pt=Pt, setup=s, pf=f)


def kappa_sweep(family, conds, N, ns=True):
    """The conditioning sweep behind KAPPA_PF_MAX, ct.kappa_sweep's protocol: for each cond(B) in conds
    the worst per-knot relative K error of the pre-feedback and of the VAR_CANON float64 recursions
    (ns: with the kernels' Newton–Schulz acceptance) against the longdouble reference recursion, and
    the largest κ∞(B₁) of the batch.  Returns rows (cond, kappa, err_prefb, err_canon)."""
    from dp_truth import relerr_per_knot
    from oracle import oracle as orc

    A, B, Q, R, Qf = family
    rows = []
    for c in conds:
        Bc = ct.with_cond(B, c)
        ref = orc.dp_reference(A, Bc, Q, R, Qf, N, dtype=np.longdouble)["K"]
        pf = dp_canon_pf(A, Bc, Q, R, Qf, N, ns=ns)
        cn = ct.dp_canon(A, Bc, Q, R, Qf, N, ns=ns)
        rows.append((c, float(pf["setup"]["kappa"].max()),
                     relerr_per_knot(pf["K"].astype(np.longdouble), ref),
                     relerr_per_knot(cn["K"].astype(np.longdouble), ref)))
    return rows
