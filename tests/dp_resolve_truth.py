"""Checker for lqrx_dp_factor / lqrx_dp_resolve (include/lqrx.h): the re-solve recursion on flat ABI
arrays in a given dtype, and the shapes its tests run.  Not a test file; pinned in
tests/test_dp_resolve.py against dp_truth.dp_solve_abi_np(kind="cross", all_P=True).

With the solve's recursion as dp_truth states it and g_k = P_{k+1}c_k, K_k, E_k⁻¹, g_k fixed per problem,
a right-hand side (q, r, qf, x0) needs

    p_N = qf
    p̃   = p_{k+1} + g_k         h_k = r_k + B_kᵀp̃         d_k = E_k⁻¹h_k
    p_k = q_k + A_kᵀp̃ − K_kᵀh_k                                          k = N−1 … 1
    x_1 = x0,  u_k = −K_k x_k − d_k,  x_{k+1} = A_k x_k + B_k u_k + c_k      k = 1 … N−1

(Gᵀd = GᵀE⁻¹h = Kᵀh because E is symmetric; no cost matrix is read.)  Trajectory t = b·S + j,
scenario-major as in lqrx_dp_scenarios.
"""
import numpy as np

from dp_truth import F32_SHAPES, _flat, _mats

# (n, m, N, batch, tv): a subset of dp_truth.PARITY within n ≤ 64, m ≤ 32
SHAPES = [(1, 1, 6, 3, False), (4, 1, 40, 8, False), (6, 3, 30, 7, False), (17, 5, 12, 3, True),
          (32, 16, 40, 4, False), (24, 18, 10, 3, False), (64, 32, 12, 2, False), (48, 16, 10, 2, True),
          (32, 16, 256, 2, True)]
__all__ = ["SHAPES", "F32_SHAPES", "factor_np", "resolve_np", "random_rhs", "xu_error"]


def factor_np(d: dict, N: int, P, dtype=np.float64) -> dict:
    """d: flat ABI B, R and optionally c (None: no Pc), n, m, batch, tv_AB / tv_QR; P flat, every P_k
    (n·n·N per problem).  Returns flat ABI Einv (m·m·(N−1) per problem), Pc (n·(N−1) per problem, or
    None) and info (the largest 1-based knot whose symmetrised E has a non-positive eigenvalue)."""
    n, m, bt = d["n"], d["m"], d["batch"]
    kab = N - 1 if d.get("tv_AB") else 1
    kqr = N - 1 if d.get("tv_QR") else 1
    dt = dtype
    B = _mats(d["B"], bt, kab, n, m, dt)
    R = _mats(d["R"], bt, kqr, m, m, dt)
    Ps = _mats(P, bt, N, n, n, dt)
    c = None if d.get("c") is None else np.asarray(d["c"], dt).reshape(bt, kab, n)
    Einv = np.zeros((bt, N - 1, m, m), dt)
    Pc = None if c is None else np.zeros((bt, N - 1, n), dt)
    info = np.zeros(bt, np.int32)
    for k in range(N - 1, 0, -1):
        Bk, Rk, Pn = B[:, (k - 1) % kab], R[:, (k - 1) % kqr], Ps[:, k]
        E = Rk + np.swapaxes(Bk, -1, -2) @ (Pn @ Bk)
        for t in range(bt):
            if info[t] == 0 and not np.linalg.eigvalsh(((E[t] + E[t].T) / 2).astype(np.float64)).min() > 0:
                info[t] = k
        Einv[:, k - 1] = np.linalg.inv(E)
        if c is not None:
            Pc[:, k - 1] = (Pn @ c[:, (k - 1) % kab][..., None])[..., 0]
    return dict(Einv=_flat(Einv), Pc=None if Pc is None else Pc.ravel(), info=info)


def resolve_np(d: dict, N: int, K, Einv, Pc, S: int, q=None, r=None, qf=None, x0=None, tv_QR: int = 0,
               dtype=np.float64) -> dict:
    """d: flat ABI A, B and optionally c, n, m, batch, tv_AB.  K, Einv, Pc: flat ABI factors (Pc None
    exactly when d has no c).  q, r, qf, x0: flat, scenario-major, None for zero; q and r carry a knot
    axis with tv_QR.  Returns logical d (bt, S, N−1, m), p (bt, S, N, n: every p_k, p_N = qf),
    X (bt, S, N, n), U (bt, S, N−1, m), every operation in `dtype`."""
    n, m, bt = d["n"], d["m"], d["batch"]
    kab = N - 1 if d.get("tv_AB") else 1
    kq = N - 1 if tv_QR else 1
    dt = dtype
    A = _mats(d["A"], bt, kab, n, n, dt)
    B = _mats(d["B"], bt, kab, n, m, dt)
    c = None if d.get("c") is None else np.asarray(d["c"], dt).reshape(bt, kab, n)
    assert (c is None) == (Pc is None)
    Ks = _mats(K, bt, N - 1, m, n, dt)
    Ei = _mats(Einv, bt, N - 1, m, m, dt)
    g = None if Pc is None else np.asarray(Pc, dt).reshape(bt, N - 1, n)
    vec = lambda a, k, w: np.zeros((bt, S, k, w), dt) if a is None else np.asarray(a, dt).reshape(bt, S, k, w)
    q, r = vec(q, kq, n), vec(r, kq, m)
    qf, x0 = vec(qf, 1, n)[:, :, 0], vec(x0, 1, n)[:, :, 0]
    # (bt, r, c) matrix times (bt, S, c) vectors
    mv = lambda Z, v: np.einsum("bij,bsj->bsi", Z, v)
    mtv = lambda Z, v: np.einsum("bji,bsj->bsi", Z, v)
    ds = np.zeros((bt, S, N - 1, m), dt)
    ps = np.zeros((bt, S, N, n), dt)
    ps[:, :, N - 1] = p = qf
    for k in range(N - 1, 0, -1):
        Ak, Bk = A[:, (k - 1) % kab], B[:, (k - 1) % kab]
        pt = p if g is None else p + g[:, None, k - 1]
        h = r[:, :, (k - 1) % kq] + mtv(Bk, pt)
        ds[:, :, k - 1] = mv(Ei[:, k - 1], h)
        p = q[:, :, (k - 1) % kq] + mtv(Ak, pt) - mtv(Ks[:, k - 1], h)
        ps[:, :, k - 1] = p
    X = np.zeros((bt, S, N, n), dt)
    U = np.zeros((bt, S, N - 1, m), dt)
    X[:, :, 0] = x0
    for k in range(1, N):
        Ak, Bk = A[:, (k - 1) % kab], B[:, (k - 1) % kab]
        U[:, :, k - 1] = -mv(Ks[:, k - 1], X[:, :, k - 1]) - ds[:, :, k - 1]
        X[:, :, k] = mv(Ak, X[:, :, k - 1]) + mv(Bk, U[:, :, k - 1])
        if c is not None:
            X[:, :, k] += c[:, None, (k - 1) % kab]
    return dict(d=ds, p=ps, X=X, U=U)


def random_rhs(n, m, N, bt, S, seed, tv_QR):
    """S right-hand sides per problem, q, r, qf, x0 ~ N(0, 1), flat and scenario-major."""
    rng = np.random.default_rng(seed)
    kq = N - 1 if tv_QR else 1
    return dict(q=rng.standard_normal(bt * S * kq * n), r=rng.standard_normal(bt * S * kq * m),
                qf=rng.standard_normal(bt * S * n), x0=rng.standard_normal(bt * S * n))


def xu_error(a, b):
    """dp_truth.check's measure for X and U: max|a − b| / max(1, max|b|)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a.reshape(b.shape) - b).max() / max(1.0, np.abs(b).max()))
