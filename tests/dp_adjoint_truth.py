"""Checkers for the costates and the adjoint pass of the DP solve (lqrx_dp_costates,
lqrx_dp_solve_adjoint; include/lqrx.h).  Not a test file; pinned in tests/test_dp_adjoint.py.

Problem, as in dp_truth: stage cost ½xᵀQ_k x + uᵀM_k x + ½uᵀR_k u + q_kᵀx + r_kᵀu, terminal
½xᵀQf x + qfᵀx, dynamics x_{k+1} = A_k x_k + B_k u_k + c_k, x_1 = x0.  Costates, with the sign
λ_k = ∂V_k/∂x = P_k x_k + p_k (= −lam[k] of dp_truth.dense_kkt):

    λ_N = Qf x_N + qf,      λ_k = Q_k x_k + M_kᵀu_k + q_k + A_kᵀλ_{k+1}

(the project evaluates it in the closed-loop form of costates_logical below, which is the same λ).

Adjoint of a loss ℓ(X, U) with gX = ∂ℓ/∂X, gU = ∂ℓ/∂U: the same problem with q' = gX_k (k < N),
qf' = gX_N, r' = gU_k, c' = 0, x0' = 0 gives X', U', λ'; then

    gA_k = λ'_{k+1} x_kᵀ + λ_{k+1} x'_kᵀ     gB_k = λ'_{k+1} u_kᵀ + λ_{k+1} u'_kᵀ     gc_k = λ'_{k+1}
    gQ_k = ½(x'_k x_kᵀ + x_k x'_kᵀ)          gR_k = ½(u'_k u_kᵀ + u_k u'_kᵀ)          gM_k = u'_k x_kᵀ + u_k x'_kᵀ
    gQf  = ½(x'_N x_Nᵀ + x_N x'_Nᵀ)          gq_k = x'_k    gr_k = u'_k    gqf = x'_N    gx0 = λ'_1

Two checkers:
  (a) dense_adjoint_truth — torch CPU float64 autograd through the dense KKT solve of
      dense_kkt, Q, R, Qf entered as ½(Z + Zᵀ): X, U, λ and the eleven gradients of one problem;
  (b) adjoint_abi — the numpy restatement of the recursion above for a batch of flat ABI arrays, in
      a chosen dtype (what the kernels are compared with).
"""
import numpy as np

from dp_truth import _flat, _mats, dp_solve_abi_np

FIELDS = ("A", "B", "c", "Q", "R", "M", "Qf", "x0", "q", "r", "qf")


def per_knot_problem(d: dict, N: int, b: int) -> dict:
    """Trajectory b of flat ABI arrays d → logical float64 arrays, every per-knot field shaped
    (N−1, …) (time-invariant ones repeated)."""
    n, m, bt = d["n"], d["m"], d["batch"]
    kab = N - 1 if d.get("tv_AB") else 1
    kqr = N - 1 if d.get("tv_QR") else 1
    rep = lambda a, k: np.repeat(a, N - 1, axis=0) if k == 1 else a
    f8 = np.float64
    return dict(
        A=rep(_mats(d["A"], bt, kab, n, n, f8)[b], kab), B=rep(_mats(d["B"], bt, kab, n, m, f8)[b], kab),
        c=rep(np.asarray(d["c"], f8).reshape(bt, kab, n)[b], kab),
        Q=rep(_mats(d["Q"], bt, kqr, n, n, f8)[b], kqr), R=rep(_mats(d["R"], bt, kqr, m, m, f8)[b], kqr),
        M=rep(_mats(d["M"], bt, kqr, m, n, f8)[b], kqr), Qf=_mats(d["Qf"], bt, 1, n, n, f8)[b, 0],
        x0=np.asarray(d["x0"], f8).reshape(bt, n)[b],
        q=rep(np.asarray(d["q"], f8).reshape(bt, kqr, n)[b], kqr),
        r=rep(np.asarray(d["r"], f8).reshape(bt, kqr, m)[b], kqr), qf=np.asarray(d["qf"], f8).reshape(bt, n)[b])


def dense_adjoint_truth(p: dict, N: int, gX: np.ndarray, gU: np.ndarray) -> dict:
    """Checker (a).  p: per_knot_problem arrays; gX (N, n), gU (N−1, m).  Returns X, U, lam (the
    costates λ_k, (N, n)) and g = {field: gradient of ℓ = Σ gX·X + Σ gU·U}, every per-knot field's
    gradient shaped (N−1, …)."""
    import torch

    t = {k: torch.tensor(np.asarray(p[k], np.float64), dtype=torch.float64, requires_grad=True) for k in FIELDS}
    n, m = p["B"].shape[-2:]
    sym = lambda Z: 0.5 * (Z + Z.transpose(-1, -2))
    Q, R, Qf = sym(t["Q"]), sym(t["R"]), sym(t["Qf"])
    nz = N * n + (N - 1) * m
    ix = lambda k: slice(k * (n + m), k * (n + m) + n)
    iu = lambda k: slice(k * (n + m) + n, k * (n + m) + n + m)
    H = torch.zeros(nz, nz, dtype=torch.float64)
    g = torch.zeros(nz, dtype=torch.float64)
    D = torch.zeros(N * n, nz, dtype=torch.float64)
    rhs = torch.zeros(N * n, dtype=torch.float64)
    eye = torch.eye(n, dtype=torch.float64)
    for k in range(N - 1):   # slice assignments are differentiable copies
        H[ix(k), ix(k)] = Q[k]
        H[iu(k), iu(k)] = R[k]
        H[iu(k), ix(k)] = t["M"][k]
        H[ix(k), iu(k)] = t["M"][k].T
        g[ix(k)] = t["q"][k]
        g[iu(k)] = t["r"][k]
    H[ix(N - 1), ix(N - 1)] = Qf
    g[ix(N - 1)] = t["qf"]
    D[0:n, ix(0)] = eye
    rhs[0:n] = t["x0"]
    for k in range(N - 1):
        rows = slice((k + 1) * n, (k + 2) * n)
        D[rows, ix(k + 1)] = eye
        D[rows, ix(k)] = -t["A"][k]
        D[rows, iu(k)] = -t["B"][k]
        rhs[rows] = t["c"][k]
    Kkt = torch.cat([torch.cat([H, D.T], 1), torch.cat([D, torch.zeros(N * n, N * n, dtype=torch.float64)], 1)], 0)
    sol = torch.linalg.solve(Kkt, torch.cat([-g, rhs]))
    z = sol[:nz]
    X = torch.stack([z[ix(k)] for k in range(N)])
    U = torch.stack([z[iu(k)] for k in range(N - 1)])
    loss = (X * torch.tensor(np.asarray(gX, np.float64))).sum() + (U * torch.tensor(np.asarray(gU, np.float64))).sum()
    grads = torch.autograd.grad(loss, [t[k] for k in FIELDS])
    return dict(X=X.detach().numpy(), U=U.detach().numpy(), lam=-sol[nz:].reshape(N, n).detach().numpy(),
                g={k: v.numpy() for k, v in zip(FIELDS, grads)})


def costates_logical(A, B, Q, R, M, Qf, q, r, qf, K, X, U, dtype=np.float64):
    """The project's costate recursion on logical batch arrays: A (bt, kab, n, n), B (bt, kab, n, m),
    Q (bt, kqr, n, n), R (bt, kqr, m, m), M (bt, kqr, m, n), Qf (bt, n, n), q (bt, kqr, n),
    r (bt, kqr, m), qf (bt, n), K (bt, N−1, m, n), X (bt, N, n), U (bt, N−1, m); a knot axis of length
    1 is time-invariant.  Returns lam (bt, N, n), every operation in dtype.

        s_k = R_k u_k + M_k x_k + r_k + B_kᵀλ_{k+1}            (stationarity: zero at the solution)
        λ_k = Q_k x_k + M_kᵀu_k + q_k + A_kᵀλ_{k+1} − K_kᵀ s_k

    the textbook sweep plus K_kᵀ times a quantity that is zero in exact arithmetic, so that rounding
    errors propagate through the stable closed loop (A − BK)ᵀ instead of the open-loop Aᵀ."""
    dt = dtype
    A, B, Q, R, M, Qf, q, r, qf, K, X, U = (np.asarray(a, dt) for a in (A, B, Q, R, M, Qf, q, r, qf, K, X, U))
    bt, N, n = X.shape
    T = lambda Z: np.swapaxes(Z, -1, -2)
    mv = lambda Z, v: (Z @ v[..., None])[..., 0]
    lam = np.zeros((bt, N, n), dt)
    lam[:, N - 1] = mv(Qf, X[:, N - 1]) + qf
    for k in range(N - 1, 0, -1):
        at = lambda Z: Z[:, (k - 1) % Z.shape[1]]
        x, u, ln = X[:, k - 1], U[:, k - 1], lam[:, k]
        s = mv(at(R), u) + mv(at(M), x) + at(r) + mv(T(at(B)), ln)
        lam[:, k - 1] = mv(at(Q), x) + mv(T(at(M)), u) + at(q) + mv(T(at(A)), ln) - mv(T(K[:, k - 1]), s)
    return lam


def costates_textbook(A, Q, M, Qf, q, qf, X, U, dtype=np.float64):
    """The open-loop sweep λ_k = Q_k x_k + M_kᵀu_k + q_k + A_kᵀλ_{k+1}: equal to costates_logical in
    exact arithmetic, kept to show what it loses on a long horizon (tests/test_dp_adjoint.py)."""
    dt = dtype
    A, Q, M, Qf, q, qf, X, U = (np.asarray(a, dt) for a in (A, Q, M, Qf, q, qf, X, U))
    bt, N, n = X.shape
    mv = lambda Z, v: (Z @ v[..., None])[..., 0]
    lam = np.zeros((bt, N, n), dt)
    lam[:, N - 1] = mv(Qf, X[:, N - 1]) + qf
    for k in range(N - 1, 0, -1):
        at = lambda Z: Z[:, (k - 1) % Z.shape[1]]
        lam[:, k - 1] = (mv(at(Q), X[:, k - 1]) + mv(np.swapaxes(at(M), -1, -2), U[:, k - 1]) + at(q)
                         + mv(np.swapaxes(at(A), -1, -2), lam[:, k]))
    return lam


def adjoint_abi(d: dict, N: int, gX, gU, dtype=np.float64) -> dict:
    """Checker (b).  d: flat ABI arrays as for dp_truth.dp_solve_abi_np (tv_AB / tv_QR optional); gX
    (bt, N, n), gU (bt, N−1, m).  Runs the forward solve, its costates, the adjoint solve, its
    costates and the formulas, every operation in `dtype`.  Returns logical arrays: X, U, lam, Xa,
    Ua, lama, info, and g = {field: gradient}: gA, gB, gc per knot (bt, N−1, …) with tv_AB, else summed
    over the knots (bt, …); gQ, gR, gM, gq, gr always per knot (bt, N−1, …)."""
    dt = dtype
    n, m, bt = d["n"], d["m"], d["batch"]
    kab = N - 1 if d.get("tv_AB") else 1
    kqr = N - 1 if d.get("tv_QR") else 1
    gX = np.asarray(gX, dt).reshape(bt, N, n)
    gU = np.asarray(gU, dt).reshape(bt, N - 1, m)
    A = _mats(d["A"], bt, kab, n, n, dt)
    Q = _mats(d["Q"], bt, kqr, n, n, dt)
    R = _mats(d["R"], bt, kqr, m, m, dt)
    M = _mats(d["M"], bt, kqr, m, n, dt)
    Qf = _mats(d["Qf"], bt, 1, n, n, dt)[:, 0]
    q = np.asarray(d["q"], dt).reshape(bt, kqr, n)
    qf = np.asarray(d["qf"], dt).reshape(bt, n)
    B = _mats(d["B"], bt, kab, n, m, dt)
    r = np.asarray(d["r"], dt).reshape(bt, kqr, m)
    fwd = dp_solve_abi_np(d, N, "cross", dtype=dt)
    X, U = fwd["X"].reshape(bt, N, n), fwd["U"].reshape(bt, N - 1, m)
    lam = costates_logical(A, B, Q, R, M, Qf, q, r, qf, _mats(fwd["K"], bt, N - 1, m, n, dt), X, U, dt)
    # the adjoint problem: per-knot cost terms (Q, R, M broadcast when time-invariant), q' r' qf' from gX gU
    bc = lambda Z: np.ascontiguousarray(np.broadcast_to(Z, (bt, N - 1) + Z.shape[2:]))
    da = dict(d)
    da.update(Q=_flat(bc(Q)), R=_flat(bc(R)), M=_flat(bc(M)), tv_QR=1,
              q=np.ascontiguousarray(gX[:, :N - 1]).ravel(), r=gU.ravel(),
              qf=np.ascontiguousarray(gX[:, N - 1]).ravel(), c=np.zeros(bt * kab * n, dt), x0=np.zeros(bt * n, dt))
    adj = dp_solve_abi_np(da, N, "cross", dtype=dt)
    Xa, Ua = adj["X"].reshape(bt, N, n), adj["U"].reshape(bt, N - 1, m)
    lama = costates_logical(A, B, Q, R, M, Qf, gX[:, :N - 1], gU, gX[:, N - 1],
                            _mats(adj["K"], bt, N - 1, m, n, dt), Xa, Ua, dt)
    outer = lambda a, b: a[..., :, None] * b[..., None, :]
    x, xa, l1, la1 = X[:, :N - 1], Xa[:, :N - 1], lam[:, 1:], lama[:, 1:]
    half = dt(0.5)
    g = dict(A=outer(la1, x) + outer(l1, xa), B=outer(la1, U) + outer(l1, Ua), c=la1.copy(),
             Q=half * (outer(xa, x) + outer(x, xa)), R=half * (outer(Ua, U) + outer(U, Ua)),
             M=outer(Ua, x) + outer(U, xa),
             Qf=half * (outer(Xa[:, N - 1], X[:, N - 1]) + outer(X[:, N - 1], Xa[:, N - 1])),
             x0=lama[:, 0].copy(), q=xa.copy(), r=Ua.copy(), qf=Xa[:, N - 1].copy())
    if kab == 1:   # ascending k, as the kernel adds them
        for k in ("A", "B", "c"):
            acc = np.zeros_like(g[k][:, 0])
            for j in range(N - 1):
                acc = acc + g[k][:, j]
            g[k] = acc
    return dict(X=X, U=U, lam=lam, Xa=Xa, Ua=Ua, lama=lama, info=fwd["info"], info_adj=adj["info"], g=g)


VECTOR_GRADS = ("c", "x0", "q", "r", "qf")     # direct outputs of the adjoint solve: bound TOL
MATRIX_GRADS = ("A", "B", "Q", "R", "M", "Qf")  # two products of such quantities: bound 4·TOL


def grad_errors(got: dict, ref: dict) -> dict:
    """Error of every gradient in got ({field: (bt, …)}) against ref (an adjoint_abi result), the
    worst trajectory's max|got − ref| over that trajectory's scale:
      lam (key "lam" in got) and the vector gradients: the largest entry of the trajectory they are
      entries of — λ for lam, λ' for gc and gx0, X' for gq and gqf, U' for gr;
      matrix gradients: the scale of their two terms — gA: max|λ'|·max|x| + max|λ|·max|x'|,
      gB: … u, u'; gQ, gQf: max|x'|·max|x|; gR: max|u'|·max|u|; gM: max|u'|·max|x| + max|u|·max|x'|
      (maxima over the trajectory) — times N−1 where the output is a sum over the knots."""
    bt = ref["X"].shape[0]
    mx = lambda a: np.abs(np.asarray(a, np.float64)).reshape(bt, -1).max(axis=1)
    x, u, l, xa, ua, la = (mx(ref[k]) for k in ("X", "U", "lam", "Xa", "Ua", "lama"))
    N = ref["X"].shape[1]
    summed = ref["g"]["A"].ndim == 3   # (bt, n, n): summed over the knots
    ks = (N - 1) if summed else 1
    scale = dict(A=ks * (la * x + l * xa), B=ks * (la * u + l * ua), Q=xa * x, Qf=xa * x, R=ua * u,
                 M=ua * x + u * xa,
                 # the vector gradients are entries of the adjoint trajectories X', U', λ'
                 lam=l, c=ks * la, x0=la, q=xa, r=ua, qf=xa)
    out = {}
    for k, v in got.items():
        r = ref["lam"] if k == "lam" else ref["g"][k]
        num = np.abs(np.asarray(v, np.float64).reshape(bt, -1) - np.asarray(r, np.float64).reshape(bt, -1)).max(axis=1)
        den = scale[k] if k in scale else mx(r)
        den = np.where(den == 0, 1.0, den)
        out[k] = float((num / den).max())
    return out


def check_grads(got: dict, ref: dict, tol: float, what: str = "") -> dict:
    """Prints every figure of grad_errors, then asserts: vector gradients and lam ≤ tol, matrix
    gradients ≤ 4·tol."""
    e = grad_errors(got, ref)
    print(what, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v <= (4 * tol if k in MATRIX_GRADS else tol), (what, k, v)
    return e


def sum_truth_like(ga: dict, d: dict) -> dict:
    """Checker (a)'s per-knot gradients → the shapes adjoint_abi returns for d: gA, gB, gc summed
    over the knots when A is time-invariant.  (Q, R, M, q, r stay per knot.)"""
    out = dict(ga)
    if not d.get("tv_AB"):
        for k in ("A", "B", "c"):
            out[k] = ga[k].sum(axis=0)
    return out
