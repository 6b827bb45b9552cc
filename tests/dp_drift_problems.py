"""Problem families that walk the Riccati kernels' Newton–Schulz acceptance rule through all of
its paths, and a numpy restatement of that rule (lqrx_dp.hip: NsTol / ns_round / ns_refine).  A plain module: tests/test_dp_ns_census.py pins the paths the
committed seeds reach (no device), tests/test_dp_ns_regimes_gpu.py runs the kernels on them.

Every family starts from lqrx.random_batch (the library's generator: R = I + GGᵀ/m, Qf = 10 Q)
and gives every trajectory of the batch a parameter of its own, so one launch covers a sweep:

  drift  per-knot data that moves by a few 1e-6 … 1e-1 per knot, as successive linearisations
         along a trajectory do.  form "scalar": R_k = R0·(1 + a_k);  "rank1": R_k = R0 +
         a_k·(8/m)·11ᵀ (both tv_QR = 1, Q_k = Q);  "B": B_k = B·(1 + a_k) (tv_AB = 1, A_k = A).
         a_k uniform in ±δ_t, δ_t = DELTAS[dtype][t].  Qf = P∞ of the undrifted problem.
  jump   R_k = R0 for k > j_t and 100·R0 for k ≤ j_t;  B_k = B for k > i_t and −B for k ≤ i_t
         (tv_QR = tv_AB = 1): a rejection in the middle of the horizon and the warm restart after
         it.  Qf = P∞ of the problem before the jump.
  cond   time-invariant, m > n, R ← ε_t·R: BᵀPB has rank ≤ n < m, so cond(E) ≈ 1e1/ε_t; per ε one
         trajectory with Qf = 10 Q (transient) and one with Qf = P∞ (stationary).

The rule, per knot k = N−2 … 1 (knot N−1 always takes the exact sweep):
    X ← 2·X_{k+1} − X_{k+2}   (X_{k+2} := X_{k+1} at k = N−2; the X's are the ones the knots ended with)
    up to 6 rounds:  ρ = 16·MT·max|I − EᵀX|
                     ρ ≤ v → accept;  !(ρ < 1) → reject;  X ← X + Xᵀ(I − EᵀX);  ρ ≤ one_step → accept
    no verdict after 6 rounds (cap), or a reject: X = E⁻¹ exactly (the LDLᵀ sweep).
The restatement runs in the working precision, out of place, with numpy's summation order; the
kernel updates in place and sums in MFMA order.  So a knot counts toward a path in the census only
if every ρ it looked at is a factor ≥ MARGIN away from every threshold it was compared with.
"""
import numpy as np

NS_TOL = {0: (1e-11, 1e-9), 1: (3e-4, 1e-5)}        # NsTol<double>, NsTol<float>: (v, one_step)
NS_ROUNDS = 6
MARGIN = 4.0
# drift per knot; the eighth value is the one at which, by the restatement below, first residuals
# land where no decade of the list puts them: fp64 between v and one_step (ρ0 ≈ 1e-10), fp32 just
# under v (ρ0 in (v/2, v] at several knots of every form — the loosest X the rule accepts)
DELTAS = {0: (0.0, 1e-6, 1e-4, 1e-3, 1e-2, 3e-2, 1e-1, 3e-12), 1: (0.0, 1e-6, 1e-4, 1e-3, 1e-2, 3e-2, 1e-1, 5e-5)}
RANK1_EIG = 8.0     # the rank-one drift is a_k·(8/m)·11ᵀ: eigenvalue 8·a_k ≥ −0.8 > −λmin(R0) = −1, R_k stays SPD
EPS = {0: (1.0, 1e-2, 1e-4, 1e-6), 1: (1.0, 1e-1, 1e-2)}
NPDT = {0: np.float64, 1: np.float32}

# paths of the rule
FIRST, ACCEPT0, ONE_STEP, ROUNDS, REJECT, CAP = "first", "accept0", "one_step", "rounds", "reject", "cap"
# ONE_STEP is a path only where one_step > v: in fp32 (v = 3e-4 > one_step = 1e-5) a ρ that fails
# ρ ≤ v fails ρ ≤ one_step too, so the test after the update never accepts.


def _logical(lqrx, n, m, N, bt, seed):
    from lqrx.dp import abi_to_batch

    b = abi_to_batch(lqrx.random_batch(n, m, N, bt, seed))
    return {k: np.array(getattr(b, k), dtype=np.float64) for k in ("A", "B", "Q", "R", "Qf", "x0")}


def stationary_P(A, B, Q, R):
    """The stabilising solution of the discrete algebraic Riccati equation per trajectory: the
    fixed point of the recursion, so Qf = P∞ makes the unperturbed problem stationary (E_k the
    same at every knot) from the first knot on."""
    from scipy.linalg import solve_discrete_are

    P = np.stack([solve_discrete_are(a, b, q, r) for a, b, q, r in zip(A, B, Q, R)])
    return (P + np.swapaxes(P, 1, 2)) / 2


def _knots(M, N):
    return np.repeat(M[:, None], N - 1, axis=1)


def drift(lqrx, n, m, N, seed, form="scalar", dtype=0):
    """One trajectory per δ in DELTAS[dtype]; Qf = P∞ of the undrifted problem, so what moves E
    from knot to knot is the drift alone (with Qf = 10 Q the transient of P itself moves E by
    percents per knot over a short horizon and buries every δ ≤ 1e-3).  Returns a dict of logical
    float64 arrays (knot axis on the drifting fields) plus N, family, form and the per-trajectory
    parameter `param`."""
    deltas = DELTAS[dtype]
    bt = len(deltas)
    p = _logical(lqrx, n, m, N, bt, seed)
    p["Qf"] = stationary_P(p["A"], p["B"], p["Q"], p["R"])
    rng = np.random.default_rng(seed + 1000)
    a = (2.0 * rng.random((bt, N - 1)) - 1.0) * np.asarray(deltas)[:, None]
    if form == "scalar":
        p["R"] = _knots(p["R"], N) * (1.0 + a)[:, :, None, None]
        p["Q"] = _knots(p["Q"], N)
    elif form == "rank1":
        p["R"] = _knots(p["R"], N) + a[:, :, None, None] * (RANK1_EIG / m) * np.ones((m, m))
        p["Q"] = _knots(p["Q"], N)
    elif form == "B":
        p["B"] = _knots(p["B"], N) * (1.0 + a)[:, :, None, None]
        p["A"] = _knots(p["A"], N)
    else:
        raise ValueError(form)
    p.update(N=N, family="drift", form=form, param=np.asarray(deltas, dtype=np.float64))
    return p


def jump(lqrx, n, m, N, seed, bt=6):
    """R ×100 at knots k ≤ j_t, B → −B at knots k ≤ i_t; j_t, i_t strictly inside the horizon and
    different for every trajectory (knot k sits at index k − 1 of the knot axis).  Qf = P∞ of the
    problem before the jump: stationary down to the jump, a transient after it.  (E = R + BᵀPB does
    not see the sign of B: the flip exercises the kernels' per-knot B and the sign of K, not the
    iteration.)"""
    p = _logical(lqrx, n, m, N, bt, seed)
    p["Qf"] = stationary_P(p["A"], p["B"], p["Q"], p["R"])
    rng = np.random.default_rng(seed + 2000)
    inner = np.arange(3, N - 3)                                   # 3 … N−4: knots on both sides
    j = rng.permutation(inner)[:bt]
    i = rng.permutation(inner)[:bt]
    assert len(j) == bt and len(set(j)) == bt and len(set(i)) == bt
    k = np.arange(1, N)[None, :]
    p["R"] = _knots(p["R"], N) * np.where(k <= j[:, None], 100.0, 1.0)[:, :, None, None]
    p["Q"] = _knots(p["Q"], N)
    p["B"] = _knots(p["B"], N) * np.where(k <= i[:, None], -1.0, 1.0)[:, :, None, None]
    p["A"] = _knots(p["A"], N)
    p.update(N=N, family="jump", form="jump", param=np.stack([j, i], axis=1).astype(np.float64))
    return p


def cond(lqrx, n, m, N, seed, dtype):
    """Time-invariant, m > n, R ← ε·R; two trajectories per ε of EPS[dtype]: the first keeps the
    generator's Qf = 10 Q (a transient: E moves at every knot), the second takes Qf = P∞ of its
    own problem (stationary: the warm start's residual sits at the rounding floor of that cond(E))."""
    assert m > n
    eps = np.repeat(np.asarray(EPS[dtype]), 2)
    p = _logical(lqrx, n, m, N, len(eps), seed)
    p["R"] = p["R"] * eps[:, None, None]
    p["Qf"][1::2] = stationary_P(p["A"][1::2], p["B"][1::2], p["Q"][1::2], p["R"][1::2])
    p.update(N=N, family="cond", form="cond", param=eps)
    return p


def with_linear(p, seed, affine=False):
    """q, r, qf (and c with `affine`) standard normal; q, r follow Q, R and c follows A, B."""
    rng = np.random.default_rng(seed + 3000)
    bt, n, m = p["B"].shape[0], p["B"].shape[-2], p["B"].shape[-1]
    N = p["N"]
    kq = (N - 1,) if p["Q"].ndim == 4 else ()
    kab = (N - 1,) if p["A"].ndim == 4 else ()
    p = dict(p, q=rng.standard_normal((bt, *kq, n)), r=rng.standard_normal((bt, *kq, m)),
             qf=rng.standard_normal((bt, n)))
    if affine:
        p["c"] = rng.standard_normal((bt, *kab, n))
    return p


def rounded(p, dtype):
    """The problem the kernel sees in `dtype`: every array rounded to it (and held in float64)."""
    t = NPDT[dtype]
    return {k: (np.asarray(v, dtype=t).astype(np.float64) if isinstance(v, np.ndarray) and k != "param" else v)
            for k, v in p.items()}


def to_batch(p):
    from lqrx.dp import LQRBatch

    return LQRBatch(p["A"], p["B"], p["Q"], p["R"], p["Qf"], p["x0"], p["N"],
                    q=p.get("q"), r=p.get("r"), qf=p.get("qf"), c=p.get("c"))


def reference(oracle, p, dtype):
    """oracle.dp_reference of the problem in `dtype` (a numpy type)."""
    return oracle.dp_reference(p["A"], p["B"], p["Q"], p["R"], p["Qf"], p["N"], q=p.get("q"), r=p.get("r"),
                               qf=p.get("qf"), c=p.get("c"), x0=p["x0"], dtype=dtype)


def per_knot_relerr(a, b):
    """(batch, knots) max|a − b| / max|b| per trajectory and knot, formed in b's precision
    (the project's per-knot measure, tests/test_dp_knot_gpu.py)."""
    b = np.asarray(b)
    a = np.asarray(a, dtype=b.dtype).reshape(b.shape[0], b.shape[1], -1)
    b = b.reshape(b.shape[0], b.shape[1], -1)
    den = np.abs(b).max(axis=2)
    den[den == 0] = 1.0
    return (np.abs(a - b).max(axis=2) / den).astype(np.float64)


def per_traj_relerr(a, b):
    """(batch,) the worst knot of per_knot_relerr."""
    return per_knot_relerr(a, b).max(axis=1)


def kernel_mt(n, m):
    """MT of the tile grid dp_launch picks for 5 ≤ n ≤ 64, m ≤ 32 (the smallest instantiated grid
    that covers (n, m): 1×1, 2×1, 2×2, then 4×2 — so n = 48, m = 16 runs with MT = 2; the padding
    is a unit diagonal and adds nothing to the residual).  n = 64, m = 16 in fp64 (dp_wg4_kernel,
    MT = 1) is not among the cases."""
    nt, mt = (n + 15) // 16, (m + 15) // 16
    assert 5 <= n <= 64 and m <= 32 and not (n == 64 and m == 16)
    return mt if nt <= 2 else 2


def ns_paths(p, P, dtype):
    """The acceptance rule restated.  p: a problem (already `rounded` to the working precision),
    P: its cost-to-go (batch, N, n, n) from the float64 reference, dtype 0 / 1.  Returns
    path (batch, N−1) of strings (index k − 1 = knot k), rounds (batch, N−1) — the number of
    updates X ← X + XᵀR the knot took —, rho0 (batch, N−1) — the first ρ (nan at knot N−1) —,
    clear (batch, N−1) bool — every ρ the knot looked at is a factor ≥ MARGIN from every threshold
    it was compared with — and condE (batch, N−1)."""
    t = NPDT[dtype]
    v, one_step = (t(x) for x in NS_TOL[dtype])
    N = p["N"]
    bt, m = p["B"].shape[0], p["B"].shape[-1]
    scale = t(16 * kernel_mt(p["B"].shape[-2], m))
    at = lambda M, tr, k: M[tr, k - 1] if M.ndim == 4 else M[tr]
    path = np.empty((bt, N - 1), dtype=object)
    rounds = np.zeros((bt, N - 1), np.int32)
    rho0 = np.full((bt, N - 1), np.nan)
    clear = np.ones((bt, N - 1), bool)
    condE = np.zeros((bt, N - 1))
    I = np.eye(m, dtype=t)

    def far(rho, thr):
        return not (thr / MARGIN < rho < thr * MARGIN)

    for tr in range(bt):
        X = Xp = None
        for k in range(N - 1, 0, -1):
            B, R = at(p["B"], tr, k), at(p["R"], tr, k)
            E64 = R + B.T @ P[tr, k] @ B                     # P[tr, k] = P_{k+1} (0-based index k)
            E64 = (E64 + E64.T) / 2
            condE[tr, k - 1] = np.linalg.cond(E64)
            E = E64.astype(t)
            exact = np.linalg.inv(E.astype(np.float64)).astype(t)
            if k == N - 1:
                path[tr, k - 1] = FIRST
                X = Xp = exact
                continue
            X1 = X
            X = t(2) * X - Xp
            Xp = X1
            verdict, ok = None, True
            for it in range(NS_ROUNDS):
                Rs = I - E.T @ X
                with np.errstate(over="ignore", invalid="ignore"):
                    rho = scale * np.abs(Rs).max()
                if it == 0:
                    rho0[tr, k - 1] = rho
                ok = ok and far(rho, v)
                if rho <= v:
                    verdict = ACCEPT0 if it == 0 else ROUNDS
                    break
                ok = ok and far(rho, t(1))
                if not rho < 1:
                    verdict = REJECT
                    break
                X = X + X.T @ Rs
                rounds[tr, k - 1] += 1
                ok = ok and far(rho, one_step)
                if rho <= one_step:
                    verdict = ONE_STEP if it == 0 else ROUNDS
                    break
            if verdict is None:
                verdict = CAP
            if verdict in (REJECT, CAP):
                X = exact
            path[tr, k - 1] = verdict
            clear[tr, k - 1] = ok
    return dict(path=path, rounds=rounds, rho0=rho0, clear=clear, condE=condE)


def census(res):
    """{path: number of knots that took it with the margin} plus "rounds2": knots accepted after
    two or more updates (with the margin)."""
    out = {}
    for name in (ACCEPT0, ONE_STEP, ROUNDS, REJECT, CAP):
        out[name] = int(((res["path"] == name) & res["clear"]).sum())
    out["rounds2"] = int(((res["path"] == ROUNDS) & res["clear"] & (res["rounds"] >= 2)).sum())
    return out


# ------------------------------------------------------------------ the committed cases
# One case = one launch: (family, form, n, m, N, dtype, entry); entry "plain" (lqrx_dp_solve),
# "linear" (lqrx_dp_solve_linear) or "affine" (lqrx_dp_solve_affine).  The census test
# (tests/test_dp_ns_census.py) asserts what these reach, the GPU tests
# (tests/test_dp_ns_regimes_gpu.py) run them.
DRIFT_FORMS = ("scalar", "rank1", "B")
GRIDS = {
    # fp64: 1×1 | headline 2×1 | padded 2×1 | 2×2 | padded 4×2 | 4×2, time-varying: dp_wg4_kernel
    0: [(16, 16, 24), (32, 16, 24), (17, 5, 24), (24, 18, 24), (48, 16, 24), (64, 32, 16)],
    1: [(32, 16, 24), (64, 32, 16)],
}
DRIFT_CASES = [("drift", f, n, m, N, dt, "plain") for dt in (0, 1) for (n, m, N) in GRIDS[dt] for f in DRIFT_FORMS]
JUMP_CASES = [("jump", "jump", n, m, N, dt, "plain") for dt in (0, 1) for (n, m, N) in GRIDS[dt]]
ENTRY_CASES = [("drift", "rank1", 32, 16, 24, 0, "linear"), ("drift", "B", 64, 32, 16, 0, "linear"),
               ("drift", "B", 32, 16, 24, 0, "affine")]
# cond: (8, 16) 1×1 tiles and (20, 32) 2×2 tiles of dp_riccati_kernel (time-invariant: the
# iteration with Q + AᵀPA in its shadow); (70, 80) is past the register tiles — dp_big_kernel, a
# potrf + potrs solve with no iteration, the triangular-solve contrast on the same family
COND_CASES = [("cond", "cond", n, m, 24, dt, "plain") for dt in (0, 1) for (n, m) in ((8, 16), (20, 32))]
COND_BIG_CASE = ("cond", "cond", 70, 80, 12, 0, "plain")
# the NS-on against NS-off comparison runs these (the child process imports this module too)
NS_OFF_CASES = [("drift", f, n, m, N, 0, "plain") for (n, m, N) in ((32, 16, 24), (64, 32, 16)) for f in DRIFT_FORMS]

_SEED0 = {"drift": 4100, "jump": 5100, "cond": 6100}
# fp32 drift and jump: the same recursion run in float32 by oracle.dp_reference is itself 6e-6 …
# 1.1e-5 off the longdouble answer on these shapes (12 seeds scanned); the GPU tests require the
# problems to leave a decade below the 1e-4 tolerance, so the seeds are ones at the low end
_SEED_F32 = {(32, 16): 5302, (64, 32): 5304}
_problems = {}


def case_id(case):
    family, form, n, m, N, dtype, entry = case
    return f"{family}-{form}-{n}x{m}-N{N}-{'f32' if dtype else 'f64'}-{entry}"


def problem(lqrx, case):
    """The case's problem (float64 logical arrays, not yet rounded to the working precision);
    built once per process and never modified."""
    if case not in _problems:
        family, form, n, m, N, dtype, entry = case
        seed = _SEED0[family] + 7 * n + m + 1000 * dtype
        if dtype == 1 and family != "cond":
            seed = _SEED_F32[(n, m)]
        if family == "drift":
            p = drift(lqrx, n, m, N, seed, form, dtype)
        elif family == "jump":
            p = jump(lqrx, n, m, N, seed)
        else:
            p = cond(lqrx, n, m, N, seed, dtype)
        if entry != "plain":
            p = with_linear(p, seed, affine=entry == "affine")
        _problems[case] = p
    return _problems[case]
