"""Host-side mirror of the reference's DP (Riccati) surface, backed by the HIP kernels.

Reference surface (Julia, /root/reference/src):
  LQRProblem{n,m,T}(Qf, Q, R, A, B, x0, u0, tf, N)        lqr_problem.jl:1-11
  size(prob) = (n, m, N); num_vars(prob) = N n + (N-1) m   lqr_problem.jl:21-25
  DPSolver(prob)                                           dynamic_programming.jl:13-23
  LQRSolution (exported, undefined upstream: fields K, X, U as used by :62-69)
  solve!(sol, solver, prob)                                dynamic_programming.jl:54-72
  compute_gain!(K, solver, prob), compute_ctg!(K, solver, prob)      :34-52 (per knot)
Extension (no upstream counterpart): linear cost terms q, r, qf on
LQRProblem / LQRBatch → feedforward d and linear cost-to-go p (lqrx_dp_solve_linear); an
affine dynamics offset c, x⁺ = A x + B u + c (lqrx_dp_solve_affine), which also returns d, p; a
cost cross term uᵀM x (lqrx_dp_solve_cross), G = BᵀPA + M, on top of both; the value function's
constant s_k, the expected reduction dV = Σ h_kᵀd_k and the optimal cost J = V_1(x0)
(lqrx_dp_solve_value, value=True) on top of all three.

Array conventions here: a single problem uses plain (rows, cols) numpy matrices; batches
use numpy arrays shaped (batch, rows, cols).  The C ABI wants Julia column-major with the
batch slowest; ``to_abi``/``from_abi`` convert (a transpose of the last two axes).
Every compute call goes through liblqrx.so — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib

__all__ = ["LQRProblem", "LQRSolution", "DPSolver", "solve", "solve_batch", "LQRBatch",
           "random_batch", "to_abi", "from_abi", "dp_solve_device", "compute_gain", "compute_ctg",
           "compute_ctg_batch", "rollout_batch", "dp_rollout_device", "factor_batch", "resolve_batch",
           "dp_factor_device", "dp_resolve_device", "box_batch", "dp_box_device"]


def to_abi(a: np.ndarray) -> np.ndarray:
    """(batch, r, c) row-major logical matrices → contiguous column-major-per-matrix."""
    a = np.asarray(a)
    if a.ndim == 2:  # vectors (batch, r)
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))


def to_soa(flat: np.ndarray, batch: int) -> np.ndarray:
    """Layout-0 flat buffer (batch slowest) → ABI layout 1 (batch fastest): [S][batch]."""
    return np.ascontiguousarray(np.asarray(flat).reshape(batch, -1).T)


def from_soa(soa: np.ndarray, batch: int) -> np.ndarray:
    """ABI layout 1 ([S][batch]) → the layout-0 flat buffer."""
    return np.ascontiguousarray(np.asarray(soa).reshape(-1, batch).T).ravel()


def from_abi(a: np.ndarray, shape: tuple) -> np.ndarray:
    """Inverse of to_abi: flat ABI buffer → (…, r, c) logical matrices."""
    *lead, r, c = shape
    return np.swapaxes(np.asarray(a).reshape(*lead, c, r), -1, -2)


@dataclass
class LQRProblem:
    """Finite-horizon LQR problem (lqr_problem.jl:1-11).  Time-invariant as upstream;
    A/B (and Q/R) may instead carry a leading knot axis of length N-1 (per-knot A_k, B_k,
    the LCRProblem layout of constrained_problem.jl:3-4)."""

    Qf: np.ndarray
    Q: np.ndarray
    R: np.ndarray
    A: np.ndarray
    B: np.ndarray
    x0: np.ndarray
    u0: np.ndarray | None = None
    tf: float = 1.0
    N: int = 2
    # linear cost terms (extension): stage ½xᵀQx + qᵀx + ½uᵀRu + rᵀu, terminal + qfᵀx;
    # q, r time-invariant or with a leading knot axis N-1 (then Q, R must carry one too)
    q: np.ndarray | None = None
    r: np.ndarray | None = None
    qf: np.ndarray | None = None
    # affine dynamics offset (extension): x_{k+1} = A x_k + B u_k + c; c (n,) or, together with a
    # knot axis on A and B, (N-1, n)
    c: np.ndarray | None = None
    # cost cross term (extension): stage cost + uᵀM x; M (m, n) or, together with a knot axis on
    # Q and R, (N-1, m, n)
    M: np.ndarray | None = None

    def size(self):
        n, m = self.B.shape[-2:]
        return n, m, self.N

    def num_vars(self):
        n, m, N = self.size()
        return N * n + (N - 1) * m


@dataclass
class LQRSolution:
    """Output container the reference exports but never defines.

    K[k] (m×n) for k = 1..N-1 stored at index k-1; X[k] (n), U[k] (m); P = P_1 (what
    solver.P holds after solve!) or all P_k when constructed with all_P=True.
    """

    K: np.ndarray
    X: np.ndarray
    U: np.ndarray
    P: np.ndarray
    info: int = 0
    d: np.ndarray | None = None   # feedforward (linear terms): u_k = −K_k x_k − d_k
    p: np.ndarray | None = None   # linear cost-to-go p_1 (or every p_k with all_P)
    # value-function constant (of(…, value=True)): s = s_1 (or every s_k with all_P, s_N = 0),
    # dV = Σ h_kᵀd_k (the expected reduction of a line search), J = V_1(x0) (the optimal cost)
    s: np.ndarray | None = None
    dV: np.ndarray | None = None
    J: np.ndarray | None = None
    # costates λ_k = P_k x_k + p_k, (N, n) (of(…, costates=True)): the multipliers of the dynamics
    lam: np.ndarray | None = None

    @classmethod
    def of(cls, prob: LQRProblem, all_P: bool = False, value: bool = False, costates: bool = False):
        n, m, N = prob.size()
        lin = prob.q is not None or prob.c is not None or prob.M is not None or value
        val = dict(s=np.zeros(N) if all_P else np.zeros(()), dV=np.zeros(()), J=np.zeros(())) if value else {}
        return cls(np.zeros((N - 1, m, n)), np.zeros((N, n)), np.zeros((N - 1, m)),
                   np.zeros((N, n, n)) if all_P else np.zeros((n, n)),
                   d=np.zeros((N - 1, m)) if lin else None,
                   p=(np.zeros((N, n)) if all_P else np.zeros(n)) if lin else None,
                   lam=np.zeros((N, n)) if costates else None, **val)


@dataclass
class DPSolver:
    """DPSolver(prob) (dynamic_programming.jl:13-23).  The Julia struct owns scratch
    (P, P_, PA, PB, APB, E); here the products live in registers/LDS inside the kernel, so
    the solver records the problem shape and dtype plus the two matrices the reference's
    per-knot surface reads and writes: P (the cost-to-go compute_gain!/compute_ctg! start
    from, zero as upstream) and P_ (what compute_ctg! produces)."""

    n: int
    m: int
    N: int
    dtype: int = _lib.F64
    P: np.ndarray | None = None
    P_: np.ndarray | None = None

    @classmethod
    def of(cls, prob: LQRProblem, dtype: int = _lib.F64):
        n, m, N = prob.size()
        return cls(n, m, N, dtype, np.zeros((n, n)), np.zeros((n, n)))


@dataclass
class LQRBatch:
    """A batch of LQRProblems with the same (n, m, N), arrays shaped (batch, r, c)."""

    A: np.ndarray
    B: np.ndarray
    Q: np.ndarray
    R: np.ndarray
    Qf: np.ndarray
    x0: np.ndarray
    N: int
    extra: dict = field(default_factory=dict)
    q: np.ndarray | None = None    # (batch, n) or (batch, N-1, n) — linear terms (extension)
    r: np.ndarray | None = None    # (batch, m) or (batch, N-1, m)
    qf: np.ndarray | None = None   # (batch, n)
    c: np.ndarray | None = None    # (batch, n) or (batch, N-1, n) — affine offset x⁺ = Ax + Bu + c
    M: np.ndarray | None = None    # (batch, m, n) or (batch, N-1, m, n) — cost cross term uᵀM x

    @property
    def batch(self):
        return self.A.shape[0]

    def size(self):
        return self.B.shape[-2], self.B.shape[-1], self.N

    def time_varying(self):
        """(tv_AB, tv_QR): 1 where the fields carry a knot axis, A (batch, N-1, n, n) —
        the per-knot LCRProblem layout (constrained_problem.jl:3-4), SURVEY §8(f) rank 1."""
        return int(np.ndim(self.A) == 4), int(np.ndim(self.Q) == 4)

    @classmethod
    def of(cls, probs: list[LQRProblem]):
        """Stack problems; a 1-D Q, Qf or R is a diagonal (the reference's LQRProblem allows
        TQ, TR = Diagonal, lqr_problem.jl:1-4) and is densified."""
        def field_(p, f):
            a = np.asarray(getattr(p, f), dtype=np.float64)
            return np.diag(a) if f in ("Q", "Qf", "R") and a.ndim == 1 else a
        st = lambda f: np.stack([field_(p, f) for p in probs])
        lin = probs[0].q is not None
        aff = probs[0].c is not None
        if aff:
            for p in probs:   # a knot axis on c needs one on A and B, and vice versa
                if (np.ndim(p.c) == 2) != (np.ndim(p.A) == 3):
                    raise ValueError("c carries a knot axis (N-1, n) exactly when A and B carry one")
        cross = probs[0].M is not None
        if cross:
            for p in probs:   # M is a cost term: its knot axis goes with the one on Q and R
                if (np.ndim(p.M) == 3) != (np.ndim(p.Q) == 3):
                    raise ValueError("M carries a knot axis (N-1, m, n) exactly when Q and R carry one")
        return cls(st("A"), st("B"), st("Q"), st("R"), st("Qf"), st("x0"), probs[0].N,
                   q=st("q") if lin else None, r=st("r") if lin else None,
                   qf=st("qf") if lin else None, c=st("c") if aff else None,
                   M=st("M") if cross else None)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _devices(devices):
    """(int32 array, ctypes pointer, count) for a devices= argument."""
    dv = np.ascontiguousarray(np.asarray(list(devices), dtype=np.int32))
    return dv, dv.ctypes.data_as(C.c_void_p), C.c_int32(len(dv))


# the entry kinds past linear have no devices= form: kind → what the ValueError names
_DP_NO_DEVICES = {"value": "value=True", "cross": "a cost cross term M", "affine": "an affine offset c"}


def solve_batch(b: LQRBatch, dtype: int = _lib.F64, all_P: bool = False, layout: int = 0,
                devices=None, value: bool = False, costates: bool = False):
    """Batched solve! through lqrx_dp_solve_host.  Returns dict of logical arrays
    K (batch, N-1, m, n), P (batch, n, n) or (batch, N, n, n), X (batch, N, n),
    U (batch, N-1, m), info (batch,), and the ABI return code.  layout = 1 hands the
    library batch-fastest (SoA) buffers (the conversion here is host-side bookkeeping; the
    result is the same logical arrays).  devices = [d0, d1, …] shards the batch over those
    GPUs in one call (lqrx_dp_solve[_linear]_host_devices; repeats allowed).  With b.c (affine
    dynamics) the call is lqrx_dp_solve_affine_host: missing q, r, qf are zeros, d and p are
    returned; it has no devices= form.  With b.M (cost cross term) the call is
    lqrx_dp_solve_cross_host: a missing c is zeros as well; no devices= form either.  With
    value=True the call is lqrx_dp_solve_value_host: missing c, M, q, r, qf are zeros, and the
    result gains s ((batch,) s_1, or (batch, N) every s_k with all_P), dV and J ((batch,)); no
    devices= form.  With costates=True the result gains lam (batch, N, n), the costates
    λ_k = P_k x_k + p_k of the solution, by one more call (lqrx_dp_costates_host, layout 0) on the
    K, X, U just returned."""
    n, m, N = b.size()
    bt = b.batch
    tvAB, tvQR = b.time_varying()
    npdt = np.float64 if dtype == _lib.F64 else np.float32
    kab, kq, kP = (N - 1 if tvAB else 1), (N - 1 if tvQR else 1), (N if all_P else 1)
    kind = ("value" if value else "cross" if b.M is not None else "affine" if b.c is not None
            else "linear" if b.q is not None else "")
    if kind in _DP_NO_DEVICES:
        if devices is not None:
            raise ValueError("devices= is not available with " + _DP_NO_DEVICES[kind])
        # missing c, M, q, r, qf are zeros, with a knot axis where their neighbours carry one
        ab, qr = ((N - 1,) if tvAB else ()), ((N - 1,) if tvQR else ())
        fill = dict(c=(bt, *ab, n), q=(bt, *qr, n), r=(bt, *qr, m), qf=(bt, n))
        if kind != "affine":
            fill["M"] = (bt, *qr, m, n)
        b = replace(b, **{k: np.zeros(sh, npdt) for k, sh in fill.items() if getattr(b, k) is None})
        if b.M is not None:
            if np.shape(b.M)[-2:] != (m, n):
                raise ValueError("M is (m, n) per trajectory (per knot), the shape of K")
            if (np.ndim(b.M) == 4) != bool(tvQR):
                raise ValueError("M carries a knot axis (batch, N-1, m, n) exactly when Q and R carry one")
        if (np.ndim(b.c) == 3) != bool(tvAB):
            raise ValueError("c carries a knot axis (batch, N-1, n) exactly when A and B carry one")
    elif kind == "linear" and (b.r is None or b.qf is None):
        raise ValueError("linear cost terms need q, r and qf together")
    # the entry's inputs by name, flat and in layout 0: matrices column-major, vectors as they are
    mats = ("A", "B", "Q", "R", "Qf") + (("M",) if b.M is not None else ())
    vecs = dict(x0=bt * n, **(dict(q=bt * kq * n, r=bt * kq * m, qf=bt * n) if kind else {}),
                **(dict(c=bt * kab * n) if b.c is not None else {}))
    in0 = {k: to_abi(np.asarray(getattr(b, k), dtype=npdt)).reshape(-1) for k in mats}
    in0.update({k: np.ascontiguousarray(np.asarray(getattr(b, k), dtype=npdt).reshape(sz)) for k, sz in vecs.items()})
    outs = dict(K=bt * (N - 1) * m * n, P=bt * n * n * kP, X=bt * N * n, U=bt * (N - 1) * m)
    if kind:
        outs.update(d=bt * (N - 1) * m, p=bt * n * kP)
    if value:
        outs.update(s=bt * kP, dV=bt, J=bt)
    buf = {k: to_soa(a, bt) for k, a in in0.items()} if layout == 1 else dict(in0)
    buf.update({k: np.zeros(sz, npdt) for k, sz in outs.items()})
    buf["info"] = np.zeros(bt, np.int32)
    args = {k: _ptr(a) for k, a in buf.items()}
    if kind:
        ln = _lib.DpLinear(*[args[k].value for k in ("q", "r", "qf", "d", "p")])
        args["lin"] = C.byref(ln)
    if value:
        vl = _lib.DpValue(*[args[k].value for k in ("s", "dV", "J")])
        args["val"] = C.byref(vl)
    if devices is not None:
        dv, args["devices"], args["ndev"] = _devices(devices)
    entry = "lqrx_dp_solve" + ("_" + kind if kind else "") + ("_host" if devices is None else "_host_devices")
    d = _lib.DpDesc(n, m, N, dtype, bt, layout, 1 if all_P else 0, tvAB, tvQR)
    rc = _lib.check(_lib.dp_call(entry, d, args))
    o = {k: from_soa(buf[k], bt) if layout == 1 else buf[k] for k in outs}
    out = dict(K=from_abi(o["K"], (bt, N - 1, m, n)),
               P=from_abi(o["P"], (bt, N, n, n) if all_P else (bt, n, n)),
               X=o["X"].reshape(bt, N, n), U=o["U"].reshape(bt, N - 1, m), info=buf["info"], rc=rc)
    if kind:
        out["d"] = o["d"].reshape(bt, N - 1, m)
        out["p"] = o["p"].reshape(bt, N, n) if all_P else o["p"].reshape(bt, n)
    if value:
        out["s"] = o["s"].reshape(bt, N) if all_P else o["s"]
        out["dV"], out["J"] = o["dV"], o["J"]
    if costates:   # λ_k from the K, X, U just returned; absent M, q, r, qf are NULL (zero)
        cin = dict(in0, K=to_abi(out["K"]).reshape(-1), X=o["X"], U=o["U"])
        lam = np.zeros(bt * N * n, npdt)
        d0 = _lib.DpDesc(n, m, N, dtype, bt, 0, 0, tvAB, tvQR)
        _lib.check(_lib.load().lqrx_dp_costates_host(
            C.byref(d0), *[_ptr(cin[k]) if k in cin else None
                           for k in ("A", "B", "Q", "R", "M", "Qf", "q", "r", "qf", "K", "X", "U")], _ptr(lam)))
        out["lam"] = lam.reshape(bt, N, n)
    return out


def solve(sol: LQRSolution, solver: DPSolver, prob: LQRProblem) -> LQRSolution:
    """solve!(sol, solver, prob) — dynamic_programming.jl:54-72 (one problem)."""
    all_P = sol.P.ndim == 3
    value = sol.s is not None
    out = solve_batch(LQRBatch.of([prob]), solver.dtype, all_P, value=value, costates=sol.lam is not None)
    sol.K[...] = out["K"][0]
    sol.X[...] = out["X"][0]
    sol.U[...] = out["U"][0]
    sol.P[...] = out["P"][0]
    sol.info = int(out["info"][0])
    if prob.q is not None or prob.c is not None or prob.M is not None or value:
        sol.d = out["d"][0]
        sol.p = out["p"][0]
    if value:
        sol.s, sol.dV, sol.J = out["s"][0], out["dV"][0], out["J"][0]
    if sol.lam is not None:
        sol.lam = out["lam"][0]
    return sol


def compute_ctg_batch(A, B, Q, R, P, dtype: int = _lib.F64, gain_only: bool = False):
    """compute_ctg! (dynamic_programming.jl:45-52; compute_gain! :34-43 with gain_only) for a
    batch through lqrx_dp_compute_ctg_host: A (batch, n, n), B (batch, n, m), Q, R, and
    P = solver.P (batch, n, n).  Returns K (batch, m, n), P_ (batch, n, n) (None with
    gain_only), info (batch,), rc."""
    lib = _lib.load()
    A = np.asarray(A)
    bt, n, m = A.shape[0], A.shape[-1], np.asarray(B).shape[-1]
    # the kernels' symmetric fast form needs symmetric P and Q (include/lqrx.h precondition);
    # the tolerance is relative to the largest entry and never tighter than 100 ulp of the
    # working dtype (an fp32 AᵀPA is symmetric only to fp32 rounding); Q never enters K, so a
    # gain-only call does not check it
    rtol = max(1e-10, 100.0 * float(np.finfo(np.float64 if dtype == _lib.F64 else np.float32).eps))
    for name, M in (("P", P),) + (() if gain_only else (("Q", Q),)):
        M = np.asarray(M, dtype=np.float64)
        if np.abs(M - np.swapaxes(M, -1, -2)).max(initial=0.0) > rtol * max(np.abs(M).max(initial=0.0), 1e-300):
            raise ValueError(f"compute_ctg: {name} must be symmetric (the Riccati cost-to-go / cost "
                             "Hessian; lqrx_dp_compute_ctg precondition)")
    npdt = np.float64 if dtype == _lib.F64 else np.float32
    ins = [to_abi(np.asarray(x, dtype=npdt)) for x in (A, B, Q, R, P)]
    K = np.zeros(bt * m * n, npdt)
    Pn = None if gain_only else np.zeros(bt * n * n, npdt)
    info = np.zeros(bt, np.int32)
    d = _lib.DpDesc(n, m, 2, dtype, bt, 0, 0, 0, 0)
    rc = _lib.check(lib.lqrx_dp_compute_ctg_host(C.byref(d), *[_ptr(a) for a in ins], _ptr(K),
                                                 None if Pn is None else _ptr(Pn), _ptr(info)))
    return dict(K=from_abi(K, (bt, m, n)), P_=None if Pn is None else from_abi(Pn, (bt, n, n)),
                info=info, rc=rc)


def compute_gain(K: np.ndarray, solver: DPSolver, prob: LQRProblem) -> np.ndarray:
    """compute_gain!(K, solver, prob) — dynamic_programming.jl:34-43: K = E⁻¹BᵀPA from
    P = solver.P (test/dp.jl:16 calls it on a fresh solver, P = 0)."""
    b = LQRBatch.of([prob])                       # densifies Diagonal Q / R
    out = compute_ctg_batch(b.A, b.B, b.Q, b.R, np.asarray(solver.P)[None], solver.dtype, gain_only=True)
    K[...] = out["K"][0]
    return K


def compute_ctg(K: np.ndarray, solver: DPSolver, prob: LQRProblem) -> np.ndarray:
    """compute_ctg!(K, solver, prob) — dynamic_programming.jl:45-52: the gain as above and
    solver.P_ = Q + AᵀPA − APB·K."""
    b = LQRBatch.of([prob])
    out = compute_ctg_batch(b.A, b.B, b.Q, b.R, np.asarray(solver.P)[None], solver.dtype)
    K[...] = out["K"][0]
    solver.P_[...] = out["P_"][0]
    return K


def random_batch(n: int, m: int, N: int, batch: int, seed: int, traj0: int = 0,
                 dtype: int = _lib.F64) -> dict:
    """Synthetic random-dense batch from the library's counter-based generator, returned
    in ABI layout (flat arrays) — the same bytes the bench feeds the kernel."""
    lib = _lib.load()
    npdt = np.float64 if dtype == _lib.F64 else np.float32
    A = np.empty(batch * n * n, npdt); B = np.empty(batch * n * m, npdt)
    Q = np.empty(batch * n * n, npdt); R = np.empty(batch * m * m, npdt)
    Qf = np.empty(batch * n * n, npdt); x0 = np.empty(batch * n, npdt)
    _lib.check(lib.lqrx_make_random_dp(n, m, batch, traj0, seed, dtype, _ptr(A), _ptr(B),
                                       _ptr(Q), _ptr(R), _ptr(Qf), _ptr(x0)))
    return dict(A=A, B=B, Q=Q, R=R, Qf=Qf, x0=x0, n=n, m=m, N=N, batch=batch)


def abi_to_batch(d: dict) -> LQRBatch:
    n, m, N, bt = d["n"], d["m"], d["N"], d["batch"]
    return LQRBatch(from_abi(d["A"], (bt, n, n)), from_abi(d["B"], (bt, n, m)),
                    from_abi(d["Q"], (bt, n, n)), from_abi(d["R"], (bt, m, m)),
                    from_abi(d["Qf"], (bt, n, n)), d["x0"].reshape(bt, n), N)


def dp_solve_device(t: dict, N: int, p_mode: int = 0, stream: int | None = None,
                    out: dict | None = None, layout: int = 0, value: bool = False,
                    costates: bool = False) -> dict:
    """Device-pointer entry point on torch tensors already in ABI layout (flat; layout 1 =
    batch fastest, every input and output).

    t: dict with torch tensors A, B, Q, R, Qf, x0 on the GPU and ints n, m, batch; with
    tensors q, r, qf as well it runs lqrx_dp_solve_linear and also returns d and p; with a
    tensor c too (n·batch, or n·(N−1)·batch with tv_AB) it runs lqrx_dp_solve_affine; with a
    tensor M on top of those (m·n·batch, or m·n·(N−1)·batch with tv_QR) lqrx_dp_solve_cross.
    value=True (needs M, c, q, r, qf) runs lqrx_dp_solve_value and also returns s (batch, or
    N·batch with p_mode 1), dV and J (batch); an `out` that holds s but None (or nothing) for dV
    or J passes NULL for it, and the library skips it.
    costates=True (layout 0) also returns lam (n·N·batch, laid out like X), the costates
    λ_k = P_k x_k + p_k, by lqrx_dp_costates on the same stream; absent M, q, r, qf are NULL (zero).
    Returns dict of output tensors (K, P, X, U, info[, d, p[, s, dV, J]]).  `stream` is a raw hipStream_t
    (torch.cuda.current_stream().cuda_stream); None = the null stream, synchronous.
    """
    import torch

    lib = _lib.load()
    n, m, bt = t["n"], t["m"], t["batch"]
    tdt = t["A"].dtype
    dtype = _lib.F64 if tdt == torch.float64 else _lib.F32
    dev = t["A"].device
    has = lambda k: t.get(k) is not None
    if has("c") and not has("q"):
        raise ValueError("dp_solve_device: c needs q, r, qf (zeros for a problem without cost terms)")
    if has("M") and not has("c"):
        raise ValueError("dp_solve_device: M needs c and q, r, qf (zeros where the problem has none)")
    if value and not has("M"):
        raise ValueError("dp_solve_device: value=True needs M, c and q, r, qf (zeros where the problem has none)")
    kind = "value" if value else "cross" if has("M") else "affine" if has("c") else "linear" if has("q") else ""
    entry = "lqrx_dp_solve" + ("_" + kind if kind else "")
    kP = N if p_mode else 1
    # outputs the caller's `out` does not hold yet, group by group (elements; info is int32)
    groups = [dict(K=bt * (N - 1) * m * n, P=bt * n * n * kP, X=bt * N * n, U=bt * (N - 1) * m, info=bt)]
    if kind:
        groups.append(dict(d=bt * (N - 1) * m, p=bt * n * kP))
    if value:
        groups.append(dict(s=bt * kP, dV=bt, J=bt))
    out = {} if out is None else out
    for g in groups:
        if next(iter(g)) not in out:
            out.update({k: torch.empty(sz, dtype=torch.int32 if k == "info" else tdt, device=dev) for k, sz in g.items()})
    d = _lib.DpDesc(n, m, N, dtype, bt, layout, p_mode, int(t.get("tv_AB", 0)), int(t.get("tv_QR", 0)))
    p = lambda x: C.c_void_p(x.data_ptr())
    st = C.c_void_p(stream) if stream else None
    tensor = lambda k: out[k] if k in out else t[k]      # input and output names are disjoint
    args = {k: p(tensor(k)) for k in _lib.DP_ENTRY_ARGS[entry] if k not in ("lin", "val", "stream")}
    args["stream"] = st
    if kind:
        ln = _lib.DpLinear(*[tensor(k).data_ptr() for k in ("q", "r", "qf", "d", "p")])
        args["lin"] = C.byref(ln)
    if value:   # dV, J: optional, NULL where `out` holds None (or nothing) for them
        vl = _lib.DpValue(*[out[k].data_ptr() if out.get(k) is not None else None for k in ("s", "dV", "J")])
        args["val"] = C.byref(vl)
    rc = _lib.check(_lib.dp_call(entry, d, args))
    if costates:
        if out.get("lam") is None:
            out["lam"] = torch.empty(bt * N * n, dtype=tdt, device=dev)
        opt = lambda k: p(t[k]) if has(k) else None
        _lib.check(lib.lqrx_dp_costates(C.byref(d), p(t["A"]), p(t["B"]), p(t["Q"]), p(t["R"]), opt("M"),
                                        p(t["Qf"]), opt("q"), opt("r"), opt("qf"), p(out["K"]), p(out["X"]),
                                        p(out["U"]), p(out["lam"]), st))
    out["rc"] = rc
    return out


_ROLLOUT_OUT = ("X", "U", "J")


def rollout_batch(b: LQRBatch, K, d, x0, alpha=None, w=None, u_lo=None, u_hi=None, dtype: int = _lib.F64,
                  outputs=("X", "U", "J")) -> dict:
    """Closed-loop rollout of the policy (K, d) of a solve over S scenarios per problem, through
    lqrx_dp_rollout_host: x_1 = x0, u_k = clip(−K_k x_k − α d_k, u_lo, u_hi), x_{k+1} = A_k x_k + B_k u_k
    + c_k + w_k, and the cost J of every trajectory.

    b gives A, B (and c; and Q, R, Qf, M, q, r, qf when J is asked for); its own x0 is not used.
    K (batch, N−1, m, n) and d (batch, N−1, m), or None for zero, are the solve's.  x0 (batch, S, n);
    alpha (batch, S) or None (1); w (batch, S, N−1, n) or None (0); u_lo, u_hi (batch, m) or None (no
    bound; ±inf entries allowed).  Returns those of X (batch, S, N, n), U (batch, S, N−1, m),
    J (batch, S) that `outputs` names, and the ABI return code rc."""
    n, m, N = b.size()
    bt = b.batch
    tvAB, tvQR = b.time_varying()
    npdt = np.float64 if dtype == _lib.F64 else np.float32
    outputs = tuple(outputs)
    if not outputs or any(k not in _ROLLOUT_OUT for k in outputs):
        raise ValueError(f"rollout_batch: outputs must name at least one of {_ROLLOUT_OUT} (got {outputs})")
    x0 = np.asarray(x0, dtype=npdt)
    if x0.ndim != 3 or x0.shape[0] != bt or x0.shape[2] != n:
        raise ValueError("rollout_batch: x0 is (batch, S, n)")
    S = x0.shape[1]
    flat = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=npdt)).reshape(-1)
    mat = lambda a: None if a is None else to_abi(np.asarray(a, dtype=npdt)).reshape(-1)

    def sized(name, a, size):
        if a is not None and a.size != size:
            raise ValueError(f"rollout_batch: {name} has {a.size} elements, expected {size}")
        return a

    kab, kq = (N - 1 if tvAB else 1), (N - 1 if tvQR else 1)
    ins = dict(A=mat(b.A), B=mat(b.B), c=sized("c", flat(b.c), bt * kab * n),
               K=sized("K", mat(K), bt * (N - 1) * m * n), d=sized("d", flat(d), bt * (N - 1) * m))
    cost = dict.fromkeys(("Q", "R", "Qf", "M", "q", "r", "qf"))
    if "J" in outputs:
        cost.update(Q=mat(b.Q), R=mat(b.R), Qf=mat(b.Qf), M=sized("M", mat(b.M), bt * kq * m * n),
                    q=sized("q", flat(b.q), bt * kq * n), r=sized("r", flat(b.r), bt * kq * m),
                    qf=sized("qf", flat(b.qf), bt * n))
    scn = dict(x0=flat(x0), alpha=sized("alpha", flat(alpha), bt * S), w=sized("w", flat(w), bt * S * (N - 1) * n),
               u_lo=sized("u_lo", flat(u_lo), bt * m), u_hi=sized("u_hi", flat(u_hi), bt * m))
    sizes = dict(X=bt * S * N * n, U=bt * S * (N - 1) * m, J=bt * S)
    out = {k: np.zeros(sizes[k], npdt) for k in outputs}
    p = lambda a: None if a is None else a.ctypes.data
    ct = _lib.DpCost(*[p(cost[k]) for k in ("Q", "R", "Qf", "M", "q", "r", "qf")])
    sc = _lib.DpScenarios(S, *[p(scn[k]) for k in ("x0", "alpha", "w", "u_lo", "u_hi")],
                          *[p(out.get(k)) for k in _ROLLOUT_OUT])
    desc = _lib.DpDesc(n, m, N, dtype, bt, 0, 0, tvAB, tvQR)
    rc = _lib.check(_lib.load().lqrx_dp_rollout_host(
        C.byref(desc), *[p(ins[k]) for k in ("A", "B", "c", "K", "d")],
        C.byref(ct) if "J" in outputs else None, C.byref(sc)))
    shapes = dict(X=(bt, S, N, n), U=(bt, S, N - 1, m), J=(bt, S))
    res = {k: out[k].reshape(shapes[k]) for k in outputs}
    res["rc"] = rc
    return res


def dp_rollout_device(t: dict, N: int, K, d, sc: dict, stream: int | None = None, out: dict | None = None) -> dict:
    """Device-pointer entry point of the scenario rollout (lqrx_dp_rollout) on torch tensors already
    in ABI layout (flat, layout 0), in the manner of dp_solve_device.

    t: the problem — tensors A, B, optionally c, and for J the cost Q, R, Qf and optionally M, q, r, qf;
    ints n, m, batch and optional tv_AB / tv_QR.  K, d: the solve's gains and feedforward (d may be
    None: zero).  sc: S, tensor x0 (n·S·batch) and optionally alpha (S·batch), w (n·(N−1)·S·batch),
    u_lo, u_hi (m·batch); "outputs" names which of X, U, J to form (default all three).  `out` may
    hold preallocated X, U, J.  Returns the dict of output tensors (trajectory t = b·S + j: X
    n·N per trajectory, U m·(N−1), J one element) and rc.  `stream` is a raw hipStream_t; None = the
    null stream, synchronous.  The call allocates nothing inside the library."""
    import torch

    lib = _lib.load()
    n, m, bt = t["n"], t["m"], t["batch"]
    tdt = t["A"].dtype
    dtype = _lib.F64 if tdt == torch.float64 else _lib.F32
    dev = t["A"].device
    S = int(sc["S"])
    outputs = tuple(sc.get("outputs", _ROLLOUT_OUT))
    if not outputs or any(k not in _ROLLOUT_OUT for k in outputs):
        raise ValueError(f"dp_rollout_device: outputs must name at least one of {_ROLLOUT_OUT} (got {outputs})")
    sizes = dict(X=bt * S * N * n, U=bt * S * (N - 1) * m, J=bt * S)
    out = {} if out is None else out
    for k in outputs:
        if out.get(k) is None:
            out[k] = torch.empty(sizes[k], dtype=tdt, device=dev)
    p = lambda x: None if x is None else x.data_ptr()
    ct = _lib.DpCost(*[p(t.get(k)) for k in ("Q", "R", "Qf", "M", "q", "r", "qf")])
    scn = _lib.DpScenarios(S, *[p(sc.get(k)) for k in ("x0", "alpha", "w", "u_lo", "u_hi")],
                           *[p(out[k]) if k in outputs else None for k in _ROLLOUT_OUT])
    desc = _lib.DpDesc(n, m, N, dtype, bt, 0, 0, int(t.get("tv_AB", 0)), int(t.get("tv_QR", 0)))
    vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    rc = _lib.check(lib.lqrx_dp_rollout(C.byref(desc), vp(t["A"]), vp(t["B"]), vp(t.get("c")), vp(K), vp(d),
                                        C.byref(ct) if "J" in outputs else None, C.byref(scn),
                                        C.c_void_p(stream) if stream else None))
    res = {k: out[k] for k in outputs}
    res["rc"] = rc
    return res


_RESOLVE_OUT = ("d", "p", "X", "U")


def _resolve_outputs(who: str, outputs) -> tuple:
    outputs = tuple(outputs)
    if not outputs or any(k not in _RESOLVE_OUT for k in outputs):
        raise ValueError(f"{who}: outputs must name at least one of {_RESOLVE_OUT} (got {outputs})")
    if "d" not in outputs and ("X" in outputs or "U" in outputs):
        raise ValueError(f"{who}: X and U need d among the outputs (d carries the backward pass to the forward one)")
    return outputs


def factor_batch(b: LQRBatch, P, dtype: int = _lib.F64) -> dict:
    """E_k⁻¹ and P_{k+1}c_k of a solved batch, through lqrx_dp_factor_host: what resolve_batch needs
    beside the solve's K.  b gives B, R (and c); P (batch, N, n, n) is every P_k of the solve
    (solve_batch(..., all_P=True)).  Returns Einv (batch, N−1, m, m), Pc (batch, N−1, n) or None
    without b.c, info (batch: 0, or the largest knot whose E is not positive definite) and rc."""
    n, m, N = b.size()
    bt = b.batch
    tvAB, tvQR = b.time_varying()
    npdt = np.float64 if dtype == _lib.F64 else np.float32
    P = np.asarray(P, dtype=npdt)
    if P.shape != (bt, N, n, n):
        raise ValueError(f"factor_batch: P is (batch, N, n, n) = {(bt, N, n, n)}, every P_k of the solve (got {P.shape})")
    kab = N - 1 if tvAB else 1
    c = None if b.c is None else np.ascontiguousarray(np.asarray(b.c, dtype=npdt)).reshape(-1)
    if c is not None and c.size != bt * kab * n:
        raise ValueError(f"factor_batch: c has {c.size} elements, expected {bt * kab * n}")
    mat = lambda a: to_abi(np.asarray(a, dtype=npdt)).reshape(-1)
    Bf, Rf, Pf = mat(b.B), mat(b.R), mat(P)
    Einv = np.zeros(bt * (N - 1) * m * m, npdt)
    Pc = None if c is None else np.zeros(bt * (N - 1) * n, npdt)
    info = np.zeros(bt, np.int32)
    p = lambda a: None if a is None else a.ctypes.data
    desc = _lib.DpDesc(n, m, N, dtype, bt, 0, 1, tvAB, tvQR)
    rc = _lib.check(_lib.load().lqrx_dp_factor_host(C.byref(desc), p(Bf), p(Rf), p(c), p(Pf), p(Einv), p(Pc), p(info)))
    return dict(Einv=from_abi(Einv, (bt, N - 1, m, m)), Pc=None if Pc is None else Pc.reshape(bt, N - 1, n),
                info=info, rc=rc)


def resolve_batch(b: LQRBatch, K, fac: dict, x0=None, q=None, r=None, qf=None, all_p: bool = False,
                  dtype: int = _lib.F64, outputs=_RESOLVE_OUT) -> dict:
    """S new right-hand sides per problem on the factors of one solve, through lqrx_dp_resolve_host.

    b gives A, B (and c); K (batch, N−1, m, n) is the solve's gain, fac = dict(Einv=, Pc=) what
    factor_batch returned (Pc None exactly when b.c is).  x0, qf (batch, S, n); q (batch, S, n) or
    (batch, S, N−1, n); r (batch, S, m) or (batch, S, N−1, m), with a knot axis on both or neither; each
    may be None (zero), at least one sets S.  Returns those of d (batch, S, N−1, m), p (batch, S, n),
    or (batch, S, N, n) with all_p), X (batch, S, N, n), U (batch, S, N−1, m) that `outputs` names, and rc."""
    n, m, N = b.size()
    bt = b.batch
    tvAB, _ = b.time_varying()
    npdt = np.float64 if dtype == _lib.F64 else np.float32
    outputs = _resolve_outputs("resolve_batch", outputs)
    given = {k: np.asarray(v, dtype=npdt) for k, v in dict(x0=x0, q=q, r=r, qf=qf).items() if v is not None}
    if not given:
        raise ValueError("resolve_batch: at least one of x0, q, r, qf must be given (it sets S)")
    first = next(iter(given.values()))
    S = first.shape[1] if first.ndim >= 2 else 0
    if S < 1:
        raise ValueError("resolve_batch: right-hand sides are (batch, S, ...) with S >= 1")
    for k in ("x0", "qf"):
        if k in given and given[k].shape != (bt, S, n):
            raise ValueError(f"resolve_batch: {k} is (batch, S, n) = {(bt, S, n)} (got {given[k].shape})")
    knot = {k: given[k].ndim == 4 for k in ("q", "r") if k in given}
    if len(set(knot.values())) > 1:
        raise ValueError("resolve_batch: q and r carry a knot axis (batch, S, N-1, ·) both or neither")
    tvQR = int(any(knot.values()))
    for k, w in (("q", n), ("r", m)):
        want = (bt, S, N - 1, w) if tvQR else (bt, S, w)
        if k in given and given[k].shape != want:
            raise ValueError(f"resolve_batch: {k} is {want} (got {given[k].shape})")
    flat = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=npdt)).reshape(-1)
    mat = lambda a: None if a is None else to_abi(np.asarray(a, dtype=npdt)).reshape(-1)

    def sized(name, a, size):
        if a is not None and a.size != size:
            raise ValueError(f"resolve_batch: {name} has {a.size} elements, expected {size}")
        return a

    kab = N - 1 if tvAB else 1
    if fac.get("Einv") is None:
        raise ValueError("resolve_batch: fac needs Einv (factor_batch's)")
    if (fac.get("Pc") is None) != (b.c is None):
        raise ValueError("resolve_batch: fac['Pc'] is given exactly when the batch has c")
    ins = dict(A=mat(b.A), B=mat(b.B), c=sized("c", flat(b.c), bt * kab * n),
               K=sized("K", mat(K), bt * (N - 1) * m * n), Einv=sized("Einv", mat(fac["Einv"]), bt * (N - 1) * m * m),
               Pc=sized("Pc", flat(fac.get("Pc")), bt * (N - 1) * n))
    rh = {k: flat(given.get(k)) for k in ("q", "r", "qf", "x0")}
    kp = N if all_p else 1
    sizes = dict(d=bt * S * (N - 1) * m, p=bt * S * kp * n, X=bt * S * N * n, U=bt * S * (N - 1) * m)
    out = {k: np.zeros(sizes[k], npdt) for k in outputs}
    p = lambda a: None if a is None else a.ctypes.data
    fc = _lib.DpFactors(p(ins["K"]), p(ins["Einv"]), p(ins["Pc"]))
    rs = _lib.DpRhs(S, *[p(rh[k]) for k in ("q", "r", "qf", "x0")], *[p(out.get(k)) for k in _RESOLVE_OUT])
    desc = _lib.DpDesc(n, m, N, dtype, bt, 0, int(all_p), tvAB, tvQR)
    rc = _lib.check(_lib.load().lqrx_dp_resolve_host(C.byref(desc), p(ins["A"]), p(ins["B"]), p(ins["c"]),
                                                     C.byref(fc), C.byref(rs)))
    shapes = dict(d=(bt, S, N - 1, m), p=(bt, S, N, n) if all_p else (bt, S, n), X=(bt, S, N, n), U=(bt, S, N - 1, m))
    res = {k: out[k].reshape(shapes[k]) for k in outputs}
    res["rc"] = rc
    return res


def dp_factor_device(t: dict, N: int, P, out: dict | None = None, stream: int | None = None) -> dict:
    """Device-pointer entry point of lqrx_dp_factor on torch tensors already in ABI layout (flat,
    layout 0), in the manner of dp_rollout_device.

    t: tensors B, R and optionally c, ints n, m, batch and optional tv_AB / tv_QR.  P: every P_k of a
    solve (dp_solve_device(..., p_mode=1)["P"], n·n·N·batch).  `out` may hold preallocated Einv
    (m·m·(N−1)·batch), Pc (n·(N−1)·batch) and info (int32, batch).  Returns dict(Einv, Pc (None without
    t["c"]), info, rc).  `stream` is a raw hipStream_t; None = the null stream, synchronous.  The call
    allocates nothing inside the library."""
    import torch

    n, m, bt = t["n"], t["m"], t["batch"]
    tdt = t["B"].dtype
    dtype = _lib.F64 if tdt == torch.float64 else _lib.F32
    dev = t["B"].device
    c = t.get("c")
    out = {} if out is None else out
    if out.get("Einv") is None:
        out["Einv"] = torch.empty(bt * (N - 1) * m * m, dtype=tdt, device=dev)
    if c is None:
        out["Pc"] = None
    elif out.get("Pc") is None:
        out["Pc"] = torch.empty(bt * (N - 1) * n, dtype=tdt, device=dev)
    if out.get("info") is None:
        out["info"] = torch.empty(bt, dtype=torch.int32, device=dev)
    desc = _lib.DpDesc(n, m, N, dtype, bt, 0, 1, int(t.get("tv_AB", 0)), int(t.get("tv_QR", 0)))
    vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    rc = _lib.check(_lib.load().lqrx_dp_factor(C.byref(desc), vp(t["B"]), vp(t["R"]), vp(c), vp(P), vp(out["Einv"]),
                                               vp(out["Pc"]), vp(out["info"]), C.c_void_p(stream) if stream else None))
    return dict(Einv=out["Einv"], Pc=out["Pc"], info=out["info"], rc=rc)


def dp_resolve_device(t: dict, N: int, fac: dict, rhs: dict, stream: int | None = None, out: dict | None = None) -> dict:
    """Device-pointer entry point of lqrx_dp_resolve on torch tensors already in ABI layout (flat,
    layout 0), in the manner of dp_rollout_device.

    t: tensors A, B and optionally c, ints n, m, batch and optional tv_AB; t["tv_QR"] is not read.
    fac = dict(K=, Einv=, Pc=): the solve's gains and dp_factor_device's tensors (Pc None exactly when
    t has no c).  rhs = dict(S=, q=, r=, qf=, x0=, outputs=("d", "p", "X", "U")): the right-hand sides,
    trajectory t = b·S + j, each tensor optional (zero); "tv_QR" (default 0) says whether q and r carry
    a knot axis (n·(N−1) resp. m·(N−1) per trajectory), "p_mode" (default 0) whether p holds every p_k
    (n·N per trajectory).  `out` may hold preallocated d, p, X, U.  Returns the dict of output tensors
    and rc.  `stream` is a raw hipStream_t; None = the null stream, synchronous.  The call allocates
    nothing inside the library."""
    import torch

    outputs = _resolve_outputs("dp_resolve_device", rhs.get("outputs", _RESOLVE_OUT))
    n, m, bt = t["n"], t["m"], t["batch"]
    tdt = t["A"].dtype
    dtype = _lib.F64 if tdt == torch.float64 else _lib.F32
    dev = t["A"].device
    S = int(rhs["S"])
    p_mode = int(rhs.get("p_mode", 0))
    sizes = dict(d=bt * S * (N - 1) * m, p=bt * S * (N if p_mode else 1) * n, X=bt * S * N * n, U=bt * S * (N - 1) * m)
    out = {} if out is None else out
    for k in outputs:
        if out.get(k) is None:
            out[k] = torch.empty(sizes[k], dtype=tdt, device=dev)
    p = lambda x: None if x is None else x.data_ptr()
    fc = _lib.DpFactors(p(fac.get("K")), p(fac.get("Einv")), p(fac.get("Pc")))
    rs = _lib.DpRhs(S, *[p(rhs.get(k)) for k in ("q", "r", "qf", "x0")],
                    *[p(out[k]) if k in outputs else None for k in _RESOLVE_OUT])
    desc = _lib.DpDesc(n, m, N, dtype, bt, 0, p_mode, int(t.get("tv_AB", 0)), int(rhs.get("tv_QR", 0)))
    vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    rc = _lib.check(_lib.load().lqrx_dp_resolve(C.byref(desc), vp(t["A"]), vp(t["B"]), vp(t.get("c")), C.byref(fc),
                                                C.byref(rs), C.c_void_p(stream) if stream else None))
    res = {k: out[k] for k in outputs}
    res["rc"] = rc
    return res


_BOX_RHS_OUT = ("d", "X", "U")
_BOX_OUT = ("iters", "res")


def _box_params(who: str, rho, relax, eps, max_iter) -> tuple:
    try:
        eps_prim, eps_dual = (float(e) for e in eps)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: eps is the pair (eps_prim, eps_dual) (got {eps!r})") from None
    return float(rho), float(relax), eps_prim, eps_dual, int(max_iter)


def box_batch(b: LQRBatch, u_lo, u_hi, x0=None, q=None, r=None, qf=None, rho: float = 1.0, relax: float = 1.6,
              eps=(1e-6, 1e-6), max_iter: int = 500, Z=None, W=None, dtype: int = _lib.F64) -> dict:
    """Input bounds u_lo ≤ u_k ≤ u_hi on S instances per problem, the whole way on logical host arrays:
    the cross solve of b with R + ρI (on every stored R knot) and all P_k, factor_batch, then
    lqrx_dp_resolve_box_host (include/lqrx.h has the iteration).

    u_lo, u_hi: (batch, m), (m,), a scalar, or None (no bound on that side); ±inf allowed.  x0, qf
    (batch, S, n); q (batch, S, n) or (batch, S, N−1, n); r (batch, S, m) or (batch, S, N−1, m), a knot axis
    on both or neither; each may be None (zero).  With all four None the batch's own x0, q, r, qf are
    the one instance (S = 1).  Z, W (batch, S, N−1, m) warm-start the iteration (None: zeros, a cold start)
    and are not modified.  eps = (eps_prim, eps_dual).  Returns X (batch, S, N, n), U, Z, W, Y = ρW
    (batch, S, N−1, m), iters (batch, S), res (batch, S, 2: r_prim, r_dual), info (batch: the solve's or
    the factor's, 0 when R + ρI gave positive definite E_k) and rc."""
    n, m, N = b.size()
    bt = b.batch
    tvAB, tvQR_b = b.time_varying()
    npdt = np.float64 if dtype == _lib.F64 else np.float32
    rho, relax, eps_prim, eps_dual, max_iter = _box_params("box_batch", rho, relax, eps, max_iter)
    if not (rho > 0 and np.isfinite(rho)):
        raise ValueError(f"box_batch: rho must be positive and finite (got {rho})")
    given = {k: np.asarray(v, dtype=npdt) for k, v in dict(x0=x0, q=q, r=r, qf=qf).items() if v is not None}
    if not given:   # the batch's own right-hand side, one instance per problem
        own = dict(x0=b.x0, q=b.q, r=b.r, qf=b.qf)
        given = {k: np.asarray(v, dtype=npdt)[:, None] for k, v in own.items() if v is not None}
    first = next(iter(given.values()))
    S = first.shape[1] if first.ndim >= 2 else 0
    if S < 1:
        raise ValueError("box_batch: right-hand sides are (batch, S, ...) with S >= 1")
    for k in ("x0", "qf"):
        if k in given and given[k].shape != (bt, S, n):
            raise ValueError(f"box_batch: {k} is (batch, S, n) = {(bt, S, n)} (got {given[k].shape})")
    knot = {k: given[k].ndim == 4 for k in ("q", "r") if k in given}
    if len(set(knot.values())) > 1:
        raise ValueError("box_batch: q and r carry a knot axis (batch, S, N-1, ·) both or neither")
    tvQR = int(any(knot.values()))
    for k, w in (("q", n), ("r", m)):
        want = (bt, S, N - 1, w) if tvQR else (bt, S, w)
        if k in given and given[k].shape != want:
            raise ValueError(f"box_batch: {k} is {want} (got {given[k].shape})")
    bounds = {}
    for k, v in (("u_lo", u_lo), ("u_hi", u_hi)):
        if v is None:
            bounds[k] = None
            continue
        try:
            bounds[k] = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=npdt), (bt, m))).reshape(-1)
        except ValueError:
            raise ValueError(f"box_batch: {k} is (batch, m) = {(bt, m)}, (m,) or a scalar (got {np.shape(v)})") from None
    zw = {}
    for k, v in (("Z", Z), ("W", W)):
        if v is None:
            zw[k] = np.zeros(bt * S * (N - 1) * m, npdt)
        elif np.shape(v) != (bt, S, N - 1, m):
            raise ValueError(f"box_batch: {k} is (batch, S, N-1, m) = {(bt, S, N - 1, m)} (got {np.shape(v)})")
        else:
            zw[k] = np.array(v, dtype=npdt).reshape(-1)
    # one solve with R + ρI on every stored R knot, every P_k kept, and its factors
    R = np.asarray(b.R, dtype=np.float64)
    br = replace(b, R=R + rho * np.eye(m), M=b.M if b.M is not None else np.zeros(R.shape[:-2] + (m, n)))
    sol = solve_batch(br, dtype=dtype, all_P=True)
    fac = factor_batch(br, sol["P"], dtype=dtype)
    info = np.where(sol["info"] != 0, sol["info"], fac["info"]).astype(np.int32)
    flat = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=npdt)).reshape(-1)
    mat = lambda a: None if a is None else to_abi(np.asarray(a, dtype=npdt)).reshape(-1)
    ins = dict(A=mat(b.A), B=mat(b.B), c=flat(b.c), K=mat(sol["K"]), Einv=mat(fac["Einv"]), Pc=flat(fac["Pc"]))
    rh = {k: flat(given.get(k)) for k in ("q", "r", "qf", "x0")}
    out = dict(d=np.zeros(bt * S * (N - 1) * m, npdt), X=np.zeros(bt * S * N * n, npdt), U=np.zeros(bt * S * (N - 1) * m, npdt))
    iters = np.zeros(bt * S, np.int32)
    res = np.zeros(bt * S * 2, npdt)
    p = lambda a: None if a is None else a.ctypes.data
    fc = _lib.DpFactors(p(ins["K"]), p(ins["Einv"]), p(ins["Pc"]))
    rs = _lib.DpRhs(S, *[p(rh[k]) for k in ("q", "r", "qf", "x0")], p(out["d"]), None, p(out["X"]), p(out["U"]))
    bx = _lib.DpBox(rho, relax, eps_prim, eps_dual, max_iter, p(bounds["u_lo"]), p(bounds["u_hi"]), p(zw["Z"]), p(zw["W"]),
                    p(iters), p(res))
    desc = _lib.DpDesc(n, m, N, dtype, bt, 0, 0, tvAB, tvQR)
    rc = _lib.check(_lib.load().lqrx_dp_resolve_box_host(C.byref(desc), p(ins["A"]), p(ins["B"]), p(ins["c"]),
                                                         C.byref(fc), C.byref(rs), C.byref(bx)))
    sh = (bt, S, N - 1, m)
    Wo = zw["W"].reshape(sh)
    return dict(X=out["X"].reshape(bt, S, N, n), U=out["U"].reshape(sh), Z=zw["Z"].reshape(sh), W=Wo, Y=npdt(rho) * Wo,
                iters=iters.reshape(bt, S), res=res.reshape(bt, S, 2), info=info, rc=rc)


def dp_box_device(t: dict, N: int, fac: dict, rhs: dict, box: dict, stream: int | None = None,
                  out: dict | None = None) -> dict:
    """Device-pointer entry point of lqrx_dp_resolve_box on torch tensors already in ABI layout (flat,
    layout 0), in the manner of dp_resolve_device.

    t, fac as in dp_resolve_device; the factors are those of a solve with R + ρI.  rhs = dict(S=, q=, r=,
    qf=, x0=, tv_QR=, outputs=("d", "X", "U")): d is always among the outputs.  box = dict(rho=, relax=1.6,
    eps_prim=1e-6, eps_dual=1e-6, max_iter=500, u_lo=, u_hi=, Z=, W=, outputs=("iters", "res")): u_lo, u_hi
    (m·batch) optional; Z, W (m·(N−1)·S·batch, required) are updated in place: zeros are a cold start.
    `out` may hold preallocated d, X, U, iters (int32, S·batch), res (2·S·batch).  Returns the dict of the
    outputs asked for, Z, W and rc.  `stream` is a raw hipStream_t; None = the null stream, synchronous.
    The call allocates nothing inside the library."""
    import torch

    outputs = tuple(rhs.get("outputs", _BOX_RHS_OUT))
    if "d" not in outputs or any(k not in _BOX_RHS_OUT for k in outputs):
        raise ValueError(f"dp_box_device: rhs outputs name d and any of {_BOX_RHS_OUT[1:]} (got {outputs})")
    box_out = tuple(box.get("outputs", _BOX_OUT))
    if any(k not in _BOX_OUT for k in box_out):
        raise ValueError(f"dp_box_device: box outputs name any of {_BOX_OUT} (got {box_out})")
    n, m, bt = t["n"], t["m"], t["batch"]
    tdt = t["A"].dtype
    dtype = _lib.F64 if tdt == torch.float64 else _lib.F32
    dev = t["A"].device
    S = int(rhs["S"])
    if box.get("rho") is None:
        raise ValueError("dp_box_device: box needs rho, the ρ of the solve the factors come from")
    rho, relax, eps_prim, eps_dual, max_iter = _box_params(
        "dp_box_device", box["rho"], box.get("relax", 1.6), (box.get("eps_prim", 1e-6), box.get("eps_dual", 1e-6)),
        box.get("max_iter", 500))
    for k in ("Z", "W"):
        if box.get(k) is None or box[k].numel() != bt * S * (N - 1) * m or box[k].dtype != tdt:
            raise ValueError(f"dp_box_device: box[{k!r}] is a tensor of m·(N−1)·S·batch = {bt * S * (N - 1) * m} elements "
                             f"of the problem's dtype (zeros: a cold start)")
    for k in ("u_lo", "u_hi"):
        if box.get(k) is not None and box[k].numel() != bt * m:
            raise ValueError(f"dp_box_device: box[{k!r}] has {box[k].numel()} elements, expected m·batch = {bt * m}")
    sizes = dict(d=bt * S * (N - 1) * m, X=bt * S * N * n, U=bt * S * (N - 1) * m, iters=bt * S, res=2 * bt * S)
    out = {} if out is None else out
    for k in outputs + box_out:
        if out.get(k) is None:
            out[k] = torch.empty(sizes[k], dtype=torch.int32 if k == "iters" else tdt, device=dev)
    p = lambda x: None if x is None else x.data_ptr()
    fc = _lib.DpFactors(p(fac.get("K")), p(fac.get("Einv")), p(fac.get("Pc")))
    rs = _lib.DpRhs(S, *[p(rhs.get(k)) for k in ("q", "r", "qf", "x0")], p(out["d"]), None,
                    *[p(out[k]) if k in outputs else None for k in ("X", "U")])
    bx = _lib.DpBox(rho, relax, eps_prim, eps_dual, max_iter, p(box.get("u_lo")), p(box.get("u_hi")), p(box["Z"]),
                    p(box["W"]), *[p(out[k]) if k in box_out else None for k in _BOX_OUT])
    desc = _lib.DpDesc(n, m, N, dtype, bt, 0, 0, int(t.get("tv_AB", 0)), int(rhs.get("tv_QR", 0)))
    vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    rc = _lib.check(_lib.load().lqrx_dp_resolve_box(C.byref(desc), vp(t["A"]), vp(t["B"]), vp(t.get("c")), C.byref(fc),
                                                    C.byref(rs), C.byref(bx), C.c_void_p(stream) if stream else None))
    res = {k: out[k] for k in outputs + box_out}
    res.update(Z=box["Z"], W=box["W"], rc=rc)
    return res
