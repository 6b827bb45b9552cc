"""Gradients through the DP solve: the adjoint pass (lqrx_dp_solve_adjoint) and a torch
``Function`` on top of it.

For a loss ℓ(X, U) of the solution of the LQ problem of lqrx_dp_solve_cross, the gradient with
respect to every field of the problem is one more solve of the same problem with ∂ℓ/∂X, ∂ℓ/∂U as
linear cost terms (x0 = 0, c = 0), the costates of both solves and a rank-2 assembly — see
include/lqrx.h.  Everything runs in liblqrx.so on the current torch stream; there is no torch
fallback.

``dp_adjoint_device`` is the thin wrapper on ABI-layout tensors, ``lqr_solve`` the differentiable
solve on logical tensors.  torch is imported on first use, so the package imports without it.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .dp import dp_solve_device

__all__ = ["dp_adjoint_device", "lqr_solve", "GRAD_FIELDS"]

# the fields a gradient can be asked for, in the order of lqrx_dp_grad's outputs
GRAD_FIELDS = ("A", "B", "c", "Q", "R", "M", "Qf", "x0", "q", "r", "qf")


def _sizes(n, m, N, tv_AB):
    """Elements per trajectory of every gradient (the shape of its field; Q, R, M, q, r per knot)."""
    kab = N - 1 if tv_AB else 1
    return dict(A=n * n * kab, B=n * m * kab, c=n * kab, Q=n * n * (N - 1), R=m * m * (N - 1),
                M=m * n * (N - 1), Qf=n * n, x0=n, q=n * (N - 1), r=m * (N - 1), qf=n)


def dp_adjoint_device(t: dict, sol: dict, gX, gU, want=GRAD_FIELDS, N: int | None = None,
                      stream: int | None = None, info=None) -> dict:
    """lqrx_dp_solve_adjoint on torch tensors in ABI layout 0 (flat).

    t: the forward problem as for dp_solve_device — tensors A, B, Q, R, M, Qf on the GPU, ints n, m,
    batch, tv_AB (0 / 1); Q, R, M are per knot (tv_QR = 1 is required by the entry).
    sol: the forward solve's X, U and lam (dp_solve_device(…, costates=True)).
    gX (n·N·batch), gU (m·(N−1)·batch): ∂ℓ/∂X, ∂ℓ/∂U.
    want: the fields whose gradient is formed; every other pointer is passed as NULL.
    Returns {field: flat gradient tensor, …, "info": int32 (batch), "rc": return code}.  `stream`
    is a raw hipStream_t; None = the null stream, synchronous."""
    import torch

    lib = _lib.load()
    n, m, bt = t["n"], t["m"], t["batch"]
    tdt = t["A"].dtype
    if N is None:
        N = sol["X"].numel() // (bt * n)
    tv_AB = int(t.get("tv_AB", 0))
    bad = [k for k in want if k not in GRAD_FIELDS]
    if bad:
        raise ValueError(f"dp_adjoint_device: unknown gradient(s) {bad}; choose from {GRAD_FIELDS}")
    dev = t["A"].device
    sz = _sizes(n, m, N, tv_AB)
    need = dict(A=sz["A"], B=sz["B"], Q=sz["Q"], R=sz["R"], M=sz["M"], Qf=sz["Qf"])
    have = [(k, t[k]) for k in need] + [("X", sol["X"]), ("U", sol["U"]), ("lam", sol["lam"]), ("gX", gX), ("gU", gU)]
    need.update(X=n * N, U=m * (N - 1), lam=n * N, gX=n * N, gU=m * (N - 1))
    for k, v in have:   # a short buffer would be read past its end on the device
        if v.numel() != bt * need[k] or v.dtype != tdt or v.device != dev:
            raise ValueError(f"dp_adjoint_device: {k} must hold {bt * need[k]} elements of {tdt} on {dev} "
                             f"(got {v.numel()} of {v.dtype} on {v.device})")
    out = {k: torch.empty(bt * sz[k], dtype=tdt, device=dev) for k in GRAD_FIELDS if k in want}
    if info is None:
        info = torch.empty(bt, dtype=torch.int32, device=dev)
    gX, gU = gX.contiguous(), gU.contiguous()
    ptr = lambda k: out[k].data_ptr() if k in out else None
    g = _lib.DpGrad(gX.data_ptr(), gU.data_ptr(), *[ptr(k) for k in GRAD_FIELDS])
    d = _lib.DpDesc(n, m, N, _lib.F64 if tdt == torch.float64 else _lib.F32, bt, 0, 0, tv_AB,
                    int(t.get("tv_QR", 1)))
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = _lib.check(lib.lqrx_dp_solve_adjoint(C.byref(d), p(t["A"]), p(t["B"]), p(t["Q"]), p(t["R"]),
                                              p(t["M"]), p(t["Qf"]), p(sol["X"]), p(sol["U"]),
                                              p(sol["lam"]), C.byref(g), p(info),
                                              C.c_void_p(stream) if stream else None))
    out["info"] = info
    out["rc"] = rc
    return out


_FN = None


def _raise_on_info(info, what):
    """info ≠ 0 at any trajectory: its X, U or gradients are unspecified (this test synchronises)."""
    bad = (info != 0).nonzero().reshape(-1)
    if bad.numel():
        b = int(bad[0].item())
        raise RuntimeError(f"lqr_solve: {what} reports info = {int(info[b].item())} at trajectory {b} "
                           f"({bad.numel()} of {info.numel()} trajectories): E = R + BᵀPB is not positive "
                           "definite there, and that trajectory's results are unspecified")


def _expect(name, t, *shapes):
    if tuple(t.shape) not in shapes:
        raise ValueError(f"lqr_solve: {name} has shape {tuple(t.shape)}, expected "
                         + " or ".join(str(s) for s in shapes))


def _function():
    """The torch Function, built on first use (torch is not needed to import the package)."""
    global _FN
    if _FN is not None:
        return _FN
    import torch
    from torch.autograd.function import once_differentiable

    class _LqrSolve(torch.autograd.Function):
        # inputs: ABI-layout flat tensors in GRAD_FIELDS order, then n, m, N, batch, tv_AB
        @staticmethod
        def forward(ctx, A, B, c, Q, R, M, Qf, x0, q, r, qf, n, m, N, bt, tv_AB, check_info):
            t = dict(A=A, B=B, c=c, Q=Q, R=R, M=M, Qf=Qf, x0=x0, q=q, r=r, qf=qf, n=n, m=m, batch=bt,
                     tv_AB=tv_AB, tv_QR=1)
            st = torch.cuda.current_stream(A.device).cuda_stream
            with torch.cuda.device(A.device):
                out = dp_solve_device(t, N, stream=st or None, costates=True)
            if check_info:
                _raise_on_info(out["info"], "the solve")
            ctx.check_info = check_info
            ctx.save_for_backward(A, B, Q, R, M, Qf, out["X"], out["U"], out["lam"])
            ctx.dims = (n, m, N, bt, tv_AB)
            return out["X"].view(bt, N, n), out["U"].view(bt, N - 1, m)

        @staticmethod
        @once_differentiable
        def backward(ctx, gX, gU):
            A, B, Q, R, M, Qf, X, U, lam = ctx.saved_tensors
            n, m, N, bt, tv_AB = ctx.dims
            want = [k for k, need in zip(GRAD_FIELDS, ctx.needs_input_grad) if need]
            t = dict(A=A, B=B, Q=Q, R=R, M=M, Qf=Qf, n=n, m=m, batch=bt, tv_AB=tv_AB, tv_QR=1)
            st = torch.cuda.current_stream(A.device).cuda_stream
            with torch.cuda.device(A.device):
                g = dp_adjoint_device(t, dict(X=X, U=U, lam=lam), gX.reshape(-1), gU.reshape(-1), want, N,
                                      stream=st or None)
            if ctx.check_info:
                _raise_on_info(g["info"], "the adjoint solve")
            return tuple(g.get(k) for k in GRAD_FIELDS) + (None,) * 6

    _FN = _LqrSolve
    return _FN


def lqr_solve(A, B, Q, R, Qf, x0, N, *, q=None, r=None, qf=None, c=None, M=None, check_info=True):
    """Differentiable batched LQ solve on the GPU: returns (X (batch, N, n), U (batch, N−1, m)) of

        min Σ_k ½xᵀQ_k x + uᵀM_k x + ½uᵀR_k u + q_kᵀx + r_kᵀu  +  ½x_NᵀQf x_N + qfᵀx_N
        s.t. x_{k+1} = A_k x_k + B_k u_k + c_k,  x_1 = x0

    with gradients of any loss of (X, U) with respect to every tensor argument (fp64 or fp32).

    Logical torch tensors on the GPU: A (batch, n, n) or (batch, N−1, n, n), B and c with the same
    choice (A, B, c carry the knot axis together); Q (batch, n, n), R (batch, m, m), M (batch, m, n),
    q (batch, n), r (batch, m), each optionally with a knot axis (batch, N−1, …), independently;
    Qf (batch, n, n), qf (batch, n), x0 (batch, n).  Absent q, r, qf, c, M are zeros.

    Q, R and Qf enter as ½(Z + Zᵀ), formed here with torch ops: a perturbation of one entry then
    has a defined meaning, and torch carries that part of the gradient.  Time-invariant Q, R, M, q,
    r are broadcast over the knots before the solve, because the adjoint entry needs per-knot cost
    terms: that costs (n² + m² + mn + n + m)·(N−1) elements per trajectory of extra memory (an
    independent knot stride for q, r in the solve kernels would remove it); torch sums their
    gradient over the knot axis.  Forward: lqrx_dp_solve_cross and lqrx_dp_costates; backward
    (once differentiable): lqrx_dp_solve_adjoint, with NULL for every gradient that is not
    needed; all on the current torch stream.

    Every shape is checked against (batch, n, m) of B and against N before anything reaches the
    kernels.  With check_info (the default) the solve's info is tested after the forward pass and
    the adjoint solve's after the backward pass, and a RuntimeError names the first trajectory whose
    E = R + BᵀPB is not positive definite — its X, U and gradients are unspecified; the test reads
    info back and so synchronises the stream.  check_info=False skips it (no synchronisation, and
    such a trajectory then passes silently)."""
    import torch

    if not A.is_cuda:
        raise ValueError("lqr_solve: tensors must be on the GPU (there is no CPU path)")
    if A.dtype not in (torch.float64, torch.float32):
        raise ValueError("lqr_solve: dtype must be float64 or float32")
    if int(N) != N or N < 2:
        raise ValueError("lqr_solve: N must be an integer >= 2")
    N = int(N)
    if B.dim() not in (3, 4):
        raise ValueError("lqr_solve: B is (batch, n, m) or (batch, N-1, n, m)")
    bt, n, m = B.shape[0], B.shape[-2], B.shape[-1]
    tv_AB = int(A.dim() == 4)
    if (B.dim() == 4) != bool(tv_AB) or (c is not None and (c.dim() == 3) != bool(tv_AB)):
        raise ValueError("lqr_solve: A, B and c carry the knot axis (batch, N-1, …) together")
    k = (bt, N - 1)
    _expect("A", A, k + (n, n) if tv_AB else (bt, n, n))
    _expect("B", B, k + (n, m) if tv_AB else (bt, n, m))
    if c is not None:
        _expect("c", c, k + (n,) if tv_AB else (bt, n))
    _expect("Q", Q, (bt, n, n), k + (n, n))
    _expect("R", R, (bt, m, m), k + (m, m))
    _expect("Qf", Qf, (bt, n, n))
    _expect("x0", x0, (bt, n))
    for name, v, tail in (("M", M, (m, n)), ("q", q, (n,)), ("r", r, (m,))):
        if v is not None:
            _expect(name, v, (bt,) + tail, k + tail)
    if qf is not None:
        _expect("qf", qf, (bt, n))
    zeros = lambda *s: torch.zeros(*s, dtype=A.dtype, device=A.device)
    if c is None:
        c = zeros(bt, N - 1, n) if tv_AB else zeros(bt, n)
    sym = lambda Z: 0.5 * (Z + Z.transpose(-1, -2))

    def knots(Z, nd):   # broadcast a time-invariant field (nd trailing axes) over the knot axis
        if Z.dim() == nd + 2:
            return Z
        return Z.unsqueeze(1).expand(bt, N - 1, *Z.shape[1:])

    Qk, Rk = knots(sym(Q), 2), knots(sym(R), 2)
    Mk = knots(M if M is not None else zeros(bt, m, n), 2)
    qk = knots(q if q is not None else zeros(bt, n), 1)
    rk = knots(r if r is not None else zeros(bt, m), 1)
    qf = qf if qf is not None else zeros(bt, n)
    mat = lambda Z: Z.transpose(-1, -2).contiguous().reshape(-1)   # logical → column-major blocks
    vec = lambda v: v.contiguous().reshape(-1)
    args = (mat(A), mat(B), vec(c), mat(Qk), mat(Rk), mat(Mk), mat(sym(Qf)), vec(x0), vec(qk), vec(rk),
            vec(qf))
    if any(a.dtype != A.dtype or a.device != A.device for a in args):
        raise ValueError("lqr_solve: every tensor must share A's dtype and device")
    return _function().apply(*args, n, m, N, bt, tv_AB, bool(check_info))
