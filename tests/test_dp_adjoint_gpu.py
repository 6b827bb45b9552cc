"""GPU tests of the costates and the adjoint pass: lqrx_dp_costates, lqrx_dp_solve_adjoint and the
torch Function lqrx.lqr_solve.

Checkers: tests/dp_adjoint_truth.py — (b) adjoint_abi, the numpy float64 restatement of the
recursion, at every shape; (a) dense_adjoint_truth, torch float64 autograd through the dense KKT
solve, where N·(2n + m) ≤ 1000.  Both are pinned against each other in tests/test_dp_adjoint.py.

Tolerances (dp_adjoint_truth.grad_errors): λ and the vector gradients gq, gr, gqf, gc, gx0 are
direct solve outputs and take the project's TOL64 = 1e-10 / TOL32 = 1e-4 on their trajectory's
scale; every matrix gradient is a sum of two products of such quantities and takes 4·TOL on the
scale of its terms (gA: max|λ'|·max|x| + max|λ|·max|x'| per trajectory, times N−1 where the
output is summed over the knots).  A gradient that is itself a sum of N−1 per-knot terms is held
to N−1 times its per-knot scale — each term may be off by the bound: grad_errors does that for gA,
gB, gc of a time-invariant A, and the time-invariant torch test does it for gQ, gR, gM, gq, gr as
well, which torch sums over the broadcast knot axis (it divides those errors by N−1 before it
compares).  The issue states the per-knot bounds only; this is the one place they are scaled.
λ against the GPU's own P_k x_k + p_k is measured on max|λ| of the trajectory, the stationarity
residual on the sum of its four terms' largest entries over the trajectory; both take TOL64.

Worst errors observed on an MI355X (the largest of λ and the eleven gradients on those scales;
every figure here is from the run kept in profiles/r07/adjoint/adjoint_gpu_tests.log), per shape
(n, m, N, batch, tv_AB), fp64 against (b):
  (1,1,2,3,0) 7.9e-16   (4,2,6,67,1) 4.2e-15   (5,2,5,3,0) 1.6e-15   (16,16,4,2,1) 5.3e-15
  (17,3,4,2,0) 2.0e-15  (33,17,3,2,1) 3.6e-15  (64,32,3,2,0) 3.5e-15 (65,33,3,2,1) 3.3e-15
  (130,5,3,2,0) 3.8e-15 (32,16,256,3,1) 9.8e-15
fp64 against (a): worst 1.8e-13 (gqf at (130,5,3,2,0)), elsewhere ≤ 3e-14.
fp32 against (b) in float64: (6,3,30,7,0) 4.9e-6, (32,16,40,3,1) 2.8e-6, (64,32,3,2,0) 2.2e-6.
λ against the GPU's own P_k x_k + p_k: worst 4.2e-15 (at (32,16,256,3,1)); stationarity residual:
worst 7.9e-15 (at (130,5,3,2,0)).  The costates are formed by the closed-loop sweep
(include/lqrx.h): in numpy the textbook open-loop sweep misses TOL64 at n = 32, m = 16, N = 256 by
five decades (tests/test_dp_adjoint.py pins that).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from dp_adjoint_truth import (FIELDS, adjoint_abi, check_grads, dense_adjoint_truth, per_knot_problem,
                              sum_truth_like)
from dp_truth import cross_problem

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL32 = 1e-4
SHAPES = [
    (1, 1, 2, 3, 0),        # degenerate, one knot
    (4, 2, 6, 67, 1),       # small n, batch past 64 and not a multiple of anything
    (5, 2, 5, 3, 0),        # smallest register-tiled solve, padded
    (16, 16, 4, 2, 1),      # exact tile, m = n
    (17, 3, 4, 2, 0),       # two row tiles, padded
    (33, 17, 3, 2, 1),      # the costate kernel's 64-register staging (n > 32)
    (64, 32, 3, 2, 0),      # largest one-wave shape
    (65, 33, 3, 2, 1),      # workgroup solve, n past a wave's lanes
    (130, 5, 3, 2, 0),      # more than two strides of 64
    (32, 16, 256, 3, 1),    # full horizon, checker (b) only
]
F32_SHAPES = [(6, 3, 30, 7, 0), (32, 16, 40, 3, 1), (64, 32, 3, 2, 0)]
KEYS = ("A", "B", "Q", "R", "Qf", "x0", "q", "r", "qf", "c", "M")


@functools.lru_cache(maxsize=None)
def case(n, m, N, bt, tv_AB):
    """Problem, gX, gU and checker (b)'s result for a shape: computed once, shared, never modified."""
    import lqrx

    d = cross_problem(lqrx, n, m, N, bt, 6100 + 13 * n + m, tv_QR=True, tv_AB=bool(tv_AB))
    d["tv_QR"], d["tv_AB"] = 1, int(tv_AB)
    rng = np.random.default_rng(n * 1000 + N)
    gX, gU = rng.standard_normal((bt, N, n)), rng.standard_normal((bt, N - 1, m))
    return d, gX, gU, adjoint_abi(d, N, gX, gU)


def upload(d, dtype=np.float64):
    import torch

    t = {k: torch.from_numpy(np.asarray(d[k], dtype=dtype)).to("cuda:0") for k in KEYS}
    t.update(n=d["n"], m=d["m"], batch=d["batch"], tv_AB=d["tv_AB"], tv_QR=d["tv_QR"])
    return t


def dev(a, dtype=np.float64):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype)).reshape(-1)).to("cuda:0")


def grads_logical(g, n, m, N, bt, tv_AB):
    from lqrx.dp import from_abi

    kn = (bt, N - 1) if tv_AB else (bt,)
    host = lambda k: g[k].cpu().numpy().astype(np.float64)
    shp = dict(A=kn + (n, n), B=kn + (n, m), Q=(bt, N - 1, n, n), R=(bt, N - 1, m, m), M=(bt, N - 1, m, n),
               Qf=(bt, n, n))
    vshp = dict(c=kn + (n,), x0=(bt, n), q=(bt, N - 1, n), r=(bt, N - 1, m), qf=(bt, n))
    out = {k: from_abi(host(k), s) for k, s in shp.items() if k in g}
    out.update({k: host(k).reshape(s) for k, s in vshp.items() if k in g})
    return out


def solve_and_adjoint(lqrx, d, N, gX, gU, dtype=np.float64, want=FIELDS):
    t = upload(d, dtype)
    sol = lqrx.dp_solve_device(t, N, costates=True)
    g = lqrx.dp_adjoint_device(t, sol, dev(gX, dtype), dev(gU, dtype), want=want, N=N)
    return t, sol, g


@pytest.mark.parametrize("n,m,N,bt,tv_AB", SHAPES)
def test_costates(lqrx, gpu_ok, n, m, N, bt, tv_AB):
    """lqrx_dp_costates against (b); up to n = 64 also against the GPU's own P_k x_k + p_k of a
    p_mode = 1 solve; the stationarity residual of the GPU's own X, U, λ."""
    from lqrx.dp import from_abi

    d, gX, gU, ref = case(n, m, N, bt, tv_AB)
    t = upload(d)
    sol = lqrx.dp_solve_device(t, N, p_mode=1, costates=True)
    assert (sol["info"].cpu().numpy() == 0).all()
    lam = sol["lam"].cpu().numpy().reshape(bt, N, n)
    X, U = sol["X"].cpu().numpy().reshape(bt, N, n), sol["U"].cpu().numpy().reshape(bt, N - 1, m)
    check_grads(dict(lam=lam), ref, TOL64, f"costates {n},{m},{N},{bt},{tv_AB}")
    mx = lambda a: np.abs(a).reshape(bt, -1).max(axis=1)
    if n <= 64:
        # λ = P x + p on the trajectory's scale, max|λ| per trajectory, like the comparison with (b)
        P = from_abi(sol["P"].cpu().numpy(), (bt, N, n, n))
        p = sol["p"].cpu().numpy().reshape(bt, N, n)
        e = mx(lam - ((P @ X[..., None])[..., 0] + p)) / mx(lam)
        print("P x + p", e.max())
        assert e.max() <= TOL64
    # stationarity R u + M x + r + Bᵀλ_{k+1} = 0, on the sum of its four terms' largest entries over
    # the trajectory (the measure of tests/test_dp_adjoint.py)
    kab = N - 1 if tv_AB else 1
    B = from_abi(d["B"], (bt, kab, n, m))
    R, M = from_abi(d["R"], (bt, N - 1, m, m)), from_abi(d["M"], (bt, N - 1, m, n))
    r = d["r"].reshape(bt, N - 1, m)
    mv = lambda Z, v: (Z @ v[..., None])[..., 0]
    terms = [mv(R, U), mv(M, X[:, :N - 1]), r, mv(np.swapaxes(B, -1, -2), lam[:, 1:])]
    scale = sum(mx(t_) for t_ in terms)
    print("stationarity", (mx(sum(terms)) / scale).max())
    assert (mx(sum(terms)) / scale).max() <= TOL64


@pytest.mark.parametrize("n,m,N,bt,tv_AB", [(5, 2, 5, 3, 0), (4, 2, 6, 67, 1), (65, 33, 3, 2, 1)])
def test_costates_null_means_zero(lqrx, gpu_ok, n, m, N, bt, tv_AB):
    """A plain problem: M, q, r, qf = NULL gives the bits of explicit zeros."""
    import torch

    d = case(n, m, N, bt, tv_AB)[0]
    t = upload(d)
    plain = {k: t[k] for k in ("A", "B", "Q", "R", "Qf", "x0", "n", "m", "batch", "tv_AB", "tv_QR")}
    sol = lqrx.dp_solve_device(plain, N, costates=True)          # M, q, r, qf absent: NULL
    lam0 = torch.empty_like(sol["lam"])
    z = lambda k: torch.zeros_like(t[k])
    p = lambda x: C.c_void_p(x.data_ptr())
    from lqrx import _lib

    desc = _lib.DpDesc(n, m, N, 0, bt, 0, 0, tv_AB, 1)
    rc = lqrx.load().lqrx_dp_costates(C.byref(desc), p(t["A"]), p(t["B"]), p(t["Q"]), p(t["R"]), p(z("M")),
                                      p(t["Qf"]), p(z("q")), p(z("r")), p(z("qf")), p(sol["K"]), p(sol["X"]),
                                      p(sol["U"]), p(lam0), None)
    assert rc == 0
    assert sol["lam"].abs().max().item() > 0
    assert torch.equal(sol["lam"], lam0)


@pytest.mark.parametrize("n,m,N,bt,tv_AB", SHAPES)
def test_gradients_f64(lqrx, gpu_ok, n, m, N, bt, tv_AB):
    """All eleven gradients against (b); against (a) as well where N·(2n + m) ≤ 1000.  The adjoint's
    info equals the forward info (all zero)."""
    d, gX, gU, ref = case(n, m, N, bt, tv_AB)
    t, sol, g = solve_and_adjoint(lqrx, d, N, gX, gU)
    assert g["rc"] == 0
    assert (sol["info"].cpu().numpy() == 0).all() and (g["info"].cpu().numpy() == 0).all()
    assert (ref["info"] == 0).all() and (ref["info_adj"] == 0).all()
    got = grads_logical(g, n, m, N, bt, tv_AB)
    assert set(got) == set(FIELDS)
    got["lam"] = sol["lam"].cpu().numpy().reshape(bt, N, n)
    check_grads(got, ref, TOL64, f"f64 (b) {n},{m},{N},{bt},{tv_AB}")
    assert (got["q"][:, 0] == 0).all() and (got["Q"][:, 0] == 0).all()   # x'_1 = 0 exactly
    if N * (2 * n + m) <= 1000:
        ta = [dense_adjoint_truth(per_knot_problem(d, N, b), N, gX[b], gU[b]) for b in range(bt)]
        truth = dict(ref)
        truth["lam"] = np.stack([x["lam"] for x in ta])
        tg = [sum_truth_like(x["g"], d) for x in ta]
        truth["g"] = {k: np.stack([x[k] for x in tg]) for k in FIELDS}
        check_grads(got, truth, TOL64, f"f64 (a) {n},{m},{N},{bt},{tv_AB}")


@pytest.mark.parametrize("n,m,N,bt,tv_AB", F32_SHAPES)
def test_gradients_f32(lqrx, gpu_ok, n, m, N, bt, tv_AB):
    d, gX, gU, ref = case(n, m, N, bt, tv_AB)
    t, sol, g = solve_and_adjoint(lqrx, d, N, gX, gU, np.float32)
    assert (g["info"].cpu().numpy() == 0).all()
    got = grads_logical(g, n, m, N, bt, tv_AB)
    got["lam"] = sol["lam"].cpu().numpy().astype(np.float64).reshape(bt, N, n)
    check_grads(got, ref, TOL32, f"f32 (b) {n},{m},{N},{bt},{tv_AB}")


@pytest.mark.parametrize("n,m,N,bt,tv_AB", [(5, 2, 5, 3, 0), (33, 17, 3, 2, 1)])
def test_subset_of_outputs_same_bits(lqrx, gpu_ok, n, m, N, bt, tv_AB):
    """Only gB, gR, gx0: the bits of the full call.  Two identical calls: identical bits."""
    import torch

    d, gX, gU, _ = case(n, m, N, bt, tv_AB)
    t, sol, full = solve_and_adjoint(lqrx, d, N, gX, gU)
    again = lqrx.dp_adjoint_device(t, sol, dev(gX), dev(gU), N=N)
    part = lqrx.dp_adjoint_device(t, sol, dev(gX), dev(gU), want=("B", "R", "x0"), N=N)
    assert set(part) == {"B", "R", "x0", "info", "rc"}
    for k in FIELDS:
        assert torch.equal(full[k], again[k]), k
    for k in ("B", "R", "x0"):
        assert full[k].abs().max().item() > 0 and torch.equal(full[k], part[k]), k


def _torch_inputs(d, N, tv, dtype=None):
    """Logical torch leaves (requires_grad) of trajectory-batched problem d; tv: per-knot fields."""
    import torch
    from lqrx.dp import from_abi

    n, m, bt = d["n"], d["m"], d["batch"]
    k = N - 1
    mat = lambda key, r, c, per: from_abi(d[key], (bt, k, r, c) if per else (bt, r, c))
    a = dict(A=mat("A", n, n, tv), B=mat("B", n, m, tv), Q=mat("Q", n, n, tv), R=mat("R", m, m, tv),
             Qf=mat("Qf", n, n, False), x0=d["x0"].reshape(bt, n), M=mat("M", m, n, tv),
             q=d["q"].reshape((bt, k, n) if tv else (bt, n)), r=d["r"].reshape((bt, k, m) if tv else (bt, m)),
             qf=d["qf"].reshape(bt, n), c=d["c"].reshape((bt, k, n) if tv else (bt, n)))
    return {key: torch.tensor(np.ascontiguousarray(v), dtype=dtype or torch.float64, device="cuda:0",
                              requires_grad=True) for key, v in a.items()}


def test_torch_gradcheck(lqrx, gpu_ok):
    """torch.autograd.gradcheck of lqr_solve in fp64 at (3, 2, 4), batch 2, every input requiring
    grad, torch's defaults (eps 1e-6, atol 1e-5, rtol 1e-3, deterministic backward)."""
    import torch

    n, m, N, bt = 3, 2, 4, 2
    d = cross_problem(lqrx, n, m, N, bt, 31, tv_QR=True, tv_AB=True)
    a = _torch_inputs(d, N, True)
    order = ("A", "B", "Q", "R", "Qf", "x0", "q", "r", "qf", "c", "M")
    fn = lambda *v: lqrx.lqr_solve(*v[:6], N, q=v[6], r=v[7], qf=v[8], c=v[9], M=v[10])
    assert torch.autograd.gradcheck(fn, tuple(a[k] for k in order))


def test_torch_time_invariant_against_dense_truth(lqrx, gpu_ok):
    """Time-invariant inputs and a scalar loss: the broadcast-and-sum path against (a), on the
    default stream and on a created one (same bits); then the same in fp32 at TOL32."""
    import torch

    n, m, N, bt = 5, 2, 6, 3
    d = cross_problem(lqrx, n, m, N, bt, 47)
    d["tv_QR"], d["tv_AB"] = 0, 0
    rng = np.random.default_rng(3)
    gX, gU = rng.standard_normal((bt, N, n)), rng.standard_normal((bt, N - 1, m))
    ref = adjoint_abi(d, N, gX, gU)
    ta = [dense_adjoint_truth(per_knot_problem(d, N, b), N, gX[b], gU[b]) for b in range(bt)]
    # every time-invariant field's gradient is the sum over the knots
    tsum = {k: np.stack([x["g"][k].sum(axis=0) if k in ("A", "B", "c", "Q", "R", "M", "q", "r") else x["g"][k]
                         for x in ta]) for k in FIELDS}
    wX, wU = torch.tensor(gX, device="cuda:0"), torch.tensor(gU, device="cuda:0")

    def run(dtype=torch.float64):
        a = _torch_inputs(d, N, False, dtype)
        X, U = lqrx.lqr_solve(a["A"], a["B"], a["Q"], a["R"], a["Qf"], a["x0"], N, q=a["q"], r=a["r"], qf=a["qf"],
                              c=a["c"], M=a["M"])
        assert X.dtype == dtype and U.dtype == dtype
        ((X * wX.to(dtype)).sum() + (U * wU.to(dtype)).sum()).backward()
        return X.detach(), {k: a[k].grad for k in FIELDS}

    X0, g0 = run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        X1, g1 = run()
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    assert np.abs(X0.cpu().numpy() - ref["X"]).max() <= TOL64 * np.abs(ref["X"]).max()
    # sums of N−1 per-knot terms: the per-knot scales of grad_errors times N−1.  grad_errors applies
    # that factor to gA, gB, gc (their (bt, n, n) shape says summed); gQ, gR, gM, gq, gr are summed
    # here as well
    from dp_adjoint_truth import MATRIX_GRADS, grad_errors

    truth = dict(ref)
    truth["g"] = tsum
    X32, g32 = run(torch.float32)
    for what, g, tol in (("f64", g0, TOL64), ("f32", g32, TOL32)):
        assert all(g[k].dtype == (torch.float64 if what == "f64" else torch.float32) for k in FIELDS)
        e = grad_errors({k: g[k].cpu().numpy() for k in FIELDS}, truth)
        for k in ("Q", "R", "M", "q", "r"):
            e[k] /= (N - 1)
        print("torch time-invariant", what, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            assert v <= (4 * tol if k in MATRIX_GRADS else tol), (what, k, v)
    assert np.abs(X32.cpu().numpy() - ref["X"]).max() <= TOL32 * np.abs(ref["X"]).max()
    for k in FIELDS:
        assert torch.equal(g0[k], g1[k]), k
    assert torch.equal(X0, X1)


def test_torch_rejects_bad_shapes_and_reports_info(lqrx, gpu_ok):
    """lqr_solve checks every shape against (batch, n, m) and N before the kernels see a pointer, and
    raises when a trajectory's E is not positive definite (info ≠ 0) unless check_info=False."""
    import torch

    n, m, N, bt = 3, 2, 4, 2
    d = cross_problem(lqrx, n, m, N, bt, 31, tv_QR=True, tv_AB=True)
    a = {k: v.detach() for k, v in _torch_inputs(d, N, True).items()}
    call = lambda **kw: lqrx.lqr_solve(*[kw.get(k, a[k]) for k in ("A", "B", "Q", "R", "Qf", "x0")], kw.get("N", N),
                                       **{k: kw.get(k, a[k]) for k in ("q", "r", "qf", "c", "M")})
    call()
    for bad in (dict(N=N + 1), dict(A=a["A"][:, :2]), dict(Q=a["Q"][:, :, :2]), dict(x0=a["x0"][:1]),
                dict(q=a["q"][:, :2]), dict(M=a["M"].transpose(-1, -2)), dict(qf=a["qf"][:, :2]),
                dict(c=a["c"][:, 0]), dict(Qf=a["Qf"][:, :2, :2])):
        with pytest.raises(ValueError):
            call(**bad)
    R = a["R"].clone()
    R[1] = -R[1]
    with pytest.raises(RuntimeError, match="trajectory 1"):
        call(R=R)
    X, U = lqrx.lqr_solve(a["A"], a["B"], a["Q"], R, a["Qf"], a["x0"], N, check_info=False)
    assert torch.isfinite(X[0]).all()
    t = upload(d)
    sol = lqrx.dp_solve_device(t, N, costates=True)
    with pytest.raises(ValueError, match="gU"):
        lqrx.dp_adjoint_device(t, sol, torch.zeros(bt * N * n, dtype=torch.float64, device="cuda:0"),
                               torch.zeros(3, dtype=torch.float64, device="cuda:0"), N=N)
