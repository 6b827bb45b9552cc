"""Guard-zone tests of lqrx_dp_costates and lqrx_dp_solve_adjoint: neither reads or writes outside
the documented extents of its arguments, and each writes every element of every output it is asked
for — the documented zeros gq_1 = 0, gQ_1 = 0 included.

The C entries are called through ctypes (lqrx.dp_adjoint_device allocates its own outputs).  Every
case runs the entry on plain exact-size tensors whose outputs are pre-filled with the guard pattern,
then on tensors from tests/guarded.py; guarded.check() must pass, the guarded outputs must be the
plain outputs bit for bit, and the plain outputs must meet checker (b) of tests/dp_adjoint_truth.py
(adjoint_abi, check_grads) at the project's TOL64 = 1e-10 / TOL32 = 1e-4 (4·TOL for the matrix
gradients, as tests/test_dp_adjoint_gpu.py).  With knot_stride_AB = 0, gA, gB and gc are the summed,
batch-sized arrays: the guard behind them is what would show a per-knot store.

Shapes (n, m, N, batch, tv_AB) and the construction of the problems, gX and gU are those of
tests/test_dp_adjoint_gpu.py (its `case`), without the N = 256 one; (6, 3, 4, 3, 0) is added in fp32.

Observed on an MI355X (every figure here is from the run kept in
profiles/r08/guards/guard_gpu_tests.log: the four test_guard_*_gpu.py files together, 314 cases,
4.09 s wall; the slowest case, 0.28 s, is the first, which loads the library).
No guard was touched and no output element was left unwritten.  Worst error on the scales of
dp_adjoint_truth.grad_errors: costates fp64 1.7e-15, fp32 3.1e-7; the eleven gradients fp64 4.1e-15,
fp32 8.6e-7.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from dp_adjoint_truth import FIELDS, adjoint_abi, check_grads
from guarded import check as guard_check, guard_all, pattern_filled
from test_dp_adjoint_gpu import case, dev, grads_logical, upload

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL32 = 1e-4
SHAPES = [(1, 1, 2, 3, 0), (4, 2, 6, 67, 1), (5, 2, 5, 3, 0), (17, 3, 4, 2, 0), (33, 17, 3, 2, 1),
          (64, 32, 3, 2, 0), (65, 33, 3, 2, 1), (130, 5, 3, 2, 0)]
CASES = [(sh, "f64") for sh in SHAPES] + [((6, 3, 4, 3, 0), "f32")]
IDS = ["x".join(map(str, sh)) + "-" + prec for sh, prec in CASES]
ADJ_IN = ("A", "B", "Q", "R", "M", "Qf")


def p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def bits(x):
    import torch

    return x.view({8: torch.int64, 4: torch.int32}[x.element_size()])


def same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def filled(like, sizes):
    import torch

    like_i = torch.empty(1, dtype=torch.int32, device="cuda:0")
    return {k: pattern_filled(like_i if k == "info" else like, sz) for k, sz in sizes.items()}


@functools.lru_cache(maxsize=None)
def plain_case(n, m, N, bt, tv_AB):
    """The shape's problem with M, q, r, qf = 0 (what NULL means) and checker (b)'s result for it."""
    d, gX, gU, _ = case(n, m, N, bt, tv_AB)
    d0 = dict(d)
    for k in ("M", "q", "r", "qf"):
        d0[k] = np.zeros_like(d[k])
    return d0, adjoint_abi(d0, N, gX, gU)


@pytest.mark.parametrize("null", [False, True], ids=["all-inputs", "null-M-q-r-qf"])
@pytest.mark.parametrize("shape,prec", CASES, ids=IDS)
def test_costates_touch_only_their_buffers(lqrx, gpu_ok, shape, prec, null):
    import torch
    from lqrx import _lib

    n, m, N, bt, tv_AB = shape
    npdt, tol = (np.float64, TOL64) if prec == "f64" else (np.float32, TOL32)
    if null:
        d, ref = plain_case(*shape)
    else:
        d, _, _, ref = case(*shape)
    t = upload(d, npdt)
    sol = lqrx.dp_solve_device(t, N)                              # the solve whose K, X, U are swept
    assert (sol["info"] == 0).all().item()
    names = ("A", "B", "Q", "R", "M", "Qf", "q", "r", "qf", "K", "X", "U")
    ins = {k: (sol[k] if k in sol else t[k]) for k in names}
    desc = _lib.DpDesc(n, m, N, _lib.F64 if prec == "f64" else _lib.F32, bt, 0, 0, tv_AB, 1)

    def call(i, lam):
        args = [None if (null and k in ("M", "q", "r", "qf")) else p(i[k]) for k in names]
        rc = lqrx.load().lqrx_dp_costates(C.byref(desc), *args, p(lam), None)
        assert rc == 0, lqrx.load().lqrx_last_error().decode()
        torch.cuda.synchronize()

    plain = filled(t["A"], dict(lam=bt * N * n))
    call(ins, plain["lam"])
    hs = []
    ig = guard_all({k: v for k, v in ins.items() if not (null and k in ("M", "q", "r", "qf"))}, "in", bt, hs)
    og = guard_all(filled(t["A"], dict(lam=bt * N * n)), "out", bt, hs)
    call(ig, og["lam"])
    guard_check(hs)
    assert same_bits(og["lam"], plain["lam"])
    lam = plain["lam"].cpu().numpy().astype(np.float64).reshape(bt, N, n)
    e = check_grads(dict(lam=lam), ref, tol, f"costates {shape} {prec} null={null}")
    print(f"PARITY adjoint costates {shape} {prec} worst {max(e.values()):.2e}")


@pytest.mark.parametrize("shape,prec", CASES, ids=IDS)
def test_adjoint_touches_only_its_buffers(lqrx, gpu_ok, shape, prec):
    """All eleven gradients and info guarded; then gB, gR, gx0 alone (the other eight NULL): the
    bits of the full call, guards intact."""
    import torch
    from lqrx import _lib
    from lqrx.autograd import _sizes

    n, m, N, bt, tv_AB = shape
    npdt, tol = (np.float64, TOL64) if prec == "f64" else (np.float32, TOL32)
    d, gX, gU, ref = case(*shape)
    t = upload(d, npdt)
    sol = lqrx.dp_solve_device(t, N, costates=True)
    assert (sol["info"] == 0).all().item()
    ins = {k: t[k] for k in ADJ_IN}
    ins.update(X=sol["X"], U=sol["U"], lam=sol["lam"], gX=dev(gX, npdt), gU=dev(gU, npdt))
    sizes = {k: bt * v for k, v in _sizes(n, m, N, tv_AB).items()}
    assert set(sizes) == set(FIELDS)
    if not tv_AB:   # summed over the knots: one matrix (vector) per trajectory
        assert (sizes["A"], sizes["B"], sizes["c"]) == (bt * n * n, bt * n * m, bt * n)
    desc = _lib.DpDesc(n, m, N, _lib.F64 if prec == "f64" else _lib.F32, bt, 0, 0, tv_AB, 1)
    order = ("A", "B", "c", "Q", "R", "M", "Qf", "x0", "q", "r", "qf")     # lqrx_dp_grad's outputs

    def call(i, o):
        g = _lib.DpGrad(i["gX"].data_ptr(), i["gU"].data_ptr(),
                        *[o[k].data_ptr() if k in o else None for k in order])
        rc = lqrx.load().lqrx_dp_solve_adjoint(C.byref(desc), *[p(i[k]) for k in ADJ_IN], p(i["X"]), p(i["U"]),
                                               p(i["lam"]), C.byref(g), p(o["info"]), None)
        assert rc == 0, lqrx.load().lqrx_last_error().decode()
        torch.cuda.synchronize()

    sizes_i = dict(sizes, info=bt)
    plain = filled(t["A"], sizes_i)
    call(ins, plain)

    hs = []
    ig = guard_all(ins, "in", bt, hs)
    og = guard_all(filled(t["A"], sizes_i), "out", bt, hs)
    assert len(hs) == len(ins) + 12
    call(ig, og)
    guard_check(hs)
    for k in sizes_i:
        assert same_bits(og[k], plain[k]), k
    assert (plain["info"] == 0).all().item()

    hs3 = []
    ig3 = guard_all(ins, "in", bt, hs3)
    og3 = guard_all(filled(t["A"], {k: sizes_i[k] for k in ("B", "R", "x0", "info")}), "out", bt, hs3)
    call(ig3, og3)
    guard_check(hs3)
    for k in ("B", "R", "x0", "info"):
        assert same_bits(og3[k], plain[k]), k

    got = grads_logical({k: plain[k] for k in FIELDS}, n, m, N, bt, tv_AB)
    e = check_grads(got, ref, tol, f"adjoint {shape} {prec}")
    print(f"PARITY adjoint grads {shape} {prec} worst {max(e.values()):.2e}")
    # x'_1 = 0: gq_1 and gQ_1 are written zeros (guard_check has shown they are not leftover pattern)
    assert (got["q"][:, 0] == 0).all() and (got["Q"][:, 0] == 0).all()
