"""Guard-zone tests of the KKT path, one case per kernel family: lqrx_kkt_solve and
lqrx_kkt_solve_ws read and write only the documented extents of Y, y, H, g, dz, lam, info — and,
for _ws, only the bytes lqrx_kkt_workspace_size reports — and write every element of dz, lam, info.

The KKT kernels address memory through buffer descriptors, whose num_records are code like any
other; tests/test_kkt_big_gpu.py::test_big_kkt_y_tail_nan pinned one kernel after an overrun was
found by hand, this file does it for every family.  Every case runs the entry on plain exact-size
tensors whose outputs hold the guard pattern, then on tensors from tests/guarded.py (inputs between
NaN guards, outputs pattern-filled between guards, the workspace exactly the reported size between
guards); guarded.check() passes, the guarded outputs are the plain ones bit for bit, info == 0, and
the plain outputs meet the oracle as the neighbouring files measure it (tests/kkt_truth.check):
fp64 1e-10 — on the batch's scale for the compile-time, direct and padded kernels
(tests/test_kkt_gpu.py, test_kkt_pad_gpu.py), per trajectory for the large-block and workgroup
kernels (tests/test_kkt_big_gpu.py, test_kkt_wg_gpu.py) — and fp32 1e-4 per trajectory against the
oracle on the fp32-rounded inputs.  A structure with as many constraint rows as variables (a square
Jacobian: cartpole N = 5, (6, 2, N = 4), (16, 8, N = 3)) takes kkt_truth's refined-truth rule — a
trajectory past the tolerance must be within 4·max(the oracle's own error, tol) of the refined truth —
as tests/test_kkt_gpu.py::test_kkt_fil_shapes does for its near-square structures: on the CPU the
oracle itself is up to 3.9e-10 from the truth at (6, 2, N = 4).

Structures whose shape the list below gives as (n, m, N) are the trajectory structure (initial
state, dynamics, goal) where that is well posed, n ≤ m·(N − 1); (5, 1, 4) and (67, 20, 3) are not
(more rows than variables: D H⁻¹ Dᵀ is singular), so they drop the goal rows, the "nogoal" kind of
tests/test_kkt_pad_gpu.py, which keeps the kernel family and the padding bin.  For the same reason the
stage-row case is ConstraintBlocks(7, 2, 5, [7, 1, 1, 1, 0]): with a goal block of 7 rows it would
have 45 rows for 43 variables, and the oracle itself reports info ≠ 0 on most of its trajectories.
(16, 8, N = 3) is square with a goal: fp64 runs it as it is, fp32 without the goal rows, because the
Schur complement of the square problem has cond(S) = 1.1e6 (numpy, on the fp32-rounded inputs), so
that eps32 · cond(S) = 6e-2 is past the 1e-4 bound whatever the kernel does (an fp32 run of it was
8.8e-3 from the oracle with every guard intact); without the goal cond(S) = 52.

Observed on an MI355X (every figure here is from the run kept in
profiles/r08/guards/guard_gpu_tests.log: the four test_guard_*_gpu.py files together, 314 cases,
4.09 s wall; the slowest case, 0.28 s, is the first, which loads the library).
No guard was touched — the workspace's included — and no output element was left unwritten.  Worst
error of dz, lam against the oracle per family (both entries give the same bits): compile-time shapes
Dubins 2.3e-12, cartpole N = 5 3.4e-9 (square; within the refined-truth rule); direct (6, 2, N = 4)
1.3e-9 in both layouts (square; likewise); padded bins 1.7e-12; large-block fp64 2.2e-11 ((16, 8, N = 3),
square), 2.6e-14 with stage rows, 1.3e-13 with dense H, fp32 1.7e-6; staged layout 1 2.3e-14; workgroup
fp64 6.8e-14, fp32 3.7e-6.
"""
import dataclasses
import functools

import numpy as np
import pytest

from guarded import check as guard_check, guard_all, guard_bytes, guarded, pattern_filled
from kkt_truth import check as truth_check
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-10
F32_TOL = 1e-4


def _nogoal(K, n, m, N):
    return K.ConstraintBlocks(n, m, N, [n] + [0] * (N - 2) + [0])


def _stage(K, n, m, N, ps):
    return K.ConstraintBlocks(n, m, N, [n] + [ps] * (N - 2) + [n])


# id → (structure, batch, h_mode, layout, dtype, dyn, scale, square Jacobian)
def _cases(K):
    traj, D, Z = K.trajectory_structure, K.H_DIAG, K.H_DENSE
    c = {}
    for bt in (1, 130):                                 # compile-time shapes (lqrx_kkt_fil.hip)
        for lay in (0, 1):
            for hm in (D, Z):
                c[f"dubins-N4-b{bt}-l{lay}-h{hm}"] = (K.dubins_structure(4), bt, hm, lay, "f64", "small", "batch", False)
    c["cartpole-N5-b67"] = (traj(4, 1, 5), 67, D, 0, "f64", "small", "batch", True)
    for lay in (0, 1):                                  # direct shapes
        c[f"direct-6x2-N4-b65-l{lay}"] = (traj(6, 2, 4), 65, D, lay, "f64", "small", "batch", True)
    c["pad-2x1-N4-b67"] = (traj(2, 1, 4), 67, D, 0, "f64", "small", "batch", False)          # padded bins
    c["pad-5x1-N4-b33"] = (_nogoal(K, 5, 1, 4), 33, D, 0, "f64", "small", "batch", False)
    c["pad-7x2-N5-stage-b31"] = (K.ConstraintBlocks(7, 2, 5, [7, 1, 1, 1, 0]), 31, D, 0, "f64", "small", "batch", False)
    c["big-16x8-N3-f64"] = (traj(16, 8, 3), 3, D, 0, "f64", "dense", "traj", True)          # large-block
    c["big-16x8-N3-f32"] = (_nogoal(K, 16, 8, 3), 3, D, 0, "f32", "dense", "traj", False)
    c["big-20x24-stage17-N4"] = (_stage(K, 20, 24, 4, 17), 3, D, 0, "f64", "dense", "traj", False)
    c["big-6x3-N4-denseH"] = (traj(6, 3, 4), 3, Z, 0, "f64", "small", "traj", False)
    c["staged-l1-5x3-N4-b5"] = (traj(5, 3, 4), 5, D, 1, "f64", "small", "batch", False)      # staged layout 1
    c["wg-67x20-N3-f32"] = (_nogoal(K, 67, 20, 3), 2, D, 0, "f32", "dense", "traj", False)   # workgroup
    c["wg-72x40-N3-f64"] = (traj(72, 40, 3), 2, D, 0, "f64", "dense", "traj", False)
    return c


def _case_ids():
    import lqrx.kkt as K          # structures only: does not load the library

    return list(_cases(K))


IDS = _case_ids()


@functools.lru_cache(maxsize=None)
def problem(cid):
    """The case's problem (fp32 cases: rounded to fp32) and the oracle's solve of it; shared by the
    two entries and never modified."""
    import lqrx.kkt as K

    st, bt, hm, lay, prec, dyn, scale, fb = _cases(K)[cid]
    pb = K.random_kkt(st, bt, seed=4100 + 13 * st.n + st.m + st.N + hm, h_mode=hm, dyn=dyn)
    if prec == "f32":
        f = lambda a: np.asarray(a, np.float32).astype(np.float64)
        pb = dataclasses.replace(pb, Y=f(pb.Y), y=f(pb.y), H=f(pb.H), g=f(pb.g))
    os_ = orc.KktStructure(st.n, st.m, st.N, st.p)
    r = orc.kkt_solve_batch(os_, bt, pb.Y, pb.y, pb.H, pb.g, h_mode=hm, ginv=1, nthreads=8)
    ref = dict(dz=r["dz"].reshape(bt, -1), lam=r["lam"].reshape(bt, -1), info=r["info"])
    return pb, ref


def same_bits(a, b):
    import torch

    v = lambda x: x.view({8: torch.int64, 4: torch.int32}[x.element_size()])
    return a.shape == b.shape and torch.equal(v(a), v(b))


@pytest.mark.parametrize("entry", ["solve", "solve_ws"])
@pytest.mark.parametrize("cid", IDS)
def test_kkt_solve_touches_only_its_buffers(lqrx, gpu_ok, cid, entry):
    import torch
    import lqrx.kkt as K

    st, bt, hm, lay, prec, dyn, scale, fb = _cases(K)[cid]
    pb, ref = problem(cid)
    assert (ref["info"] == 0).all()
    tdt, ldt, tol = (torch.float64, lqrx.F64, TOL) if prec == "f64" else (torch.float32, lqrx.F32, F32_TOL)
    arr = (lambda a: np.ascontiguousarray(np.asarray(a).reshape(bt, -1).T)) if lay == 1 else np.ascontiguousarray
    t = {k: torch.from_numpy(arr(getattr(pb, k)).reshape(-1)).to("cuda:0", tdt) for k in ("Y", "y", "H", "g")}
    t["batch"] = bt
    sY, sy, sH, sg = st.sizes(hm)
    sizes = dict(dz=bt * sg, lam=bt * sy, info=bt)
    like_i = torch.empty(1, dtype=torch.int32, device="cuda:0")
    outs = lambda: {k: pattern_filled(like_i if k == "info" else t["Y"], sz) for k, sz in sizes.items()}

    plain = K.kkt_solve_device(st, t, hm, out=outs(), layout=lay)
    torch.cuda.synchronize()
    assert plain["rc"] == 0

    hs = []
    tg = guard_all(t, "in", bt, hs)
    og = guard_all(outs(), "out", bt, hs)
    ws = None
    if entry == "solve_ws":
        nb = K.workspace_size(st, bt, hm, 1, lay, ldt)
        ws, h = guarded(torch.empty(nb, dtype=torch.uint8, device="cuda:0"), "ws", guard_bytes(nb, bt), "workspace")
        assert ws.numel() == nb
        hs.append(h)
    got = K.kkt_solve_device(st, tg, hm, out=og, workspace=ws, layout=lay)
    assert got["rc"] == 0
    guard_check(hs)
    for k in sizes:
        assert same_bits(got[k], plain[k]), (k, cid, entry)
    assert (plain["info"] == 0).all().item()

    unlay = (lambda a: a.reshape(-1, bt).T) if lay == 1 else (lambda a: a.reshape(bt, -1))
    host = {k: unlay(plain[k].double().cpu().numpy()) for k in ("dz", "lam")}
    den = lambda b: np.abs(b).max() if scale == "batch" else np.abs(b).max(axis=1)
    e = {k: float((np.abs(host[k] - ref[k]).max(axis=1) / den(ref[k])).max()) for k in ("dz", "lam")}
    print(f"PARITY kkt {cid} {entry} worst {max(e.values()):.2e} : dz {e['dz']:.2e} lam {e['lam']:.2e}")
    square = int((st.p + st.n2).sum()) >= int(st.w.sum())
    assert square == fb, cid
    truth_check(st, pb, 1, host, ref, tol, scale=scale, fallback=square)
