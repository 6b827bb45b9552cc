"""Guard-zone tests of lqrx_ls_solve and lqrx_sqp_solve (device entries): neither reads or writes
outside the documented extents of its arguments, and each writes every element of its outputs.

As in tests/test_guard_dp_gpu.py every case runs the entry on plain exact-size tensors whose
outputs hold the guard pattern, then on tensors from tests/guarded.py; guarded.check() passes, the
guarded outputs are the plain ones bit for bit, and the plain outputs meet the oracle exactly as
the neighbouring files measure it:
  LS   tests/test_ls.py — U, X within 1e-9 of oracle/ls_oracle.py per trajectory (cond(H) ≤ 1e6,
       else 1e-14·cond as test_ls_gpu_big_path_parity), Ā and b̄ within 1e-12 of buildAb;
  SQP  tests/test_sqp.py — status and iters equal, z and λ within 1e-9 (Dubins) / 1e-8 (cartpole,
       DoubleIntegrator) of oracle/sqp_oracle.py.
SQP: Z is in/out (NaN guards, real payload); lam of a trajectory that accepted no step (iters = 0)
is unspecified (include/lqrx.h) and exempt from the "written" check — every case here starts from
a guess that needs at least one step, and asserts that it did.

Observed on an MI355X (every figure here is from the run kept in
profiles/r08/guards/guard_gpu_tests.log: the four test_guard_*_gpu.py files together, 314 cases,
4.09 s wall; the slowest case, 0.28 s, is the first, which loads the library).
No guard was touched and no output element was left unwritten; Ā's block upper triangle comes back as
written zeros, as buildAb! leaves it.  Worst error against the oracles: LS U, X 5.1e-16 at (2, 1, 2),
2.0e-13 at (3, 2, 5), 3.1e-13 at (2, 2, 98); SQP z, λ Dubins 6.3e-15 (10 steps), cartpole 1.3e-13
(4–5 steps), DoubleIntegrator(3) 2.5e-14 (1 step).  The three cases from tests/sqp_cases.py (padded
KKT bin, large-block KKT kernels), in a later run: no guard touched; Dubins with a stage row 1.3e-12,
DoubleIntegrator(1) 2.5e-15, DoubleIntegrator(3) with two stage rows 9.7e-12.
"""
import numpy as np
import pytest

from guarded import check as guard_check, guard_all, pattern_filled
from oracle import ls_oracle as LO
from oracle import sqp_oracle as S
from test_ls import _batch
from test_sqp import _cartpole, _double_integrator, _problem

pytestmark = pytest.mark.gpu


def bits(x):
    import torch

    return x.view({8: torch.int64, 4: torch.int32}[x.element_size()])


def same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def filled(sizes, int_keys=("info", "iters", "status")):
    import torch

    f = torch.empty(1, dtype=torch.float64, device="cuda:0")
    i = torch.empty(1, dtype=torch.int32, device="cuda:0")
    return {k: pattern_filled(i if k in int_keys else f, sz) for k, sz in sizes.items()}


@pytest.mark.parametrize("hu", [0, 2])
@pytest.mark.parametrize("n,m,N,bt", [(2, 1, 2, 3), (3, 2, 5, 5),      # LDS path
                                      (2, 2, 98, 2)])                   # Nm = 194 > 192: global-H path
def test_ls_solve_touches_only_its_buffers(lqrx, gpu_ok, n, m, N, bt, hu):
    import torch
    from lqrx import ls
    from lqrx.dp import to_abi

    rng = np.random.default_rng(7 * n + m + N)
    A, B, Q, R, Qf, x0 = _batch(rng, n, m, bt)
    t = {k: torch.from_numpy(to_abi(v).reshape(-1)).to("cuda:0") for k, v in dict(A=A, B=B, Q=Q, R=R, Qf=Qf).items()}
    t["x0"] = torch.from_numpy(np.ascontiguousarray(x0).reshape(-1)).to("cuda:0")
    t.update(n=n, m=m, batch=bt)
    sizes = dict(U=bt * (N - 1) * m, X=bt * N * n, info=bt, Ab=bt * N * n * (N - 1) * m, bb=bt * N * n)

    plain = ls.ls_solve_device(t, N, hu_mode=hu, out=filled(sizes), with_Ab=True)
    torch.cuda.synchronize()
    hs = []
    tg = guard_all(t, "in", bt, hs)
    og = guard_all(filled(sizes), "out", bt, hs)
    assert len(hs) == 6 + 5
    got = ls.ls_solve_device(tg, N, hu_mode=hu, out=og, with_Ab=True)
    assert got["rc"] == 0
    guard_check(hs)
    for k in sizes:
        assert same_bits(got[k], plain[k]), k
    assert (plain["info"] == 0).all().item()

    U = plain["U"].cpu().numpy().reshape(bt, N - 1, m)
    X = plain["X"].cpu().numpy().reshape(bt, N, n)
    Ab = plain["Ab"].cpu().numpy().reshape(bt, (N - 1) * m, N * n)
    bb = plain["bb"].cpu().numpy().reshape(bt, N * n)
    worst = 0.0
    for b in range(bt):
        o = LO.ls_solve(A[b], B[b], Q[b], R[b], Qf[b], x0[b], N, hu=hu)
        cond = np.linalg.cond(o["H"])
        tol = 1e-9 if cond <= 1e6 else 1e-15 * cond * 10
        eU = np.abs(U[b] - o["U"]).max() / np.abs(o["U"]).max()
        eX = np.abs(X[b] - o["X"]).max() / np.abs(o["X"]).max()
        Abr, bbr = LO.buildAb(A[b], B[b], Q[b], Qf[b], x0[b], N)
        eA = np.abs(Ab[b].T - Abr).max() / np.abs(Abr).max()
        eb = np.abs(bb[b] - bbr).max() / np.abs(bbr).max()
        worst = max(worst, eU, eX)
        print(f"ls {n},{m},{N} hu{hu} traj {b}: cond {cond:.1e} U {eU:.2e} X {eX:.2e} Abar {eA:.2e} bbar {eb:.2e}")
        assert eU <= tol and eX <= tol, (b, cond, eU, eX)
        assert eA <= 1e-12 and eb <= 1e-12, (b, eA, eb)
    print(f"PARITY ls {n}x{m}x{N} hu{hu} worst {worst:.2e}")


def _sqp_cases():
    import lqrx.sqp as Q

    def dubins():
        N = 4
        dt, x0, xf, probs, Z0 = _problem(N, 1.0, 2, 3)
        return Q.DubinsSQP(N, dt, mu=1.0), probs, Z0, x0, xf, 1e-9

    def cartpole():
        N, tf = 6, 2.0
        probs, Z0, x0, xf = _cartpole(N, 1.0, 3, 3, "gentle", tf)
        return Q.CartpoleSQP(N, tf=tf, mu=1.0), probs, Z0, x0, xf, 1e-8

    def di3():
        prob, probs, Z0, x0, xf = _double_integrator(3, 5, 10.0, 5, 3)
        return prob, probs, Z0, x0, xf, 1e-8

    def matrix(name):
        """a case of tests/sqp_cases.py: the padded-bin and whole-batch KKT routes' scratch carving"""
        import sqp_cases as C

        return lambda: (*C.case(name), C.tol(name))

    return dict(dubins=dubins, cartpole=cartpole, di3=di3, dubins_pk1=matrix("dubins_pk1_N4"),
                di1_pk0=matrix("di1_pk0_N4"), di3_pk2=matrix("di3_pk2_N8"))


@pytest.mark.parametrize("model", ["dubins", "cartpole", "di3", "dubins_pk1", "di1_pk0", "di3_pk2"])
def test_sqp_solve_touches_only_its_buffers(lqrx, gpu_ok, model):
    """Dubins N = 4, cartpole N = 6, DoubleIntegrator(3) N = 5 with its stage row; Dubins N = 4 with a
    stage row and DoubleIntegrator(1) N = 4 (padded KKT bin), DoubleIntegrator(3) N = 8 with two stage
    rows (large-block KKT kernels, whole batch); batch 3."""
    import torch
    import lqrx.sqp as Q

    prob, probs, Z0, x0, xf, tol = _sqp_cases()[model]()
    bt = Z0.shape[0]
    nlam = Q.num_multipliers(prob.N, prob.model, prob.stage_rows)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64).reshape(-1)).to("cuda:0")
    ins = dict(x0=up(x0), xf=up(xf))
    sizes = dict(lam=bt * nlam, iters=bt, status=bt)

    plain = dict(ins, Z=up(Z0).clone(), **filled(sizes))
    Q.sqp_solve_device(prob, plain)
    torch.cuda.synchronize()

    hs = []
    g = guard_all(ins, "in", bt, hs)
    g.update(guard_all(dict(Z=up(Z0)), "inout", bt, hs))
    g.update(guard_all(filled(sizes), "out", bt, hs))
    assert sorted(h.name for h in hs) == ["Z", "iters", "lam", "status", "x0", "xf"]
    Q.sqp_solve_device(prob, g)
    torch.cuda.synchronize()
    iters = plain["iters"].cpu().numpy()
    assert (iters >= 1).all(), iters            # every guess needed a step
    lam_h = next(h for h in hs if h.name == "lam")
    lam_h.unspecified = np.repeat(g["iters"].cpu().numpy() == 0, nlam)
    guard_check(hs)
    for k in ("Z", "lam", "iters", "status"):
        assert same_bits(g[k], plain[k]), k
    assert torch.isfinite(plain["Z"]).all().item()

    z = plain["Z"].cpu().numpy().reshape(bt, -1)
    lam = plain["lam"].cpu().numpy().reshape(bt, nlam)
    status = plain["status"].cpu().numpy()
    worst = 0.0
    for b in range(bt):
        r = S.solve(probs[b], Z0[b], iters=prob.max_iters, tol_p=prob.tol_p, tol_d=prob.tol_d)   # the defaults, or the case's
        assert status[b] == r["status"] and iters[b] == r["iters"], (b, status[b], r["status"], iters[b], r["iters"])
        ez = np.abs(z[b] - r["z"]).max() / np.abs(r["z"]).max()
        el = np.abs(lam[b] - r["lam"]).max() / max(np.abs(r["lam"]).max(), 1e-300) if r["iters"] else 0.0
        worst = max(worst, ez, el)
        print(f"sqp {model} traj {b}: status {status[b]} iters {iters[b]} z {ez:.2e} lam {el:.2e}")
        assert ez <= tol and el <= tol, (b, ez, el)
    print(f"PARITY sqp {model} worst {worst:.2e}")
