"""SQP case matrix, CPU side (tests/sqp_cases.py; the device side is tests/test_sqp_matrix_gpu.py).

1. Oracle pinning for the (model, stage rows) combinations tests/test_sqp.py does not pin —
   Dubins with a stage row, DoubleIntegrator(1/2/3) without one, DoubleIntegrator(3) with two:
   the block assembly of oracle/sqp_oracle.py at a perturbed point, fed to the KAT-pinned block
   KKT oracle on the matching structure, reproduces the dense Newton step (ginv = 1) and the
   second-order correction (ginv = 0).  Tolerances are those of the neighbouring assembly tests:
   1e-10 (Dubins), 1e-9 for δz / 1e-8 for λ (DoubleIntegrator: dt = (N−1)/tf as the reference
   writes it).
2. The conditions every device-parity case must meet, so that parity tests the kernels and not
   the rounding of a tie: the oracle's smallest decision margin (every Armijo, SOC, backtrack and
   convergence comparison, oracle.sqp_oracle.new_trace) is ≥ 1e-6 relative, the constraint
   Jacobian at Z0 has σ_min/σ_max ≥ 1e-4, every trajectory accepts a step, the nonlinear cases
   have a trajectory with ≥ 3 steps; across the cases the SOC branch and a backtrack are taken;
   the cases on the KKT routes that solve the whole batch have trajectories stopping apart.
"""
import numpy as np
import pytest

import sqp_cases as C
from oracle import oracle as orc
from oracle import sqp_oracle as S

MARGIN, SIGMA = 1e-6, 1e-4


@pytest.mark.parametrize("name", C.PINNED)
def test_assembly_matches_kkt_oracle(name):
    prob, probs, Z0, _, _ = C.case(name)
    nx, nu, N, p = C.structure(name)
    st = orc.KktStructure(nx, nu, N, p)
    di = C.SPECS[name].family == "di"
    tz, tl = (1e-9, 1e-8) if di else (1e-10, 1e-10)
    # the data the case is there for: weights all different, stage_b nonzero, A_s ≠ its transpose's packing
    for v in (prob.Q, prob.R, prob.Qf):
        assert len(set(v)) == len(v)
    assert set(prob.Q) != set(prob.Qf)
    SA = np.asarray(prob.stage_A).reshape(prob.stage_rows, nx)
    assert all(b != 0.0 for b in prob.stage_b)
    if prob.stage_rows == 2:
        assert not np.array_equal(SA.ravel(), SA.T.ravel())
    rng = np.random.default_rng(4)
    for b, q in enumerate(probs):
        assert np.array_equal(q.SA, SA) and np.array_equal(q.Sb, prob.stage_b)
        z = Z0[b] + 0.05 * rng.standard_normal(Z0.shape[1])
        dz, lam = q.newton(z)
        Y, y, H, g = S.assemble(q, z)
        r = orc.kkt_solve_batch(st, 1, Y[None], y[None], H[None], g[None], h_mode=2, ginv=1, nthreads=1)
        assert np.abs(r["dz"].ravel() - dz).max() <= tz * np.abs(dz).max()
        assert np.abs(r["lam"].ravel() - lam).max() <= tl * np.abs(lam).max()
        # second-order correction = the ginv = 0 variant on the same blocks with y = c(z + dz)
        _, y2, _, _ = S.assemble(q, z + dz)
        r0 = orc.kkt_solve_batch(st, 1, Y[None], y2[None], H[None], g[None], h_mode=2, ginv=0, nthreads=1)
        soc = q.soc(z, dz)
        assert np.abs(r0["dz"].ravel() - soc).max() <= tz * max(np.abs(soc).max(), 1e-300)


def test_trace_leaves_the_solve_unchanged():
    """The optional trace records; the iterates, counts and return keys are those without it."""
    _, probs, Z0, _, _ = C.case("dubins_pk1_N4")
    plain = S.solve(probs[0], Z0[0], tol_d=1e-2)
    tr = S.new_trace()
    traced = S.solve(probs[0], Z0[0], tol_d=1e-2, trace=tr)
    assert sorted(plain) == sorted(traced) == ["hist", "iters", "lam", "soc", "status", "z"]
    assert plain["status"] == traced["status"] and plain["iters"] == traced["iters"] and plain["soc"] == traced["soc"]
    assert np.array_equal(plain["z"], traced["z"]) and np.array_equal(plain["lam"], traced["lam"])
    assert len(tr["lam"]) == len(tr["alpha"]) == plain["iters"] == len(plain["hist"]) - 1
    assert np.array_equal(tr["lam"][-1], plain["lam"])
    kinds = {k for _, k, _ in tr["margins"]}
    assert {"tol_p", "armijo"} <= kinds <= {"tol_p", "tol_d", "armijo", "soc", "backtrack"}


@pytest.mark.parametrize("name", C.GPU_CASES)
def test_case_is_well_posed(name):
    sp = C.SPECS[name]
    prob = C.case(name)[0]
    assert prob.N * prob.n + (prob.N - 1) * prob.m >= prob.n * (prob.N + 1) + prob.stage_rows * (prob.N - 2)
    iters = []
    for b in range(sp.batch):
        r, tr = C.reference(name, b)
        worst = min(tr["margins"], key=lambda m: m[2])
        assert worst[2] >= MARGIN, (b, worst)
        assert C.sigma_ratio(name, b) >= SIGMA, b
        assert r["iters"] >= 1, b
        iters.append(r["iters"])
    if name in C.NONLINEAR:
        assert max(iters) >= 3, iters


def test_cases_cover_the_line_search_and_the_frozen_trajectories():
    soc = [n for n in C.GPU_CASES for b in range(C.SPECS[n].batch) if any(C.reference(n, b)[0]["soc"])]
    back = [n for n in C.GPU_CASES for b in range(C.SPECS[n].batch)
            if any(a != 1.0 for a in C.reference(n, b)[1]["alpha"])]
    assert soc and back
    # whole-batch KKT routes: while some trajectories still iterate, others are frozen
    out = lambda n: {(C.reference(n, b)[0]["status"], C.reference(n, b)[0]["iters"]) for b in range(C.SPECS[n].batch)}
    assert len({it for _, it in out("dubins_pk0_N3")}) >= 2
    assert len({it for _, it in out("dubins_pk1_ragged")}) >= 3
    # DoubleIntegrator is linear-quadratic: a trajectory either converges with its first full
    # step or (μ too small for it) backtracks once and fails its second line search, so all
    # stop in iteration 1 — the converged ones at its check, frozen while the others run that
    # iteration's two KKT solves.
    assert out("di3_pk2_ragged") == {(0, 1), (2, 1)}


@pytest.mark.parametrize("name", ["dubins_pk1_ragged", "di3_pk2_ragged"])
def test_second_call_is_decided_with_margin(name):
    """The device test feeds a first call's result to a second call (λ restarts at zero): a
    trajectory that had converged is converged at entry there too, with the same margins."""
    prob, probs, _, _, _ = C.case(name)
    done = 0
    for b in range(C.SPECS[name].batch):
        r, _ = C.reference(name, b)
        if r["status"] != 0:
            continue
        tr = S.new_trace()
        r2 = S.solve(probs[b], r["z"], iters=prob.max_iters, tol_p=prob.tol_p, tol_d=prob.tol_d, trace=tr)
        assert r2["status"] == 0 and r2["iters"] == 0, b
        assert min(m for _, _, m in tr["margins"]) >= MARGIN, b
        done += 1
    assert 10 <= done <= C.SPECS[name].batch - 10
