"""Which paths of the Newton–Schulz acceptance rule the committed problems of
tests/dp_drift_problems.py reach, by its numpy restatement of the rule (ns_paths).  No device is
needed; tests/test_dp_ns_regimes_gpu.py runs the kernels on the same problems.

A knot counts toward a path only with the factor-4 margin (every ρ it looked at is ≥ 4× away from
every threshold it was compared with): the restatement is not the kernel, a rounding difference
must not be able to move the knot.  Per family and precision every path must occur, except the
ones the rule or the family's parameters cannot reach with that margin:

  one_step, fp32   v = 3e-4 > one_step = 1e-5: a ρ that failed ρ ≤ v fails ρ ≤ one_step too; the
                   test after the update is dead code in fp32.
  cap, drift/jump  the exact step squares the residual (I − E(X + XR) = R²) and ρ ≥ ‖R‖∞, so a knot
                   that passed ρ < 1 with the margin (ρ0 ≤ 1/4) has ρ5 ≤ ρ0·‖R‖^31 ≤ 4^-32 ≪ v: on
                   a well-conditioned E the cap is unreachable.  It is reached where the rounding
                   floor of ρ itself is above the thresholds: cond, fp64, ε = 1e-6.
  cap, cond fp32   the floor at ε = 1e-2 is ρ ≈ 2e-4 … 6e-4, within the margin of v = 3e-4 (knots
                   there alternate between accept, one more round and the cap on rounding alone —
                   the GPU tests cover them, the census cannot count them); the ε list stops there.
  one_step, jump   before the jump ρ0 is at the floor (1e-14), at the jump ≫ 1, after it P's
                   transient moves E by ≥ 1e-3 per knot for the rest of a horizon N ≤ 24: no ρ0
                   falls into (1e-11, 1e-9].
"rounds2" is `rounds` with two or more updates.
"""
import numpy as np
import pytest

import dp_drift_problems as D

REQUIRED = {
    ("drift", 0): ("accept0", "one_step", "rounds", "rounds2", "reject"),
    ("drift", 1): ("accept0", "rounds", "rounds2", "reject"),
    ("jump", 0): ("accept0", "rounds", "rounds2", "reject"),
    ("jump", 1): ("accept0", "rounds", "rounds2", "reject"),
    ("cond", 0): ("accept0", "one_step", "rounds", "rounds2", "reject", "cap"),
    ("cond", 1): ("accept0", "rounds", "rounds2", "reject"),
}
CASES = {"drift": D.DRIFT_CASES + D.ENTRY_CASES, "jump": D.JUMP_CASES, "cond": D.COND_CASES}
_cache = {}


def _paths(lqrx, oracle, case):
    if case not in _cache:
        dtype = case[5]
        p = D.rounded(D.problem(lqrx, case), dtype)
        ref = D.reference(oracle, p, np.float64)
        assert (ref["info"] == 0).all()
        _cache[case] = D.ns_paths(p, ref["P"], dtype)
    return _cache[case]


def test_rule_constants_mirror_the_kernel():
    """NS_TOL restates NsTol of lqrx_dp.hip (tests/test_ns_keys.py mirrors the same constants)."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "lqr.jl_amd", "csrc", "lqrx_dp.hip"), encoding="utf-8").read()
    for dtype, ctype in ((0, "double"), (1, "float")):
        mm = re.search(r"NsTol<%s> \{\s*static constexpr %s v = ([0-9.e-]+)f?, one_step = ([0-9.e-]+)f?; "
                       r"static constexpr int it = (\d+);" % (ctype, ctype), src)
        assert mm, ctype
        assert (float(mm.group(1)), float(mm.group(2))) == D.NS_TOL[dtype]
        assert int(mm.group(3)) == D.NS_ROUNDS


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("family", ["drift", "jump", "cond"])
def test_every_path_is_reached(lqrx, oracle, family, dtype):
    total = {}
    for case in CASES[family]:
        if case[5] != dtype:
            continue
        res = _paths(lqrx, oracle, case)
        c = D.census(res)
        unclear = int((~res["clear"]).sum())
        print(f"{D.case_id(case):42s} " + " ".join(f"{k}={v}" for k, v in c.items())
              + f" no-margin={unclear} cond(E)<={res['condE'].max():.1e}")
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
        if family != "cond":
            assert res["condE"].max() <= 1e2, "drift and jump are well-conditioned by construction"
        if family != "jump":
            # trajectories of one launch on different paths
            per_traj = [set(res["path"][t][res["clear"][t]]) for t in range(res["path"].shape[0])]
            assert len({frozenset(s) for s in per_traj}) >= 2, per_traj
    print(f"{family} dtype={dtype} total: {total}")
    for name in REQUIRED[(family, dtype)]:
        assert total.get(name, 0) >= 1, f"{family} dtype={dtype}: no knot takes '{name}' with the margin"
    if dtype == 1:
        assert total["one_step"] == 0


def test_fp32_drift_has_knots_accepted_just_under_v(lqrx, oracle):
    """The loosest X the rule accepts: round-0 accepts with ρ0 in (v/2, v].  (Inside the margin of
    v, so the census above does not count them and the kernel may take one more round on some; the
    eighth δ of the fp32 list is there to supply them in numbers.)"""
    v = D.NS_TOL[1][0]
    total = 0
    for case in D.DRIFT_CASES:
        if case[5] == 1:
            res = _paths(lqrx, oracle, case)
            near = (res["path"] == D.ACCEPT0) & (res["rho0"] > v / 2)
            print(D.case_id(case), "accepted with rho0 in (v/2, v]: per trajectory", near.sum(axis=1).tolist())
            total += int(near.sum())
            if case[1] != "B":      # B_k = B(1 + a) moves E by ≈ 2a·BᵀPB, several times what R's drift does
                assert near[-1].sum() + near[2].sum() >= 1, "δ = 5e-5 and δ = 1e-4 supply none here"
    assert total >= 12


@pytest.mark.parametrize("case", D.JUMP_CASES, ids=D.case_id)
def test_jump_rejects_mid_horizon_and_restarts(lqrx, oracle, case):
    """At the jump knot j (and at j − 1, whose extrapolation still uses the inverse from before the
    jump) the rule rejects; every knot above j sits at the floor (accept in round 0); below j − 1
    the warm start is accepted again after some rounds: a rejection followed by a warm restart."""
    res = _paths(lqrx, oracle, case)
    p = D.problem(lqrx, case)
    N = case[4]
    for t, (j, i) in enumerate(p["param"].astype(int)):
        assert 2 < j < N - 2 and 2 < i < N - 2
        path = res["path"][t]
        assert path[j - 1] == D.REJECT and res["clear"][t, j - 1]
        assert all(path[k - 1] == D.ACCEPT0 for k in range(j + 1, N - 1)), (t, j, list(path))
        assert D.ROUNDS in set(path[: j - 2]), (t, j, list(path))
    assert len(set(p["param"][:, 0])) == len(p["param"]) and len(set(p["param"][:, 1])) == len(p["param"])


@pytest.mark.parametrize("case", D.COND_CASES + [D.COND_BIG_CASE], ids=D.case_id)
def test_cond_reference_alone_meets_the_gpu_criteria(lqrx, oracle, case):
    """The GPU test lets at most half of a cond batch pass on the ratio rule (error ≤ 4× that of
    the recursion in the working precision) and requires every fp64 trajectory with ε ≥ 1e-2 within
    1e-10 outright.  The reference recursion in the working precision must itself satisfy both,
    or no kernel could."""
    dtype = case[5]
    tol = 1e-4 if dtype else 1e-10
    p = D.rounded(D.problem(lqrx, case), dtype)
    ld = D.reference(oracle, p, np.longdouble)
    w = D.reference(oracle, p, D.NPDT[dtype])
    e = np.maximum(D.per_traj_relerr(w["K"], ld["K"]), D.per_traj_relerr(w["P"], ld["P"]))
    print(D.case_id(case), "eps", p["param"], "working-precision error", " ".join(f"{x:.1e}" for x in e))
    assert (e > tol).mean() <= 0.5
    if dtype == 0:
        assert (e[p["param"] >= 1e-2] <= tol / 10).all()
