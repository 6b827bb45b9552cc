"""GPU: the Riccati kernels' Newton–Schulz acceptance (lqrx_dp.hip NsTol / ns_round / ns_refine
and the AND-ed verdicts of dp_wg4_kernel) on inputs that take every path of the rule
— not only the exact sweep and the round-0 accept at the rounding floor that the rest of the suite
reaches.  Problems and the census of paths: tests/dp_drift_problems.py, tests/test_dp_ns_census.py.

Every case is one launch through lqrx.solve_batch(all_P=True) on the problem rounded to the
working precision, compared per trajectory and knot with oracle.dp_reference in longdouble
(K, P; d and p where the entry has linear terms) and, for the rollout, with its float64 run.
Every case asserts rc == 0, info == 0 and every stored P_k bitwise symmetric.

Criteria (none taken from the kernels' output):
  drift, jump  cond(E) ≤ 1e2; the reference's own error in the working precision must be
               ≤ tol/10, and then EVERY trajectory and knot meets the project's tolerance outright:
               1e-10 fp64, 1e-4 fp32, relative per knot (tests/test_dp_knot_gpu.py); d, p relative
               to their trajectory's max (tests/test_dp_linear_gpu.py); X, U within tol·max(1, |ref|).
  cond         the rule of assert_parity (tests/test_dp_lane_gpu.py): a trajectory beyond the
               tolerance passes iff its K and P error against longdouble is ≤ 4 × the error of the
               same recursion run in the working precision; fp64 trajectories with ε ≥ 1e-2 must
               meet 1e-10 outright; at most half of a batch may use the ratio rule.
  NS on / off  the drift batches of (32, 16) and (64, 32) fp64 solved by one child process with
               LQRX_DP_NS_OFF=1 (every knot the exact sweep) agree per knot with the parent's own
               solve within 1e-10: the iteration against the sweep, no reference in between.

Kernels reached (lqrx_dp.hip dp_launch): fp64 (16, 16) 1×1 tiles, (32, 16) the headline 2×1,
(17, 5) padded 2×1, (24, 18) 2×2, (48, 16) 4×2 tiles padded (no 3×1 grid is instantiated) — all
dp_riccati_kernel<VAR_TV> here — and (64, 32) time-varying: dp_wg4_kernel, four waves, verdicts
AND-ed; fp32 (32, 16) 2×1 and (64, 32) 4×2 of dp_riccati_kernel; linear (32, 16)
dp_riccati_kernel<VAR_TV | VAR_LIN>, linear (64, 32) dp_wg4_kernel with linear terms, affine
(32, 16) dp_riccati_kernel<VAR_TV | VAR_LIN | VAR_AFF>; cond (8, 16) 1×1 and (20, 32) 2×2 of the
time-invariant dp_riccati_kernel (Q + AᵀPA in the iteration's shadow), (70, 80) dp_big_kernel
(potrf + potrs, no iteration: the contrast; its P_ keeps the reference's op order and is not
mirrored, so bitwise symmetry is printed there, not asserted).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dp_drift_problems as D

pytestmark = pytest.mark.gpu

TOL = {0: 1e-10, 1: 1e-4}
_cache = {}


def _run(lqrx, oracle, case):
    """One launch and the three reference runs per case, shared and never modified."""
    if case not in _cache:
        dtype = case[5]
        p = D.rounded(D.problem(lqrx, case), dtype)
        got = lqrx.solve_batch(D.to_batch(p), dtype=dtype, all_P=True)
        ld = D.reference(oracle, p, np.longdouble)
        f64 = D.reference(oracle, p, np.float64)
        work = f64 if dtype == 0 else D.reference(oracle, p, np.float32)
        _cache[case] = (p, got, ld, work, f64)
    return _cache[case]


def _traj_rel(a, b):
    """(batch,) max|a − b| / max|b| over the whole trajectory (vectors that change sign)."""
    b = np.asarray(b)
    a = np.asarray(a, dtype=b.dtype).reshape(b.shape[0], -1)
    b = b.reshape(b.shape[0], -1)
    den = np.abs(b).max(axis=1)
    den[den == 0] = 1.0
    return (np.abs(a - b).max(axis=1) / den).astype(np.float64)


def _asymmetric(P):
    return [(t, k) for t in range(P.shape[0]) for k in range(P.shape[1]) if not np.array_equal(P[t, k], P[t, k].T)]


def _common(case, got, N, n, m, bt, symmetric=True):
    assert got["rc"] == 0 and (got["info"] == 0).all(), (got["rc"], got["info"])
    assert got["P"].shape == (bt, N, n, n) and got["K"].shape == (bt, N - 1, m, n)
    bad = _asymmetric(got["P"])
    if symmetric:
        assert not bad, f"P_k not bitwise symmetric at (trajectory, knot index) {bad[:6]}"
    else:
        print(f"FIG {D.case_id(case)}: {len(bad)} of {bt * N} stored P_k not bitwise symmetric (not asserted)")


def _rollout(got, f64, lim):
    """X, U against the float64 run of the reference; lim (batch,) relative to max(1, |ref|)."""
    out = []
    for k in ("X", "U"):
        r = f64[k]
        e = np.abs(got[k] - r).reshape(r.shape[0], -1).max(axis=1) / max(1.0, float(np.abs(r).max()))
        out.append(float(e.max()))
        assert (e <= lim).all(), (k, e, lim)
    return out


@pytest.mark.parametrize("case", D.DRIFT_CASES + D.JUMP_CASES + D.ENTRY_CASES, ids=D.case_id)
def test_well_conditioned_every_knot_within_tolerance(lqrx, oracle, gpu_ok, case):
    family, form, n, m, N, dtype, entry = case
    p, got, ld, work, f64 = _run(lqrx, oracle, case)
    bt, tol = p["B"].shape[0], TOL[dtype]
    _common(case, got, N, n, m, bt)
    assert (ld["info"] == 0).all() and (work["info"] == 0).all()
    e_work = np.maximum(D.per_knot_relerr(work["K"], ld["K"]).max(), D.per_knot_relerr(work["P"], ld["P"]).max())
    eK, eP = D.per_knot_relerr(got["K"], ld["K"]), D.per_knot_relerr(got["P"], ld["P"])
    fig = f"FIG {D.case_id(case)}: reference in working precision {e_work:.2e} | kernel K {eK.max():.2e} P {eP.max():.2e}"
    lin = entry != "plain"
    if lin:
        ed, ep = _traj_rel(got["d"], ld["d"]), _traj_rel(got["p"], ld["p"])
        e_work = max(e_work, _traj_rel(work["d"], ld["d"]).max(), _traj_rel(work["p"], ld["p"]).max())
        fig += f" d {ed.max():.2e} p {ep.max():.2e}"
    print(fig + f" | worst K per trajectory {' '.join(f'{x:.1e}' for x in eK.max(axis=1))} (param {p['param'].tolist()})")
    assert e_work <= tol / 10, "the problem is not well-conditioned enough to hold the kernel to tol"
    assert (eK <= tol).all(), np.argwhere(eK > tol)[:6]
    assert (eP <= tol).all(), np.argwhere(eP > tol)[:6]
    if lin:
        assert (ed <= tol).all() and (ep <= tol).all(), (ed, ep)
    eX, eU = _rollout(got, f64, np.full(bt, tol))
    print(f"FIG {D.case_id(case)}: rollout X {eX:.2e} U {eU:.2e}")


@pytest.mark.parametrize("case", D.COND_CASES + [D.COND_BIG_CASE], ids=D.case_id)
def test_ill_conditioned_no_worse_than_the_recursion(lqrx, oracle, gpu_ok, case):
    """Measured on MI355X (DESIGN.md §3.1 has the table): fp64 kernel/recursion error ratio ≤ 2.1
    wherever the tolerance is exceeded or approached; fp32 (8, 16) ε = 1e-2, Qf = 10 Q: kernel
    5.29e-4 against 1.33e-4, ratio 3.97 of the 4 allowed — the tightest figure here."""
    family, form, n, m, N, dtype, entry = case
    p, got, ld, work, f64 = _run(lqrx, oracle, case)
    bt, tol, eps = p["B"].shape[0], TOL[dtype], p["param"]
    _common(case, got, N, n, m, bt, symmetric=case != D.COND_BIG_CASE)
    assert (ld["info"] == 0).all() and (work["info"] == 0).all()
    e_work = np.maximum(D.per_traj_relerr(work["K"], ld["K"]), D.per_traj_relerr(work["P"], ld["P"]))
    e_gpu = np.maximum(D.per_traj_relerr(got["K"], ld["K"]), D.per_traj_relerr(got["P"], ld["P"]))
    ratio = e_gpu / np.maximum(e_work, 1e-300)
    for t in range(bt):
        print(f"FIG {D.case_id(case)}: eps {eps[t]:g} Qf {'P_inf' if t % 2 else '10Q'}: kernel {e_gpu[t]:.2e} "
              f"reference in working precision {e_work[t]:.2e} ratio {ratio[t]:.2f}")
    bad = e_gpu > tol
    lim = np.maximum(tol, 4.0 * e_work)
    assert (e_gpu <= lim).all(), (e_gpu, e_work)
    if dtype == 0:
        assert (e_gpu[eps >= 1e-2] <= tol).all(), e_gpu
    assert bad.mean() <= 0.5, bad
    _rollout(got, f64, lim)


_NS_OFF_CHILD = """
import sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path[:0] = [root + "/lqr.jl_amd", root, root + "/tests"]
import lqrx
import dp_drift_problems as D
res = {}
for i, case in enumerate(D.NS_OFF_CASES):
    got = lqrx.solve_batch(D.to_batch(D.rounded(D.problem(lqrx, case), case[5])), dtype=case[5], all_P=True)
    assert got["rc"] == 0 and (got["info"] == 0).all()
    res[f"K{i}"], res[f"P{i}"] = got["K"], got["P"]
np.savez(out, **res)
"""


def test_iteration_equals_exact_sweep(lqrx, oracle, gpu_ok, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "ns_off.npz")
    env = dict(os.environ, LQRX_DP_NS_OFF="1")
    r = subprocess.run([sys.executable, "-c", _NS_OFF_CHILD, root, out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    sweep = np.load(out)
    assert os.environ.get("LQRX_DP_NS_OFF") != "1", "the parent must run with the iteration on"
    for i, case in enumerate(D.NS_OFF_CASES):
        p, got, ld, work, f64 = _run(lqrx, oracle, case)
        eK, eP = D.per_knot_relerr(got["K"], sweep[f"K{i}"]), D.per_knot_relerr(got["P"], sweep[f"P{i}"])
        print(f"FIG ns-on vs ns-off {D.case_id(case)}: K {eK.max():.2e} P {eP.max():.2e}")
        assert not _asymmetric(sweep[f"P{i}"])
        assert (eK <= TOL[0]).all() and (eP <= TOL[0]).all(), (np.argwhere(eK > TOL[0])[:6], np.argwhere(eP > TOL[0])[:6])
