"""GPU parity of the small-n lane-per-trajectory Riccati kernel (lqrx_dp_lane.hip, n ≤ 4,
m ≤ 4 — cartpole / Dubins / double-integrator shapes) and of the time-varying extension
(per-knot A_k, B_k, Q_k, R_k), through the C ABI, against the CPU
oracle (oracle/lqr_oracle.c, restating dynamic_programming.jl:28-72; the time-varying
variant indexes knot k's matrices in the same loop).

Tolerance (north star): 1e-10 relative per knot in fp64 for K and P, same for X, U;
fp32 1e-4 against the fp64 oracle.
"""
import numpy as np
import pytest

from dp_truth import relerr_per_knot
from test_dp_gpu import TOL32, TOL64, run_pair

pytestmark = pytest.mark.gpu


def per_traj_relerr(a, b):
    """(batch,) max over knots of max|a−b| / max|b| (per knot)."""
    a = a.reshape(a.shape[0], a.shape[1], -1)
    b = b.reshape(b.shape[0], b.shape[1], -1)
    den = np.abs(b).max(axis=2)
    den[den == 0] = 1.0
    return (np.abs(a - b).max(axis=2) / den).max(axis=1)


def assert_parity(got, ref, d, N, tol=TOL64, eps_ratio=1.0, rare=0.01, c=4.0):
    """K, P, X, U within `tol` per knot (vs the fp64 oracle) for every trajectory — except
    trajectories whose Riccati recursion is itself ill-conditioned.  The §8(d) generator
    A = I + 0.1/√n·G gives, at n ≤ 4, a few trajectories per thousand with ρ(A) ≈ 1.1 and
    weak actuation; on them the fp64 oracle (reference op order) is itself off the exact
    answer by up to ~3e-9 (measured against the same recursion in 80-bit extended precision,
    oracle.dp_extended).  Such a trajectory passes iff the kernel is no less accurate than
    the reference algorithm in fp64: its K/P error against the extended-precision solution
    is ≤ c × the oracle's own error (× eps(dtype)/eps(fp64) for fp32 runs), its X/U within
    c × that error of the oracle; and such trajectories are fewer than `rare`.  Measured on
    MI355X (round 2): 17 of 4101 cartpole-shaped random trajectories fall back to this rule,
    the kernel's error is ≤ 1.41× the oracle's own (fp64) and ≤ 2.0× its eps-scaled error
    (fp32) — c = 4 leaves headroom."""
    from lqrx.dp import abi_to_batch
    from oracle import oracle as orc

    got = {k: np.asarray(got[k], dtype=np.float64) for k in ("K", "P", "X", "U")}
    bt = got["K"].shape[0]
    xs = lambda a: a.reshape(bt, 1, -1)                 # X, U: one block per trajectory
    err = np.maximum.reduce([per_traj_relerr(got["K"], ref["K"]),
                             per_traj_relerr(got["P"], ref["P"]),
                             per_traj_relerr(xs(got["X"]), xs(ref["X"])),
                             per_traj_relerr(xs(got["U"]), xs(ref["U"]))])
    if (err <= tol).all():
        return
    b = abi_to_batch(d)
    Kx, Px = orc.dp_extended(b.A, b.B, b.Q, b.R, b.Qf, N)
    Px = Px if ref["P"].ndim == 4 else Px[:, 0]
    ld = lambda a: np.asarray(a, dtype=np.longdouble)
    pt = lambda a, x: per_traj_relerr(ld(a), x).astype(np.float64)
    P2 = (lambda a: a) if ref["P"].ndim == 4 else (lambda a: a[:, None])
    e_orc = np.maximum(pt(ref["K"], Kx), pt(P2(ref["P"]), P2(Px)))
    e_gpu = np.maximum(pt(got["K"], Kx), pt(P2(got["P"]), P2(Px)))
    bad = err > tol
    lim = np.maximum(tol, c * np.maximum(e_orc, 1e-16) * eps_ratio)
    ratio = e_gpu[bad] / np.maximum(e_orc[bad], 1e-300)
    print(f"\n{bad.sum()} of {bt} trajectories beyond {tol:g} vs the oracle; oracle's own error vs "
          f"80-bit up to {e_orc[bad].max():.2e}; kernel/oracle error ratio max {ratio.max():.2f}")
    assert (e_gpu[bad] <= lim[bad]).all(), (e_gpu[bad].max(), e_orc[bad].max())
    assert (err[bad] <= lim[bad]).all(), (err[bad].max(), e_orc[bad].max())
    assert bad.mean() < rare


@pytest.mark.parametrize("n,m,N,batch", [
    (4, 1, 101, 4096 + 5),   # cartpole shape (cfg2), ragged last wave
    (3, 2, 101, 130),        # Dubins shape
    (2, 1, 50, 64),          # double integrator 1-D
    (1, 1, 7, 3),
    (4, 4, 33, 65),
    (4, 3, 20, 9),
    (3, 1, 2, 11),           # N = 2: one backward knot
])
def test_lane_parity_f64(lqrx, oracle, gpu_ok, n, m, N, batch):
    seed = 300 + 11 * n + m
    got, ref = run_pair(lqrx, oracle, n, m, N, batch, seed=seed)
    assert got["rc"] == 0 and (got["info"] == 0).all()
    assert_parity(got, ref, lqrx.random_batch(n, m, N, batch, seed), N)


def test_lane_p1_only(lqrx, oracle, gpu_ok):
    got, ref = run_pair(lqrx, oracle, 4, 2, 40, 70, seed=9, all_P=False)
    assert relerr_per_knot(got["P"][:, None], ref["P"][:, None]) <= TOL64


@pytest.mark.parametrize("n,m", [(4, 1), (3, 2)])
def test_lane_parity_f32(lqrx, oracle, gpu_ok, n, m):
    got, ref = run_pair(lqrx, oracle, n, m, 60, 100, seed=78, dtype=1)
    assert_parity(got, ref, lqrx.random_batch(n, m, 60, 100, 78), 60, tol=TOL32,
                  eps_ratio=float(np.finfo(np.float32).eps / np.finfo(np.float64).eps),
                  rare=1.0)   # fp32 on weakly actuated random problems: the bound is conditioning


def test_lane_cartpole_problem(lqrx, oracle, gpu_ok):
    """cfg2 on the real RK3-linearised cartpole (test/cartpole.jl), per-trajectory x0."""
    from lqrx.dp import to_abi, from_abi
    from lqrx.models import cartpole_batch

    bt, N = 256, 101
    cb = cartpole_batch(bt, N, seed=5)
    got = lqrx.solve_batch(cb, all_P=True)
    d = {k: to_abi(getattr(cb, k)).ravel() for k in ("A", "B", "Q", "R", "Qf")}
    d.update(x0=cb.x0.ravel(), n=4, m=1, batch=bt)
    ref = oracle.dp_solve_abi(d, N, all_P=True)
    assert relerr_per_knot(got["K"], from_abi(ref["K"], (bt, N - 1, 1, 4))) <= TOL64
    assert relerr_per_knot(got["P"], from_abi(ref["P"], (bt, N, 4, 4))) <= TOL64
    assert np.abs(got["X"] - ref["X"].reshape(bt, N, 4)).max() <= TOL64


@pytest.mark.parametrize("mode", ["lane", "quad", "hex"])
def test_lane_non_spd_sets_info(lqrx, gpu_ok, monkeypatch, mode):
    from lqrx.dp import abi_to_batch

    monkeypatch.setenv("LQRX_DP_SMALL", mode)

    n, m, N, bt = 4, 2, 10, 70
    d = lqrx.random_batch(n, m, N, bt, seed=3)
    b = abi_to_batch(d)
    b.R[65] = -100.0 * np.eye(m)      # second wave, trajectory 1 is broken
    b.B[65] *= 1e-3
    got = lqrx.solve_batch(b)
    assert got["rc"] == 1
    assert got["info"][65] == N - 1
    assert (np.delete(got["info"], 65) == 0).all()


def _tv_batch(lqrx, n, m, N, bt, seed, tv_ab=True, tv_qr=True):
    """Per-knot A_k, B_k, Q_k, R_k: the time-invariant random problem perturbed per knot."""
    from lqrx.dp import abi_to_batch

    b = abi_to_batch(lqrx.random_batch(n, m, N, bt, seed))
    rng = np.random.default_rng(seed)
    if tv_ab:
        b.A = b.A[:, None] + 0.05 * rng.standard_normal((bt, N - 1, n, n)) / np.sqrt(n)
        b.B = b.B[:, None] + 0.05 * rng.standard_normal((bt, N - 1, n, m)) / np.sqrt(n)
    if tv_qr:
        s = 1.0 + 0.5 * rng.random((bt, N - 1, 1, 1))
        b.Q = b.Q[:, None] * s
        b.R = b.R[:, None] * (2.0 - s[..., :1, :1])
    return b


@pytest.mark.parametrize("n,m,tv_ab,tv_qr,N,bt", [
    (4, 1, True, True, 41, 67), (3, 2, True, False, 41, 67), (4, 4, False, True, 41, 67),
    # the MFMA kernel's VAR_TV variant (n ≥ 5): 1×1, 2×1 (cfg4 shape), padded, 4×2 tiles
    (6, 3, True, True, 30, 5), (32, 16, True, True, 40, 3), (20, 5, False, True, 25, 4),
    (17, 3, True, False, 12, 2), (64, 32, True, True, 9, 2)])
def test_time_varying_parity(lqrx, oracle, gpu_ok, n, m, tv_ab, tv_qr, N, bt):
    from lqrx.dp import to_abi, from_abi

    b = _tv_batch(lqrx, n, m, N, bt, seed=21 + n, tv_ab=tv_ab, tv_qr=tv_qr)
    got = lqrx.solve_batch(b, all_P=True)
    d = {k: to_abi(getattr(b, k)).ravel() for k in ("A", "B", "Q", "R", "Qf")}
    d.update(x0=b.x0.ravel(), n=n, m=m, batch=bt, tv_AB=int(tv_ab), tv_QR=int(tv_qr))
    ref = oracle.dp_solve_abi(d, N, all_P=True)
    assert got["rc"] == 0
    assert relerr_per_knot(got["K"], from_abi(ref["K"], (bt, N - 1, m, n))) <= TOL64
    assert relerr_per_knot(got["P"], from_abi(ref["P"], (bt, N, n, n))) <= TOL64
    refX = ref["X"].reshape(bt, N, n)
    assert np.abs(got["X"] - refX).max() <= TOL64 * max(1.0, np.abs(refX).max())


@pytest.mark.parametrize("mode", ["lane", "quad", "hex"])
@pytest.mark.parametrize("n,m,N,batch", [(4, 1, 101, 300), (3, 2, 60, 130), (4, 4, 20, 33),
                                         (4, 2, 30, 70), (2, 1, 25, 17), (4, 3, 40, 4100)])
def test_small_kernel_modes(lqrx, oracle, gpu_ok, monkeypatch, mode, n, m, N, batch):
    """The three small-n kernels — one lane per trajectory (dp_lane_kernel), one quad per
    trajectory (dp_quad_kernel, n ∈ {3, 4}, batch ≤ 16384) and sixteen lanes per trajectory
    (dp_hex_kernel, an A/B alternative) — against the oracle; LQRX_DP_SMALL selects
    the kernel per call."""
    if mode == "quad" and n < 3:
        pytest.skip("the quad kernel serves n in {3, 4}")
    monkeypatch.setenv("LQRX_DP_SMALL", mode)
    seed = 700 + 11 * n + m
    got, ref = run_pair(lqrx, oracle, n, m, N, batch, seed=seed, all_P=True)
    assert got["rc"] == 0 and (got["info"] == 0).all()
    assert_parity(got, ref, lqrx.random_batch(n, m, N, batch, seed), N)


def test_small_kernel_auto_large_batch(lqrx, oracle, gpu_ok):
    """batch > 16384 at n = 4 selects the lane kernel (auto; the quad kernel below)."""
    got, ref = run_pair(lqrx, oracle, 4, 1, 12, 16384 + 70, seed=77)
    assert got["rc"] == 0
    assert_parity(got, ref, lqrx.random_batch(4, 1, 12, 16384 + 70, 77), 12)


@pytest.mark.parametrize("n,m,N,k0", [(4, 2, 30, 17), (6, 3, 30, 17), (32, 16, 24, 9), (20, 5, 20, 11)])
def test_time_varying_info_middle_knot(lqrx, oracle, gpu_ok, n, m, N, k0):
    """An indefinite E = R_k + BᵀPB at a MIDDLE knot k0 of a time-varying problem (R_k0 =
    −100·I, B_k0 ≈ 0) is reported per trajectory as info = k0, as potrf's info at that knot
    (dynamic_programming.jl:29; the oracle reports the same).  On the MFMA kernel (n ≥ 5)
    knots after the first take the Newton–Schulz inverse; its residual test must reject the
    step and hand the knot to the pivoted LDLᵀ sweep that detects the definiteness flip.
    Knots solved before the break (k > k0, the backward sweep runs k = N−1 … 1) still match
    the oracle."""
    from lqrx.dp import to_abi, from_abi

    bt = 5
    b = _tv_batch(lqrx, n, m, N, bt, seed=55 + n, tv_ab=True, tv_qr=True)
    b.R = np.array(b.R)
    b.B = np.array(b.B)
    b.R[1, k0 - 1] = -100.0 * np.eye(m)             # knot k0 (index k0 − 1)
    b.B[1, k0 - 1] *= 1e-3
    got = lqrx.solve_batch(b, all_P=True)
    d = {k: to_abi(getattr(b, k)).ravel() for k in ("A", "B", "Q", "R", "Qf")}
    d.update(x0=b.x0.ravel(), n=n, m=m, batch=bt, tv_AB=1, tv_QR=1)
    ref = oracle.dp_solve_abi(d, N, all_P=True)
    assert ref["info"][1] == k0 and (np.delete(ref["info"], 1) == 0).all()
    assert got["rc"] == 1
    assert got["info"][1] == k0
    assert (np.delete(got["info"], 1) == 0).all()
    refK = from_abi(ref["K"], (bt, N - 1, m, n))
    ok = [0, 2, 3, 4]
    assert relerr_per_knot(got["K"][ok], refK[ok]) <= TOL64
    assert relerr_per_knot(got["K"][1:2, k0:], refK[1:2, k0:]) <= TOL64   # knots k0+1 … N−1


@pytest.mark.parametrize("n,m,N,mode", [(32, 16, 40, "all"), (32, 16, 40, "one"), (8, 4, 30, "all"),
                                        (6, 3, 60, "one"), (20, 5, 33, "slow"), (64, 32, 24, "one")])
def test_time_varying_info_gradual_indefiniteness(lqrx, oracle, gpu_ok, n, m, N, mode):
    """E = R_k + BᵀPB loses definiteness GRADUALLY along the horizon: R_k ramps linearly
    through zero (R_k = (2k/N − 1)·I, or only its last eigenvalue — "one" — or a slow ramp
    with an offset) with B_k scaled by 1e-2, so E's smallest eigenvalue crosses zero over
    several knots instead of flipping at one.  The MFMA kernel (n ≥ 5) inverts E by a
    warm-started Newton–Schulz iteration after the first knot; it must not converge onto the
    inverse of an indefinite E: info must equal the oracle's first failing knot (potrf's
    info, dynamic_programming.jl:29), and every knot solved before it must still match."""
    from lqrx.dp import to_abi, from_abi

    bt = 3
    b = _tv_batch(lqrx, n, m, N, bt, seed=91 + n, tv_ab=True, tv_qr=True)
    b.R = np.array(b.R)
    b.B = np.array(b.B) * 1e-2
    k = np.arange(1, N)                                   # knot k at index k − 1
    if mode == "slow":
        ramp = 0.3 * (k / N - 0.45)
    else:
        ramp = 2.0 * k / N - 1.0
    for t in (1, 2):                                      # trajectory 0 stays SPD
        for j, r in enumerate(ramp):
            if mode == "one":
                b.R[t, j] = np.eye(m)
                b.R[t, j, m - 1, m - 1] = r
            else:
                b.R[t, j] = r * np.eye(m)
    got = lqrx.solve_batch(b, all_P=True)
    d = {f: to_abi(getattr(b, f)).ravel() for f in ("A", "B", "Q", "R", "Qf")}
    d.update(x0=b.x0.ravel(), n=n, m=m, batch=bt, tv_AB=1, tv_QR=1)
    ref = oracle.dp_solve_abi(d, N, all_P=True)
    assert ref["info"][0] == 0 and ref["info"][1] > 0 and ref["info"][2] > 0
    assert list(got["info"]) == list(ref["info"]), (got["info"], ref["info"])
    assert got["rc"] == 1
    refK = from_abi(ref["K"], (bt, N - 1, m, n))
    assert relerr_per_knot(got["K"][:1], refK[:1]) <= TOL64
    for t in (1, 2):
        k0 = int(ref["info"][t])                          # knots k0+1 … N−1 solved before the break
        assert relerr_per_knot(got["K"][t:t + 1, k0:], refK[t:t + 1, k0:]) <= TOL64
