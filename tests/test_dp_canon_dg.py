"""CPU checks of the diagonal-A₂₁ model (tests/dp_canon_dg_truth.py): the recursion the
VAR_DIAG kernel runs is VAR_PREFB's in a rotated basis.

  * the identities on the bench's family at (32, 16): P̃ rotated back, the ABI's K and P₁ equal the
    pre-feedback model's to rounding — 1e-12 relative per knot, the bound tests/test_dp_canon_pf.py holds
    its identities to; the lower-left block of T′ᵀAT′ is diagonal to the admission bound
    (OFFDIAG_MULT·ε·σ_max); T′ is orthogonal to the level of T: T's own defect plus what the Jacobi may add,
    16ε from the accepted cosines of U₂'s columns and ε per step of U₁'s at most 15·JACOBI_SWEEPS rotations;
  * the κ sweep behind the bound at three points under it: the modelled gain error (the kernels'
    Newton–Schulz acceptance, longdouble recursion as truth) stays ≤ 1e-11, the last of them within a
    factor 4 of the bound; and at cond(B) = 1.4e2, where the sweep of DESIGN §3.1 (N = 256) first reaches
    1e-11, κ∞(B₁) is 4 times the bound;
  * the header's constants are the model's;
  * the tier rule: 3, 2, 1 and 0 for B as generated, κ∞(B₁) between the two bounds, cond(B) = 1e6 and a
    zero column; 2 for a zero A₂₁; the switch;
  * the whole headline batch is admitted: all 65536 trajectories of the bench's default problem are
    tier 3 under the model's rule (about a minute and a half of numpy: the one slow test here, asked for
    as the condition of shipping the tier).

Shapes: N = 48 (the recursion is at its fixed point long before), batch 2.
"""
import os
import re

import numpy as np

import dp_canon_dg_truth as dg
import dp_canon_pf_truth as pt
import dp_canon_truth as ct
from dp_truth import relerr_per_knot

N, BT, n, m = 48, 2, 32, 16
EPS = np.finfo(np.float64).eps
_cache = {}


def family(lqrx):
    if not _cache:
        from lqrx.dp import abi_to_batch

        b = abi_to_batch(lqrx.random_batch(n, m, N, BT, seed=88))
        _cache["f"] = (b.A, b.B, b.Q, b.R, b.Qf)
    return _cache["f"]


def test_identities(lqrx):
    fam = family(lqrx)
    d, pf = dg.dp_canon_dg(*fam, N), pt.dp_canon_pf(*fam, N)
    s, r = d["setup"], d["setup"]["diag"]
    sw = lambda M: np.swapaxes(M, -1, -2)
    eK = relerr_per_knot(d["K"], pf["K"])
    eP1 = relerr_per_knot(d["P1"][:, None], pf["P1"][:, None])
    # P̃_k rotated back into the pre-feedback model's basis: D·P̃′·Dᵀ, D = diag(U₁, U₂)
    D = np.zeros((BT, n, n))
    D[:, :m, :m], D[:, m:, m:] = r["U1"], r["U2"]
    eP = max(float(relerr_per_knot((D @ d["Pt"][:, k] @ sw(D))[:, None], pf["Pt"][:, k][:, None])) for k in range(N))
    I = np.eye(n)
    eT, eTp = np.abs(sw(s["plain"]["T"]) @ s["plain"]["T"] - I).max(), np.abs(sw(s["T"]) @ s["T"] - I).max()
    smax = np.abs(r["sigma"]).max(axis=1)
    print(f"K {eK:.2e}  P̃_k {eP:.2e}  P1 {eP1:.2e}  TᵀT−I {eT:.2e}  T′ᵀT′−I {eTp:.2e}  "
          f"off-diagonal/(ε·σ_max) {(r['offdiag'] / (EPS * smax)).max():.1f}")
    assert max(eK, eP, eP1) <= 1e-12
    assert (r["offdiag"] <= dg.OFFDIAG_MULT * EPS * smax).all() and r["converged"].all()
    assert eTp <= eT + (16 + 15 * dg.JACOBI_SWEEPS) * EPS
    assert dg.admitted(r, s["kappa"]).all()


def test_conditioning_sweep_up_to_the_bound(lqrx):
    """The derivation of KAPPA_DG_MAX, in short: under the bound the modelled gain error
    stays under a tenth of the 1e-10 tolerance; the sweep first reaches that tenth at cond(B) = 1.4e2,
    κ∞(B₁) = 5.6e2, and the bound is a factor 4 under it."""
    rows = dg.kappa_sweep(family(lqrx), [4.0, 12.0, 25.0, 1.4e2], N)
    for cond, kappa, ed, ep in rows:
        print(f"cond(B) {cond:.1e}: κ∞(B₁) {kappa:.2e}  diagonal A₂₁ {ed:.2e}  pre-feedback {ep:.2e}")
    for cond, kappa, ed, ep in rows[:3]:
        assert kappa <= dg.KAPPA_DG_MAX and ed <= 1e-11
    assert rows[2][1] >= dg.KAPPA_DG_MAX / 4
    cond, kappa, ed, ep = rows[3]
    # (the error there is printed, not asserted: it sits on the line)
    assert kappa / 4.1 <= dg.KAPPA_DG_MAX <= kappa / 3.9


def test_header_constants():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "lqr.jl_amd", "csrc", "lqrx_internal.h")).read()
    val = lambda name: float(re.search(name + r"\s*=\s*([0-9.e+-]+)[;,]", src).group(1))
    assert val("DP_DIAG_KAPPA_F64") == dg.KAPPA_DG_MAX < pt.KAPPA_PF_MAX
    assert val("DP_DIAG_SWEEPS") == dg.JACOBI_SWEEPS and val("DP_DIAG_ROT_EPS") * EPS == dg.JACOBI_TOL
    assert val("DP_DIAG_OFF_EPS") == dg.OFFDIAG_MULT
    assert (val("DP_DIAG_SIGMA_LO"), val("DP_DIAG_SIGMA_HI")) == (dg.SIGMA_LO, dg.SIGMA_HI)


def test_tier_rule(lqrx):
    A, B, *_ = family(lqrx)
    assert list(dg.tier(A, B)) == [3, 3]
    mid = ct.with_cond(B, 60.0)                      # κ∞(B₁) between the two bounds
    kap = ct.canon_setup(A, mid, A, np.zeros((BT, m, m)), A)["kappa"]
    assert ((kap > dg.KAPPA_DG_MAX) & (kap <= pt.KAPPA_PF_MAX)).all() and list(dg.tier(A, mid)) == [2, 2]
    assert list(dg.tier(A, ct.with_cond(B, 1e6))) == [1, 1]
    zero = B.copy()
    zero[0][:, 5] = 0.0
    assert list(dg.tier(A, zero)) == [0, 3]
    # a zero A₂₁ has no σ > 0: the pre-feedback tier keeps it
    T = np.linalg.qr(B[1], mode="complete")[0]
    At = T.T @ A[1] @ T
    At[m:, :m] = 0.0
    A0 = A.copy()
    A0[1] = T @ At @ T.T
    assert list(dg.tier(A0, B)) == [3, 2]
    # the switches LQRX_DP_DIAG=0 and LQRX_DP_PREFB=0 are zero bounds: κ∞ ≥ 1, so nobody is admitted
    assert list(dg.tier(A, B, kappa_dg=0.0)) == [2, 2]
    assert list(dg.tier(A, B, kappa_pf=0.0, kappa_dg=0.0)) == [1, 1]


def test_headline_batch_is_admitted(lqrx):
    from lqrx.dp import abi_to_batch

    b = abi_to_batch(lqrx.random_batch(n, m, 256, 65536, seed=20260104))
    zq, zr = np.zeros((2048, n, n)), np.zeros((2048, m, m))
    count, kmax, omax = 0, 0.0, 0.0
    for i in range(0, 65536, 2048):
        A, B = b.A[i:i + 2048], b.B[i:i + 2048]
        s = ct.canon_setup(A, B, zq, zr, zq)
        r = dg.diag_setup(s, A, m)
        count += int(dg.admitted(r, s["kappa"]).sum())
        kmax = max(kmax, float(s["kappa"].max()))
        omax = max(omax, float((r["offdiag"] / (EPS * np.abs(r["sigma"]).max(axis=1))).max()))
    print(f"admitted {count} of 65536: κ∞(B₁) ≤ {kmax:.1f}, off-diagonal ≤ {omax:.1f}·ε·σ_max")
    assert count == 65536
