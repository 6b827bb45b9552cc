"""CPU checks of the pre-feedback model (tests/dp_canon_pf_truth.py): the recursion the
VAR_PREFB kernel runs is VAR_CANON's in other variables.

  * the identities on the bench's family at (32, 16): with Q′, M′ and C the canonical P̃_k of every
    knot, the canonical gain K̃ = K_v + A₁ and the ABI's K equal the VAR_CANON model's to rounding —
    1e-12 relative per knot, the bound tests/test_dp_canon.py holds its identities to — and Ẽ is the
    same to the rounding of its one addend P̃[0:m, 0:m] (the same 1e-12; the recursions differ in
    floating point, so P̃ does too);
  * the κ sweep behind the bound at three points under it: the modelled gain error (the kernels'
    Newton–Schulz acceptance, longdouble recursion as truth) stays ≤ 1e-11, the last of them within a
    factor 4 of the bound; and at cond(B) = 5e2, where the sweep of DESIGN §3.1 first reaches 1e-11,
    κ∞(B₁) is 4 times the bound;
  * the header's constant is the model's;
  * the exclusion rule: tiers 2, 1 and 0 for a well-conditioned B, cond(B) = 1e6 and a zero column.

Shapes: N = 48 (the recursion is at its fixed point long before), batch 2.
"""
import os
import re

import numpy as np

import dp_canon_pf_truth as pt
import dp_canon_truth as ct
from dp_truth import relerr_per_knot

N, BT, n, m = 48, 2, 32, 16
_cache = {}


def family(lqrx):
    if not _cache:
        from lqrx.dp import abi_to_batch

        b = abi_to_batch(lqrx.random_batch(n, m, N, BT, seed=88))
        _cache["f"] = (b.A, b.B, b.Q, b.R, b.Qf)
    return _cache["f"]


def test_identities(lqrx):
    fam = family(lqrx)
    pf, cn = pt.dp_canon_pf(*fam, N), ct.dp_canon(*fam, N)
    s, f = pf["setup"], pf["pf"]
    sw = lambda M: np.swapaxes(M, -1, -2)
    eK = relerr_per_knot(pf["K"], cn["K"])
    eKt = relerr_per_knot(pf["Kt"], cn["Kt"])
    eE = relerr_per_knot(pf["Et"], cn["Et"])
    eP1 = relerr_per_knot(pf["P1"][:, None], cn["P1"][:, None])
    # P̃_k of the pre-feedback recursion against the VAR_CANON recursion, replayed from its gains:
    # one knot from the pre-feedback P̃_{k+1}, in VAR_CANON's variables
    At, Qt, Rt = s["At"], s["Qt"], s["Rt"]
    eP = 0.0
    for k in range(N - 1, 0, -1):
        P = pf["Pt"][:, k]
        PA = P @ At
        G = PA[:, :m]
        Pn = Qt + sw(At) @ PA - sw(G) @ np.linalg.solve(Rt + P[:, :m, :m], G)
        eP = max(eP, float(relerr_per_knot(pf["Pt"][:, k - 1][:, None], ((Pn + sw(Pn)) / 2)[:, None])))
    # the set-up's own data: C = S·(T₁ᵀA) is S·A₁·Tᵀ, M′ = −R̃A₁, Q′ − Q̃ = A₁ᵀR̃A₁
    C2 = s["S"] @ f["A1"] @ sw(s["T"])
    eC = np.abs(f["C"] - C2).max() / np.abs(C2).max()
    eQ = np.abs(f["Qp"] - Qt - sw(f["A1"]) @ Rt @ f["A1"]).max() / np.abs(f["Qp"]).max()
    print(f"K {eK:.2e}  K̃ {eKt:.2e}  Ẽ {eE:.2e}  P̃_k {eP:.2e}  P1 {eP1:.2e}  C {eC:.2e}  Q′ {eQ:.2e}")
    assert max(eK, eKt, eE, eP, eP1, eC, eQ) <= 1e-12
    assert np.array_equal(f["Mp"], -(Rt @ f["A1"]))


def test_conditioning_sweep_up_to_the_bound(lqrx):
    """The derivation of KAPPA_PF_MAX, in short: under the bound the modelled gain error
    stays under a tenth of the 1e-10 tolerance; the sweep first reaches that tenth at cond(B) = 5e2,
    κ∞(B₁) = 1.9e3, and the bound is a factor 4 under it."""
    rows = pt.kappa_sweep(family(lqrx), [4.0, 30.0, 1e2, 5e2], N)
    for cond, kappa, ep, ec in rows:
        print(f"cond(B) {cond:.1e}: κ∞(B₁) {kappa:.2e}  pre-feedback {ep:.2e}  canonical {ec:.2e}")
    for cond, kappa, ep, ec in rows[:3]:
        assert kappa <= pt.KAPPA_PF_MAX and ep <= 1e-11
    assert rows[2][1] >= pt.KAPPA_PF_MAX / 4
    cond, kappa, ep, ec = rows[3]
    # (the error there is 1.0e-11 in the DESIGN table — printed, not asserted: it sits on the line)
    assert kappa / 4.1 <= pt.KAPPA_PF_MAX <= kappa / 3.9


def test_header_constant():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "lqr.jl_amd", "csrc", "lqrx_internal.h")).read()
    assert float(re.search(r"DP_PREFB_KAPPA_F64\s*=\s*([0-9.e+-]+);", src).group(1)) == pt.KAPPA_PF_MAX
    assert pt.KAPPA_PF_MAX < ct.KAPPA_MAX


def test_exclusion_rule(lqrx):
    _, B, *_ = family(lqrx)
    assert list(pt.tier(B)) == [2, 2]
    assert list(pt.tier(ct.with_cond(B, 1e6))) == [1, 1]
    zero = B.copy()
    zero[0][:, 5] = 0.0
    assert list(pt.tier(zero)) == [0, 2]
    assert list(pt.tier(ct.with_cond(B, 1e15))) == [0, 0]
    # the switch LQRX_DP_PREFB=0 is a zero bound: κ∞ ≥ 1, so nobody is admitted
    assert list(pt.tier(B, kappa_pf=0.0)) == [1, 1]
