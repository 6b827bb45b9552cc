"""CPU checks of the canonical-coordinates model (tests/dp_canon_truth.py): the
recursion the VAR_CANON kernel runs computes the gains and P_1 of the direct one.

  * against the longdouble reference recursion (oracle.dp_reference) and the direct float64 fast
    form, on the bench's problem family at (32, 16) and (16, 16), cond(B) swept to 1e6.  Bounds:
    a well-conditioned B leaves the canonical gain at rounding level (the sweep of DESIGN §3.1 sees
    ≤ 3e-14 up to cond 1e3), so 1e-12, a hundredth of the GPU tolerance 1e-10; at cond 1e6 a
    tenth of it, 1e-11 — the level at which the conditioning bound is set.  The direct form is held
    to the same bounds and the two to twice them against each other.  (No bound relative to the
    direct form's own error: K = S·K̃·Tᵀ may lose up to κ(B₁)·u where the direct form does not —
    2e-13 against 9e-15 at (16, 16), cond 1e6 — which is what the conditioning bound is for.)
  * the identities E = B₁ᵀẼB₁ (a congruence: the pivot test sees the same inertia) and
    K = S·K̃·Tᵀ against the direct recursion at 1e-12, relative per knot.
  * the exclusion rule: a B with a zero column, one with two equal columns, one past the bound.

Shapes: N = 48 (the recursion is at its fixed point long before), batch 2.
"""
import numpy as np
import pytest

import dp_canon_truth as ct
from dp_truth import relerr_per_knot

N, BT = 48, 2
_cache = {}


def family(lqrx, n, m):
    if (n, m) not in _cache:
        from lqrx.dp import abi_to_batch

        b = abi_to_batch(lqrx.random_batch(n, m, N, BT, seed=40 + n + m))
        _cache[(n, m)] = (b.A, b.B, b.Q, b.R, b.Qf)
    return _cache[(n, m)]


@pytest.mark.parametrize("n,m", [(32, 16), (16, 16)])
@pytest.mark.parametrize("cond,tol", [(None, 1e-12), (1e3, 1e-12), (1e6, 1e-11)])
def test_canonical_model_matches_reference(lqrx, oracle, n, m, cond, tol):
    A, B, Q, R, Qf = family(lqrx, n, m)
    if cond is not None:
        B = ct.with_cond(B, cond)
    ref = oracle.dp_reference(A, B, Q, R, Qf, N, dtype=np.longdouble)
    cn, dr = ct.dp_canon(A, B, Q, R, Qf, N), ct.dp_direct(A, B, Q, R, Qf, N)
    ld = lambda x: x.astype(np.longdouble)
    ek, ed = relerr_per_knot(ld(cn["K"]), ref["K"]), relerr_per_knot(ld(dr["K"]), ref["K"])
    ep = relerr_per_knot(ld(cn["P1"])[:, None], ref["P"][:, :1])
    print(f"n={n} m={m} cond(B)={cond}: K canonical {ek:.2e} direct {ed:.2e}  P1 canonical {ep:.2e}")
    assert ek <= tol and ep <= tol
    assert ed <= tol and relerr_per_knot(cn["K"], dr["K"]) <= 2 * tol


@pytest.mark.parametrize("n,m", [(32, 16), (16, 16)])
def test_identities(lqrx, n, m):
    A, B, Q, R, Qf = family(lqrx, n, m)
    cn, dr = ct.dp_canon(A, B, Q, R, Qf, N), ct.dp_direct(A, B, Q, R, Qf, N)
    s = cn["setup"]
    B1, S, T = s["B1"][:, None], s["S"][:, None], s["T"][:, None]
    sw = lambda M: np.swapaxes(M, -1, -2)
    eE = relerr_per_knot(sw(B1) @ cn["Et"] @ B1, dr["E"])
    eK = relerr_per_knot(S @ cn["Kt"] @ sw(T), dr["K"])
    # TᵀB = [B₁; 0] and S·B₁ = I: the set-up itself
    TB = sw(s["T"]) @ B
    e0 = max(np.abs(TB[:, m:]).max(initial=0.0), np.abs(TB[:, :m] - s["B1"]).max()) / np.abs(B).max()
    eS = np.abs(s["S"] @ s["B1"] - np.eye(m)).max()
    print(f"n={n} m={m}: E {eE:.2e}  K {eK:.2e}  TᵀB {e0:.2e}  S·B₁ {eS:.2e}")
    assert eE <= 1e-12 and eK <= 1e-12 and e0 <= 1e-12 and eS <= 1e-12


def test_conditioning_sweep_up_to_the_bound(lqrx):
    """The derivation of KAPPA_MAX, in short: kappa_sweep — both forms with the kernels'
    Newton–Schulz inverse against the longdouble recursion — at cond(B) up to the bound.  The
    canonical gain stays under a tenth of the 1e-10 tolerance at every point whose κ∞(B₁) the bound
    admits, and the last point is within a factor 4 of the bound."""
    rows = ct.kappa_sweep(family(lqrx, 32, 16), [1e3, 1e9, 8e12], N)
    for cond, kappa, ec, ed in rows:
        print(f"cond(B) {cond:.1e}: κ∞(B₁) {kappa:.2e}  canonical {ec:.2e}  direct {ed:.2e}")
        assert kappa <= ct.KAPPA_MAX and ec <= 1e-11
    assert rows[-1][1] >= ct.KAPPA_MAX / 4


def test_exclusion_rule(lqrx):
    _, B, *_ = family(lqrx, 32, 16)
    assert ct.canon_applies(B).all()
    zero = B.copy()
    zero[0][:, 5] = 0.0
    twin = B.copy()
    twin[1][:, 9] = twin[1][:, 2]
    assert list(ct.canon_applies(zero)) == [False, True]
    assert list(ct.canon_applies(twin)) == [True, False]
    assert list(ct.canon_applies(ct.with_cond(B, 1e15))) == [False, False]
    assert ct.canon_applies(ct.with_cond(B, 1e6)).all()
    # the bound sits where DESIGN §3.1 puts it: the library's constant
    import os, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "lqr.jl_amd", "csrc", "lqrx_internal.h")).read()
    assert float(re.search(r"DP_CANON_KAPPA_F64\s*=\s*([0-9.e+-]+);", src).group(1)) == ct.KAPPA_MAX
