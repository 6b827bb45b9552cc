"""GPU parity along the leaves of the DP launch dispatch: kind × time-varying × layout × dtype, per
kernel family, on the public Python API (lqrx.solve_batch), N = 3.

The other DP suites reach the five kinds (plain ⊂ linear ⊂ affine ⊂ cross ⊂ value) through the
shapes each of them picked; this one walks what dp_launch (lqrx_dp.hip) and its launchers choose
between, so that a wrong template argument in a launcher shows as a wrong result:

  lane family (B = 65, a full wave and one lane): dp_lane_kernel<T, NP, MP, TV, SOA, LIN, AFF,
    CROSS, VALUE> — every kind × tv × layout × dtype at (n, m) = (2, 1), (4, 3); the other
    (NP, MP) classes (2, 2), (4, 1), (4, 2) at the plain and value kinds.  Plain and linear,
    time-invariant, n = 4 fall to dp_quad_kernel<T, MP, SOA, LIN, EX> at this batch; they run once
    more on the lane kernel (LQRX_DP_SMALL=lane, read on every call).
  tile family (B = 2): dp_riccati_kernel<T, NT, MT, WAVES, VAR, FULL> — every kind × tv × dtype on
    the padded grids (5, 1), (17, 1), (17, 17), (33, 17) and the exact ones (16, 16), (32, 16),
    (32, 32), (64, 32); (64, 16) and (48, 16) at plain and linear (fp64: dp_wg4_kernel<…, 1, …>,
    and the one-wave 4×2 grid); layout 1, which is staged on this family, once per kind at (17, 1).
  big family (B = 2): dp_big_kernel<T> at (65, 4) — every kind × tv in fp64, plain and value in fp32.

The leaves behind a switch the library reads once per process (LQRX_DP_WG4=0, LQRX_DP_BIG=1) and
LQRX_DP_SMALL=hex stay with the tests that start a child process or already select them.

References: plain oracle.dp_solve_abi, linear oracle.dp_solve_lin_abi, the other kinds
tests/dp_truth.py (float64), computed once per problem; the value kind also through value_errors.
Problems: dp_truth.cross_problem, seed 9000 + 37·n + m (+ 1 time-varying); each kind takes the
fields it has.  Tolerances are the project's, with the error measures of dp_truth.check: fp64 1e-10,
fp32 1e-4.
The fp32 bound: the checker (value kind) run in float32 against float64 on the CPU at every
(shape, tv) below, on the same error measures, is worst at 3.1e-6 (p at (2, 1), time-invariant; K
2.4e-6 at (65, 4), d 2.5e-6 at (4, 2), P, X, U below 2.0e-6, s, dV, J below 8.8e-7), so 1e-4 leaves
the kernels more than a decade at every shape.  ((2, 2) time-invariant has a seed of its own for
that: see seed_of.)
"""
import numpy as np
import pytest

from dp_truth import (check, cross_problem, dp_solve_abi_np, logical, relerr_per_knot, to_batch,
                      value_errors)

pytestmark = pytest.mark.gpu

TOL = {0: 1e-10, 1: 1e-4}
N = 3
FIELDS = {"plain": (), "linear": ("q", "r", "qf"), "affine": ("q", "r", "qf", "c"),
          "cross": ("q", "r", "qf", "c", "M"), "value": ("q", "r", "qf", "c", "M")}
KINDS = tuple(FIELDS)
ENDS = ("plain", "value")
LOW = ("plain", "linear")


def cases():
    """(n, m, bt, kind, tv, layout, dtype, small)"""
    out = []
    for n, m, kinds in [(2, 1, KINDS), (4, 3, KINDS), (2, 2, ENDS), (4, 1, ENDS), (4, 2, ENDS)]:
        for kind in kinds:
            for tv in (False, True):
                for layout in (0, 1):
                    for dtype in (0, 1):
                        out.append((n, m, 65, kind, tv, layout, dtype, None))
                        if kind in LOW and n >= 3 and not tv:      # fell to the quad kernel: the lane one too
                            out.append((n, m, 65, kind, tv, layout, dtype, "lane"))
    tiles = [(5, 1), (17, 1), (17, 17), (33, 17), (16, 16), (32, 16), (32, 32), (64, 32)]
    for n, m, kinds in [(n, m, KINDS) for n, m in tiles] + [(64, 16, LOW), (48, 16, LOW)]:
        out += [(n, m, 2, kind, tv, 0, dtype, None) for kind in kinds for tv in (False, True) for dtype in (0, 1)]
    out += [(17, 1, 2, kind, False, 1, 0, None) for kind in KINDS]
    out += [(65, 4, 2, kind, tv, 0, 0, None) for kind in KINDS for tv in (False, True)]
    out += [(65, 4, 2, kind, tv, 0, 1, None) for kind in ENDS for tv in (False, True)]
    return out


CASES = cases()
_refs = {}


def seed_of(n, m, tv):
    # (2, 2) time-invariant: seed 9076 left the fp32 bound less than a decade (p at 1.2e-5 in the
    # float32 checker run), so that shape has a seed of its own
    return 9501 if (n, m, tv) == (2, 2, False) else 9000 + 37 * n + m + int(tv)


def reference(lqrx, oracle, n, m, bt, tv, kind):
    """(problem, float64 reference of `kind`), each computed once and shared between the cases"""
    key = (n, m, bt, tv)
    if key not in _refs:
        _refs[key] = dict(d=cross_problem(lqrx, n, m, N, bt, seed_of(n, m, tv), tv, tv))
    r = _refs[key]
    if kind not in r:
        d = r["d"]
        r[kind] = (oracle.dp_solve_abi(d, N, all_P=True) if kind == "plain" else
                   oracle.dp_solve_lin_abi(d, N, all_P=True) if kind == "linear" else
                   dp_solve_abi_np(d, N, kind, all_P=True))
    return r["d"], r[kind]


@pytest.mark.parametrize("n,m,bt,kind,tv,layout,dtype,small", CASES,
                         ids=[f"n{n}-m{m}-{kind}-tv{int(tv)}-l{layout}-f{64 >> dtype}" + (f"-{small}" if small else "")
                              for n, m, bt, kind, tv, layout, dtype, small in CASES])
def test_dispatch_leaf(lqrx, oracle, gpu_ok, monkeypatch, n, m, bt, kind, tv, layout, dtype, small):
    from lqrx.dp import from_abi

    if small:
        monkeypatch.setenv("LQRX_DP_SMALL", small)
    else:
        monkeypatch.delenv("LQRX_DP_SMALL", raising=False)
    d, ref = reference(lqrx, oracle, n, m, bt, tv, kind)
    got = lqrx.solve_batch(to_batch(d, N, fields=FIELDS[kind]), dtype=dtype, all_P=True, layout=layout,
                           value=kind == "value")
    assert got["rc"] == 0
    tol, what = TOL[dtype], f"{kind} n={n} m={m} tv={int(tv)} layout={layout} f{64 >> dtype} {small or ''}"
    if kind == "plain":
        assert "d" not in got
        K, P = from_abi(ref["K"], (bt, N - 1, m, n)), from_abi(ref["P"], (bt, N, n, n))
        X, U = ref["X"].reshape(bt, N, n), ref["U"].reshape(bt, N - 1, m)
        e = dict(K=relerr_per_knot(got["K"], K), P=relerr_per_knot(got["P"], P),
                 X=float(np.abs(got["X"] - X).max() / max(1.0, np.abs(X).max())),
                 U=float(np.abs(got["U"] - U).max() / max(1.0, np.abs(U).max())))
        print(what, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert (got["info"] == 0).all() and (ref["info"] == 0).all()
        for k, v in e.items():
            assert v <= tol, (k, v)
        return
    check(got, logical(ref, n, m, N, bt, True), True, tol, what)
    if kind == "value":
        e = value_errors(got, ref)
        print(what, " ".join(f"{k} {v.max():.2e}" for k, v in e.items()))
        for k, v in e.items():
            assert v.max() <= tol, (k, v)
