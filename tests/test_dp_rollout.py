"""CPU tests of the scenario rollout (lqrx_dp_rollout, include/lqrx.h): the numpy checker
tests/dp_rollout_truth.py pinned against tests/dp_truth.py with no library compute, the clamp inputs
of the GPU tests, and the argument codes of both entries, which are decided without a device.
"""
import ctypes as C

import numpy as np
import pytest

from dp_rollout_truth import (check_clamp_condition, clamp_bounds, cross_problem, j_error, rollout_np,
                              scenarios, xu_error)
from dp_truth import cost_of, dp_solve_abi_np

# (n, m, N, batch, tv)
SHAPES = [(1, 1, 6, 3, False), (4, 1, 40, 4, False), (6, 3, 30, 3, True), (17, 5, 12, 2, True)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
# the shapes of the GPU clamp test (tests/test_dp_rollout_gpu.py)
CLAMP_SHAPES = [(4, 1, 40, 8, False), (6, 3, 30, 7, False), (32, 16, 40, 4, False), (64, 32, 12, 2, False),
                (65, 4, 8, 2, False)]


def solved(lqrx, shape, seed=5):
    n, m, N, bt, tv = shape
    d = cross_problem(lqrx, n, m, N, bt, seed, tv_QR=tv, tv_AB=tv)
    return d, dp_solve_abi_np(d, N, "value")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_checker_reproduces_the_solve_rollout(lqrx, shape):
    """S = 1, α = 1, no w, no bounds on the solve's own K, d and x0: the solve checker's X and U to
    1e-12, J = cost_of, and J = the value checker's J to 1e-10 of its scale."""
    n, m, N, bt, tv = shape
    d, ref = solved(lqrx, shape)
    cross = dp_solve_abi_np(d, N, "cross")
    got = rollout_np(d, N, cross["K"], cross["d"], d["x0"].reshape(bt, 1, n))
    eX = xu_error(got["X"][:, 0], cross["X"].reshape(bt, N, n))
    eU = xu_error(got["U"][:, 0], cross["U"].reshape(bt, N - 1, m))
    Jc = cost_of(d, got["X"][:, 0], got["U"][:, 0])
    eJc = float((np.abs(got["J"][:, 0] - Jc) / np.maximum(1, got["T"][:, 0])).max())
    eJv = float((np.abs(got["J"][:, 0] - ref["J"]) / np.maximum(1, ref["S"] + np.abs(ref["J"]))).max())
    print(f"rollout checker {shape}: X {eX:.2e} U {eU:.2e} J vs cost_of {eJc:.2e} J vs value {eJv:.2e}")
    assert eX <= 1e-12 and eU <= 1e-12
    assert eJc <= 1e-12 and eJv <= 1e-10


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_checker_step_length_identity(lqrx, shape):
    """J(α) = J(1) + ½(1 − α)² dV for α ∈ {0, ½, 1}: completion of squares around the optimal policy,
    exact for affine problems."""
    n, m, N, bt, tv = shape
    d, ref = solved(lqrx, shape)
    al = np.array([0.0, 0.5, 1.0])
    x0 = np.repeat(d["x0"].reshape(bt, 1, n), 3, axis=1)
    got = rollout_np(d, N, ref["K"], ref["d"], x0, alpha=np.tile(al, (bt, 1)))
    want = got["J"][:, 2:3] + 0.5 * (1 - al) ** 2 * ref["dV"][:, None]
    e = float((np.abs(got["J"] - want) / np.maximum(1, got["T"])).max())
    print(f"rollout checker {shape}: three-α identity {e:.2e}")
    assert e <= 1e-10


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_checker_superposition(lqrx, shape):
    """X(x0, w) − X(x0, 0) is the rollout of the homogeneous closed loop (c = 0, d = 0) from 0 driven by w."""
    n, m, N, bt, tv = shape
    d, ref = solved(lqrx, shape)
    sc = scenarios(n, m, N, bt, 3, seed=9)
    full = rollout_np(d, N, ref["K"], ref["d"], sc["x0"], alpha=sc["alpha"], w=sc["w"])
    free = rollout_np(d, N, ref["K"], ref["d"], sc["x0"], alpha=sc["alpha"])
    hom = rollout_np(dict(d, c=None), N, ref["K"], None, np.zeros_like(sc["x0"]), w=sc["w"])
    e = xu_error(full["X"] - free["X"], hom["X"])
    print(f"rollout checker {shape}: superposition {e:.2e}")
    assert e <= 1e-12


@pytest.mark.parametrize("shape", CLAMP_SHAPES, ids=["x".join(map(str, s)) for s in CLAMP_SHAPES])
def test_clamp_inputs_saturate_and_stay_inside(lqrx, shape):
    """The clamp inputs of the GPU test: ±(0.9 quantile of |u| per control row of the unclamped
    rollout) leaves at least 5 % of U exactly at a bound and at least 5 % strictly inside."""
    n, m, N, bt, tv = shape
    d, ref = solved(lqrx, shape)
    sc = scenarios(n, m, N, bt, 21, seed=9)
    free = rollout_np(d, N, ref["K"], ref["d"], sc["x0"], alpha=sc["alpha"], w=sc["w"])
    lo, hi = clamp_bounds(free["U"])
    got = rollout_np(d, N, ref["K"], ref["d"], sc["x0"], alpha=sc["alpha"], w=sc["w"], u_lo=lo, u_hi=hi)
    assert np.isfinite(got["X"]).all() and np.isfinite(got["J"]).all()
    check_clamp_condition(got["U"], lo, hi, f"{shape}")


# ---- argument codes: decided before the device is touched ----
def _call(lqrx, host, desc, A, B, c, K, d, cost, sc):
    from lqrx import _lib

    lib = lqrx.load()
    vp = lambda x: None if x is None else C.c_void_p(x)
    args = [C.byref(desc) if desc is not None else None, vp(A), vp(B), vp(c), vp(K), vp(d),
            C.byref(cost) if cost is not None else None, C.byref(sc) if sc is not None else None]
    rc = lib.lqrx_dp_rollout_host(*args) if host else lib.lqrx_dp_rollout(*args, None)
    return rc, lib.lqrx_last_error().decode()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_rollout_argument_codes(lqrx, host):
    from lqrx import _lib

    buf = np.zeros(4096)
    p = buf.ctypes.data
    desc = lambda **kw: _lib.DpDesc(**{**dict(n=8, m=4, N=10, dtype=_lib.F64, batch=4, layout=0, p_mode=0,
                                              knot_stride_AB=0, knot_stride_QR=0), **kw})
    cost = lambda **kw: _lib.DpCost(**{**{k: p for k in ("Q", "R", "Qf", "M", "q", "r", "qf")}, **kw})
    scen = lambda **kw: _lib.DpScenarios(**{**dict(S=5, x0=p, alpha=p, w=p, u_lo=p, u_hi=p, X=p, U=p, J=p), **kw})
    call = lambda **kw: _call(lqrx, host, **{**dict(desc=desc(), A=p, B=p, c=p, K=p, d=p, cost=cost(), sc=scen()), **kw})

    for name, code in (("A", -2), ("B", -3), ("K", -5), ("cost", -7), ("sc", -8)):
        rc, msg = call(**{name: None})
        assert rc == code and name in msg, (name, rc, msg)
    assert call(desc=None)[0] == -1
    assert call(desc=desc(n=0))[0] == -1
    assert call(desc=desc(N=1))[0] == -1
    assert call(desc=desc(dtype=7))[0] == -1
    assert call(desc=desc(n=513))[0] == _lib.ERR_UNSUPPORTED
    assert call(desc=desc(layout=1))[0] == _lib.ERR_UNSUPPORTED
    assert call(desc=desc(p_mode=9), A=None)[0] == -2            # p_mode is ignored
    for member in ("Q", "R", "Qf"):
        rc, msg = call(cost=cost(**{member: None}))
        assert rc == -7 and "cost->" + member in msg, (member, rc, msg)
    for kw, text in ((dict(S=0), "sc->S"), (dict(S=-2), "sc->S"), (dict(x0=None), "sc->x0"),
                     (dict(X=None, U=None, J=None), "sc->X")):
        rc, msg = call(sc=scen(**kw))
        assert rc == -8 and text in msg, (kw, rc, msg)
    # without J the cost is not needed: a NULL cost passes the checks, and what answers is the next one
    assert call(cost=None, sc=scen(J=None, x0=None))[0] == -8
    assert call(cost=cost(Qf=None), sc=scen(J=None, S=0))[0] == -8
    # an empty batch is a no-op whatever the pointers
    assert call(desc=desc(batch=0), A=None, B=None, c=None, K=None, d=None, cost=None, sc=None)[0] == 0


def test_rollout_symbols_and_mirrors(lqrx):
    """The entries are additive to ABI 5 (detect by symbol) and stay out of the solve-entry table."""
    from lqrx import _lib

    lib = lqrx.load()
    assert lib.lqrx_abi_version() == 5
    assert hasattr(lib, "lqrx_dp_rollout") and hasattr(lib, "lqrx_dp_rollout_host")
    assert not any("rollout" in k for k in _lib.DP_ENTRY_ARGS)
    assert C.sizeof(_lib.DpCost) == 7 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.DpScenarios) == 8 + 8 * C.sizeof(C.c_void_p)
    assert callable(lqrx.rollout_batch) and callable(lqrx.dp_rollout_device)
