"""GPU checks of the Riccati knot's non-arithmetic paths (lqrx_dp.hip dp_riccati_kernel):

  * the symmetrize that reads its diagonal tiles at (max(row, col), min(row, col)) of the LDS
    image — every stored P_k must be EXACTLY symmetric, on every tile grid the kernel has;
  * Q + AᵀPA issued in chunks beside the Newton–Schulz chain (PnShadow) — parity against the
    C oracle on the same runs, per knot, at the project's tolerances (1e-10 fp64, 1e-4 fp32);
  * the exact-sweep path with the whole of Q + AᵀPA issued ahead of it (LQRX_DP_NS_OFF=1, the
    library's switch, read once per process: one child process);
  * potrf's verdict: a non-SPD R gives the oracle's `info` knot.

Shapes: N = 6, batch = 3 — knot N−1 takes the exact sweep, knot N−2 the first warm start, the
rest extrapolated warm starts (one or more Newton–Schulz rounds), so every path through the
iteration and the remainder of the chunks runs; the grids are one per tile count (and one
padded), the smallest of each.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from dp_truth import relerr_per_knot

pytestmark = pytest.mark.gpu

TOL = {0: 1e-10, 1: 1e-4}
N, BT = 6, 3
# (n, m, dtype): fp64 NT=1 | NT=2 (the headline grid) | padded NT=2 | NT=3 ; fp32 NT=4
GRIDS = [(16, 16, 0), (32, 16, 0), (17, 3, 0), (48, 16, 0), (64, 32, 1)]
_cache = {}


def _run(lqrx, oracle, n, m, dtype):
    """One GPU run and one oracle run per grid, shared by the tests below (never modified)."""
    key = (n, m, dtype)
    if key not in _cache:
        from lqrx.dp import abi_to_batch, from_abi

        d = lqrx.random_batch(n, m, N, BT, seed=700 + 3 * n + m)
        got = lqrx.solve_batch(abi_to_batch(d), dtype=dtype, all_P=True)
        ref = oracle.dp_solve_abi(d, N, all_P=True)
        _cache[key] = (got, dict(K=from_abi(ref["K"], (BT, N - 1, m, n)), P=from_abi(ref["P"], (BT, N, n, n)),
                                 info=ref["info"]))
    return _cache[key]


@pytest.mark.parametrize("n,m,dtype", GRIDS)
def test_stored_P_exactly_symmetric(lqrx, oracle, gpu_ok, n, m, dtype):
    got, _ = _run(lqrx, oracle, n, m, dtype)
    P = got["P"]
    assert P.shape == (BT, N, n, n)
    bad = [(b, k) for b in range(BT) for k in range(N) if not np.array_equal(P[b, k], P[b, k].T)]
    assert not bad, f"P_k not bitwise symmetric at (trajectory, knot index) {bad[:6]}"


@pytest.mark.parametrize("n,m,dtype", GRIDS)
def test_parity_per_knot(lqrx, oracle, gpu_ok, n, m, dtype):
    got, ref = _run(lqrx, oracle, n, m, dtype)
    ek, ep = relerr_per_knot(got["K"], ref["K"]), relerr_per_knot(got["P"], ref["P"])
    print(f"n={n} m={m} dtype={dtype}: K {ek:.3e}  P {ep:.3e}")
    assert got["rc"] == 0 and (got["info"] == 0).all()
    assert ek <= TOL[dtype] and ep <= TOL[dtype]


_SWEEP = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import lqrx
from oracle import oracle as orc
from lqrx.dp import abi_to_batch, from_abi
n, m, N, bt = 32, 16, 6, 3
d = lqrx.random_batch(n, m, N, bt, seed=812)
got = lqrx.solve_batch(abi_to_batch(d), all_P=True)
ref = orc.dp_solve_abi(d, N, all_P=True)
K = from_abi(ref["K"], (bt, N - 1, m, n)); P = from_abi(ref["P"], (bt, N, n, n))
def rel(a, b):
    a = a.reshape(bt, a.shape[1], -1); b = b.reshape(bt, b.shape[1], -1)
    return float((np.abs(a - b).max(axis=2) / np.abs(b).max(axis=2)).max())
ek, ep = rel(got["K"], K), rel(got["P"], P)
sym = all(np.array_equal(got["P"][b, k], got["P"][b, k].T) for b in range(bt) for k in range(N))
print("K", ek, "P", ep, "symmetric", sym)
sys.exit(0 if (got["rc"] == 0 and (got["info"] == 0).all() and sym and max(ek, ep) <= 1e-10) else 1)
"""


def test_exact_sweep_path_parity(lqrx, gpu_ok):
    """ns_off: every knot takes the exact LDLᵀ sweep, with all of Q + AᵀPA issued before it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LQRX_DP_NS_OFF="1",
               PYTHONPATH=os.pathsep.join([os.path.join(root, "lqr.jl_amd"), root, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _SWEEP, root], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_non_spd_info_matches_oracle(lqrx, oracle, gpu_ok):
    """A non-SPD R on one trajectory (injected as tests/test_dp_gpu.py does): the kernel's `info`
    is the oracle's — the first backward knot, N − 1, for that trajectory and 0 for the rest."""
    from lqrx.dp import abi_to_batch, to_abi

    n, m = 32, 16
    d = lqrx.random_batch(n, m, N, BT, seed=31)
    b = abi_to_batch(d)
    b.R[1] = -100.0 * np.eye(m)
    b.B[1] *= 1e-3
    got = lqrx.solve_batch(b)
    d2 = dict(d, R=to_abi(b.R), B=to_abi(b.B))
    ref = oracle.dp_solve_abi(d2, N)
    assert got["rc"] == 1
    assert np.array_equal(np.asarray(got["info"]).ravel(), np.asarray(ref["info"]).ravel()), (got["info"], ref["info"])
    assert got["info"][1] == N - 1
