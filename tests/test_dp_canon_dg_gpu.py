"""GPU checks of the diagonal-A₂₁ tier of the canonical Riccati solve (dp_riccati_kernel's VAR_DIAG in
lqrx_dp_diag.hip, the set-up's flag 3 and its Jacobi in lqrx_dp_canon.hip): fp64, n = 32,
m = 16, plain, time-invariant, P_1 only.

Every case is solved three times: in this process (all four tiers on) and in two child processes —
LQRX_DP_CANON=0, the generic kernel, and LQRX_DP_DIAG=0, the parent's three tiers (the library reads
either switch once per process) — each dumping all cases into one file.  Against those and the C oracle:

  * N = 2 (only the exact first knot), 3, 40 at batch 5: K per knot, P_1, X, U within 1e-10 of the
    oracle and within 1e-11 of the generic run, P_1 bitwise symmetric, info zero, and K not the
    LQRX_DP_DIAG=0 run's bits — the new tier ran;
  * a mixed batch of 6 with all four tiers — B as generated, κ∞(B₁) = 300 (between the two bounds),
    cond(B) = 1e6, a zero column: tiers 2, 1 and 0 bit-identical to the LQRX_DP_DIAG=0 run, tier 3 within
    1e-10 of the oracle and not its bits;
  * a trajectory at κ∞(B₁) just under DP_DIAG_KAPPA_F64 (0.97 of it by the model's QR): tier 3, within
    1e-10 of the oracle;
  * degenerate A₂₁, set into A = T·Ã·Tᵀ with the model's T — exactly zero, rank 3, 0.1 × an orthogonal
    matrix (all σ equal), σ spread over 1e6: the run returns (the Jacobi's loops are counted) and every
    trajectory is within 1e-10 of the oracle, whichever tier took it;
  * a non-SPD R on one trajectory: the generic run's info knot, the neighbours unaffected;
  * a p_mode 1 call and a call with linear terms: bit-identical to the LQRX_DP_DIAG=0 run;
  * one captured-graph replay equals the eager call bitwise;
  * one guard-zone run: no write outside the buffers, same bits as on plain tensors, nothing
    allocated through the caller's allocator.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

n, m = 32, 16
TOL_ORACLE, TOL_GENERIC = 1e-10, 1e-11
OUT = ("K", "P", "X", "U", "info")
EDGE = 0.97          # the edge case's κ∞(B₁) as a fraction of the bound
DEGENERATE = ("zero", "rank3", "equal", "spread")


def _batch(lqrx, N, bt, seed):
    from lqrx.dp import abi_to_batch

    return abi_to_batch(lqrx.random_batch(n, m, N, bt, seed=seed))


def _with_cond(B, cond):
    u, s, vt = np.linalg.svd(B, full_matrices=False)
    return (u * (s[0] * cond ** (-np.arange(s.size) / (s.size - 1.0)))) @ vt


def _kappa(B):
    """κ∞(B₁) of one B by the model's QR (tests/dp_canon_truth.py canon_setup's formula)"""
    r = np.triu(np.linalg.qr(B, mode="complete")[1][:m])
    return np.abs(r).sum(axis=1).max() * np.abs(np.linalg.inv(r)).sum(axis=1).max()


def _at_kappa(B, target):
    """B with its singular values respaced so that κ∞(B₁) = target to 1e-6 (bisection on cond(B))"""
    lo, hi = 1.0, 1e4
    for _ in range(60):
        mid = np.sqrt(lo * hi)
        lo, hi = (mid, hi) if _kappa(_with_cond(B, mid)) < target else (lo, mid)
    return _with_cond(B, lo)


def _bound():
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "lqr.jl_amd", "csrc", "lqrx_internal.h")).read()
    return float(re.search(r"DP_DIAG_KAPPA_F64\s*=\s*([0-9.e+-]+);", src).group(1))


def _with_a21(A, B, block):
    """A with the lower-left block of TᵀAT replaced by `block`, T the model's (numpy's QR of B)"""
    T = np.linalg.qr(B, mode="complete")[0]
    At = T.T @ A @ T
    At[m:, :m] = block
    return T @ At @ T.T


def _degenerate_blocks():
    rng = np.random.default_rng(16)
    q1, q2 = (np.linalg.qr(rng.standard_normal((m, m)))[0] for _ in range(2))
    return dict(zero=np.zeros((m, m)), rank3=0.02 * rng.standard_normal((m, 3)) @ rng.standard_normal((3, m)),
                equal=0.1 * q1, spread=(q1 * 10.0 ** (-6 * np.arange(m) / (m - 1.0))) @ q2.T)


def cases(lqrx):
    """name → (LQRBatch, solve_batch keyword arguments)"""
    from dataclasses import replace

    c = {f"N{N}": (_batch(lqrx, N, 5, 900 + N), {}) for N in (2, 3, 40)}
    b = _batch(lqrx, 12, 6, 91)
    B = b.B.copy()
    B[1][:, 3] = 0.0                               # rank-deficient: tier 0
    B[2] = _with_cond(B[2], 1e6)                   # past the pre-feedback bound: tier 1
    B[4] = _at_kappa(B[4], 300.0)                  # between the two bounds: tier 2
    B[5] = _at_kappa(B[5], 300.0)
    c["mixed"] = (replace(b, B=B), {})
    b = _batch(lqrx, 40, 4, 92)
    B = b.B.copy()
    B[2] = _at_kappa(B[2], EDGE * _bound())
    c["edge"] = (replace(b, B=B), {})
    b = _batch(lqrx, 40, 5, 93)
    A = b.A.copy()
    for t, blk in enumerate(_degenerate_blocks().values()):
        A[t] = _with_a21(A[t], b.B[t], blk)        # trajectory 4 stays as generated
    c["degenerate"] = (replace(b, A=A), {})
    b = _batch(lqrx, 6, 4, 32)
    R, B = b.R.copy(), b.B.copy()
    R[1] = -100.0 * np.eye(m)
    B[1] *= 1e-3
    c["nonspd"] = (replace(b, R=R, B=B), {})
    b = c["N3"][0]
    c["pmode1"] = (b, dict(all_P=True))
    rng = np.random.default_rng(6)
    c["linear"] = (replace(b, q=rng.standard_normal((5, n)), r=rng.standard_normal((5, m)),
                           qf=rng.standard_normal((5, n))), {})
    return c


def solve_all(lqrx):
    return {k: lqrx.solve_batch(b, **kw) for k, (b, kw) in cases(lqrx).items()}


if __name__ == "__main__":          # a child: every case under the switch of its environment, dumped to argv[1]
    assert "0" in (os.environ.get("LQRX_DP_CANON"), os.environ.get("LQRX_DP_DIAG"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "lqr.jl_amd"), root]
    import lqrx as L

    L.load()
    np.savez(sys.argv[1], **{f"{c}/{k}": np.asarray(v) for c, o in solve_all(L).items() for k, v in o.items()})
    sys.exit(0)


_runs = {}


@pytest.fixture(scope="module")
def runs(lqrx, gpu_ok, tmp_path_factory):
    """(four-tier results, LQRX_DP_DIAG=0 results, LQRX_DP_CANON=0 results, cases), computed once and
    never modified."""
    if not _runs:
        cs = cases(lqrx)
        d = tmp_path_factory.mktemp("diag")
        for name, var in (("prefb", "LQRX_DP_DIAG"), ("generic", "LQRX_DP_CANON")):
            path = str(d / f"{name}.npz")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, **{var: "0"}),
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            z = np.load(path)
            _runs[name] = {c: {k.split("/")[1]: z[k] for k in z.files if k.startswith(c + "/")} for c in cs}
        _runs.update(diag=solve_all(lqrx), cases=cs)
    return _runs


def _oracle(oracle, b):
    from lqrx.dp import from_abi, to_abi

    bt, N = b.batch, b.N
    d = dict({k: to_abi(np.asarray(getattr(b, k), np.float64)).reshape(-1) for k in ("A", "B", "Q", "R", "Qf")},
             x0=np.ascontiguousarray(b.x0, np.float64).reshape(-1), n=n, m=m, N=N, batch=bt)
    ref = oracle.dp_solve_abi(d, N)
    return dict(K=from_abi(ref["K"], (bt, N - 1, m, n)), P=from_abi(ref["P"], (bt, n, n)),
                X=ref["X"].reshape(bt, N, n), U=ref["U"].reshape(bt, N - 1, m), info=ref["info"])


def _err(got, ref, rows):
    """worst relative error over the trajectories `rows`: K per knot, P_1, X and U per trajectory"""
    from dp_truth import relerr_per_knot, relerr_traj

    r = list(rows)
    return dict(K=relerr_per_knot(got["K"][r], ref["K"][r]), P=relerr_per_knot(got["P"][r][:, None], ref["P"][r][:, None]),
                X=relerr_traj(got["X"][r], ref["X"][r]), U=relerr_traj(got["U"][r], ref["U"][r]))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N", [2, 3, 40])
def test_parity(runs, oracle, N):
    c = f"N{N}"
    got, gen, pfb, b = runs["diag"][c], runs["generic"][c], runs["prefb"][c], runs["cases"][c][0]
    eo, eg = _err(got, _oracle(oracle, b), range(5)), _err(got, gen, range(5))
    print(f"N={N}: vs oracle", " ".join(f"{k} {v:.2e}" for k, v in eo.items()),
          "| vs generic", " ".join(f"{k} {v:.2e}" for k, v in eg.items()))
    assert got["rc"] == 0 and (got["info"] == 0).all()
    assert got["P"].shape == (5, n, n) and all(np.array_equal(P, P.T) for P in got["P"])
    assert max(eo.values()) <= TOL_ORACLE, eo
    assert max(eg.values()) <= TOL_GENERIC, eg
    # the new tier did run: another recursion does not give the VAR_PREFB kernel's bits, trajectory by trajectory
    assert all(not _same_bits(got["K"][t], pfb["K"][t]) for t in range(5))


def test_mixed_batch(runs, oracle):
    import dp_canon_dg_truth as dg

    got, pfb, b = runs["diag"]["mixed"], runs["prefb"]["mixed"], runs["cases"]["mixed"][0]
    tiers = list(dg.tier(b.A, b.B))
    assert tiers == [3, 0, 1, 3, 2, 2]
    old = [t for t in range(6) if tiers[t] != 3]
    new = [t for t in range(6) if tiers[t] == 3]
    for k in OUT:
        assert _same_bits(got[k][old], pfb[k][old]), k
    eo = _err(got, _oracle(oracle, b), range(6))
    print("mixed: vs oracle", " ".join(f"{k} {v:.2e}" for k, v in eo.items()))
    assert (got["info"] == 0).all() and (pfb["info"] == 0).all()
    assert max(eo.values()) <= TOL_ORACLE, eo
    assert all(not _same_bits(got["K"][t], pfb["K"][t]) for t in new)


def test_just_under_the_bound(runs, oracle):
    import dp_canon_dg_truth as dg

    got, pfb, b = runs["diag"]["edge"], runs["prefb"]["edge"], runs["cases"]["edge"][0]
    kap = _kappa(b.B[2])
    assert abs(kap / (EDGE * _bound()) - 1) <= 1e-3 and list(dg.tier(b.A, b.B)) == [3, 3, 3, 3]
    eo = {t: _err(got, _oracle(oracle, b), (t,)) for t in (2, 0)}
    print(f"κ∞(B₁) = {kap:.4e}: vs oracle", " ".join(f"{k} {v:.2e}" for k, v in eo[2].items()),
          "| neighbour", " ".join(f"{k} {v:.2e}" for k, v in eo[0].items()))
    assert got["rc"] == 0 and (got["info"] == 0).all()
    assert max(eo[2].values()) <= TOL_ORACLE and max(eo[0].values()) <= TOL_ORACLE, eo
    assert not _same_bits(got["K"][2], pfb["K"][2])          # tier 3 did take it


def test_degenerate_a21(runs, oracle):
    got, pfb, b = runs["diag"]["degenerate"], runs["prefb"]["degenerate"], runs["cases"]["degenerate"][0]
    ref = _oracle(oracle, b)
    assert got["rc"] == 0 and (got["info"] == 0).all() and (ref["info"] == 0).all()
    worst = {}
    for t, name in enumerate(DEGENERATE + ("plain",)):
        eo = worst[name] = _err(got, ref, (t,))
        print(f"A₂₁ {name}: vs oracle", " ".join(f"{k} {v:.2e}" for k, v in eo.items()),
              "| the LQRX_DP_DIAG=0 run's bits:", _same_bits(got["K"][t], pfb["K"][t]))
    assert all(max(eo.values()) <= TOL_ORACLE for eo in worst.values()), worst


def test_non_spd_info(runs, oracle):
    got, gen, b = runs["diag"]["nonspd"], runs["generic"]["nonspd"], runs["cases"]["nonspd"][0]
    ref = _oracle(oracle, b)
    assert got["rc"] == 1 and np.array_equal(got["info"], gen["info"]), (got["info"], gen["info"])
    assert list(got["info"]) == [0, b.N - 1, 0, 0] and np.array_equal(got["info"], ref["info"])
    eo = _err(got, ref, (0, 2, 3))
    assert max(eo.values()) <= TOL_ORACLE, eo


@pytest.mark.parametrize("case", ["pmode1", "linear"])
def test_other_calls_keep_their_path(runs, case):
    got, pfb = runs["diag"][case], runs["prefb"][case]
    for k in [k for k in got if k != "rc"]:
        assert _same_bits(got[k], pfb[k]), (case, k)


def _device_problem(lqrx, N, bt, seed):
    import torch

    d = lqrx.random_batch(n, m, N, bt, seed)
    t = {k: torch.from_numpy(d[k]).cuda() for k in ("A", "B", "Q", "R", "Qf", "x0")}
    t.update(n=n, m=m, batch=bt)
    return t


def test_graph_replay(lqrx, gpu_ok):
    import torch
    from lqrx.dp import dp_solve_device

    N, bt = 12, 7
    t, second = _device_problem(lqrx, N, bt, 44), _device_problem(lqrx, N, bt, 45)
    call = lambda s: dp_solve_device(t, N, 0, stream=s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(side.cuda_stream)                       # warm-up: the pool's first block
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(torch.cuda.current_stream().cuda_stream)
    for k in ("A", "B", "Q", "R", "Qf", "x0"):
        t[k].copy_(second[k])
    g.replay()
    torch.cuda.synchronize()
    got = {k: out[k].clone() for k in OUT}
    ref = call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k in OUT:
        assert got[k].equal(ref[k]), k
    assert (ref["info"] == 0).all().item()


def test_guard_zones(lqrx, gpu_ok):
    import torch
    from guarded import check as guard_check, guard_all, pattern_filled
    from lqrx.dp import dp_solve_device

    N, bt = 5, 4
    t = _device_problem(lqrx, N, bt, 46)
    sizes = dict(K=bt * (N - 1) * m * n, P=bt * n * n, X=bt * N * n, U=bt * (N - 1) * m, info=bt)
    like_i = torch.empty(1, dtype=torch.int32, device="cuda:0")
    outs = lambda: {k: pattern_filled(like_i if k == "info" else t["A"], sz) for k, sz in sizes.items()}
    plain = dp_solve_device(t, N, 0, out=outs())
    assert plain["rc"] == 0
    hs = []
    tg, og = guard_all(t, "in", bt, hs), guard_all(outs(), "out", bt, hs)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = dp_solve_device(tg, N, 0, out=og)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before     # the workspace is not the caller's allocator's
    assert got["rc"] == 0
    guard_check(hs)
    for k in sizes:
        a, b_ = got[k], plain[k]
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), k
