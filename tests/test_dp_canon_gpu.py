"""GPU checks of the canonical-coordinates Riccati solve (lqrx_dp_canon.hip, dp_riccati_kernel's
VAR_CANON and VAR_MASK): fp64, n = 32, m = 16, plain, time-invariant, P_1 only — the one
grid the change enables (every other grid dispatches as before, so there is no further grid to run).

Every case is solved twice: in this process (canonical path on) and once in a child process with
LQRX_DP_CANON=0 (the library reads the switch once per process), which dumps the generic kernel's
results of all cases into one file.  Against those and the C oracle:

  * N = 2 (only the exact first knot), 3, 40 at batch 5: K per knot, P_1, X, U within 1e-10 of the
    oracle, within 1e-11 of the generic run, P_1 bitwise symmetric, info all zero;
  * cond(B) = 1e6 and 1e12, under the conditioning bound, at N = 40: within 1e-10 of the oracle;
  * a mixed batch of 6 with two trajectories the set-up excludes (a zero column in B; cond(B) = 1e15,
    past the bound): those two bit-identical to the generic run, the others within 1e-10 of the oracle;
  * a non-SPD R on one trajectory: the generic path's info knot, the neighbours unaffected;
  * a p_mode 1 call and a call with linear terms on the same data: bit-identical to the generic run
    (they never take the new path);
  * one captured-graph replay equals the eager call bitwise;
  * one guard-zone run: no write outside the buffers, same bits as on plain tensors, and the call
    allocates nothing through the caller's allocator (the workspace is the library pool's).
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


def _batch(lqrx, N, bt, seed):
    from lqrx.dp import abi_to_batch

    return abi_to_batch(lqrx.random_batch(n, m, N, bt, seed=seed))


def _with_cond(B, cond):
    u, s, vt = np.linalg.svd(B, full_matrices=False)
    return (u * (s[0] * cond ** (-np.arange(s.size) / (s.size - 1.0)))) @ vt


def cases(lqrx):
    """name → (LQRBatch, solve_batch keyword arguments)"""
    from dataclasses import replace

    c = {f"N{N}": (_batch(lqrx, N, 5, 900 + N), {}) for N in (2, 3, 40)}
    b = _batch(lqrx, 12, 6, 77)
    B = b.B.copy()
    B[1][:, 3] = 0.0                               # rank-deficient
    B[4] = _with_cond(B[4], 1e15)                  # κ∞(B₁) past the bound
    c["mixed"] = (replace(b, B=B), {})
    for e in (6, 12):                              # ill-conditioned B under the bound: the canonical path
        b = _batch(lqrx, 40, 3, 60 + e)
        c[f"cond{e}"] = (replace(b, B=np.stack([_with_cond(x, 10.0 ** e) for x in b.B])), {})
    b = _batch(lqrx, 6, 3, 31)
    R, B = b.R.copy(), b.B.copy()
    R[1] = -100.0 * np.eye(m)
    B[1] *= 1e-3
    c["nonspd"] = (replace(b, R=R, B=B), {})
    b = c["N3"][0]
    c["pmode1"] = (b, dict(all_P=True))
    rng = np.random.default_rng(5)
    c["linear"] = (replace(b, q=rng.standard_normal((5, n)), r=rng.standard_normal((5, m)),
                           qf=rng.standard_normal((5, n))), {})
    return c


def solve_all(lqrx):
    return {k: lqrx.solve_batch(b, **kw) for k, (b, kw) in cases(lqrx).items()}


if __name__ == "__main__":          # the child: every case on the generic path, dumped to argv[1]
    assert os.environ.get("LQRX_DP_CANON") == "0"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "lqr.jl_amd"), root]
    import lqrx as L

    L.load()
    np.savez(sys.argv[1], **{f"{c}/{k}": np.asarray(v) for c, o in solve_all(L).items() for k, v in o.items()})
    sys.exit(0)


_runs = {}


@pytest.fixture(scope="module")
def runs(lqrx, gpu_ok, tmp_path_factory):
    """(canonical-path results, generic-path results, cases), computed once and never modified."""
    if not _runs:
        path = str(tmp_path_factory.mktemp("canon") / "generic.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, LQRX_DP_CANON="0"),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        z = np.load(path)
        cs = cases(lqrx)
        gen = {c: {k.split("/")[1]: z[k] for k in z.files if k.startswith(c + "/")} for c in cs}
        _runs.update(canon=solve_all(lqrx), generic=gen, cases=cs)
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
    got, gen, b = runs["canon"][c], runs["generic"][c], runs["cases"][c][0]
    eo, eg = _err(got, _oracle(oracle, b), range(5)), _err(got, gen, range(5))
    print(f"N={N}: vs oracle", " ".join(f"{k} {v:.2e}" for k, v in eo.items()),
          "| vs generic", " ".join(f"{k} {v:.2e}" for k, v in eg.items()))
    assert got["rc"] == 0 and (got["info"] == 0).all()
    assert got["P"].shape == (5, n, n) and all(np.array_equal(P, P.T) for P in got["P"])
    assert max(eo.values()) <= TOL_ORACLE, eo
    assert max(eg.values()) <= TOL_GENERIC, eg
    # the canonical kernel did run: a different recursion does not give the generic kernel's bits
    assert not _same_bits(got["K"], gen["K"])


@pytest.mark.parametrize("e", [6, 12])
def test_parity_ill_conditioned_B(runs, oracle, e):
    """cond(B) = 1e6 and 1e12 (κ∞(B₁) ≈ 1.5 cond(B), under the 2.5e13 bound): the set-up's own
    reflectors and back substitution with entries of S up to ~1e12, the canonical kernel on them."""
    c = f"cond{e}"
    got, gen, b = runs["canon"][c], runs["generic"][c], runs["cases"][c][0]
    eo, eg = _err(got, _oracle(oracle, b), range(3)), _err(got, gen, range(3))
    print(f"cond(B)=1e{e}: vs oracle", " ".join(f"{k} {v:.2e}" for k, v in eo.items()),
          "| vs generic", " ".join(f"{k} {v:.2e}" for k, v in eg.items()))
    assert got["rc"] == 0 and (got["info"] == 0).all()
    assert all(np.array_equal(P, P.T) for P in got["P"])
    assert max(eo.values()) <= TOL_ORACLE, eo
    assert not _same_bits(got["K"], gen["K"])          # the canonical kernel did take them


def test_mixed_batch(runs, oracle):
    got, gen, b = runs["canon"]["mixed"], runs["generic"]["mixed"], runs["cases"]["mixed"][0]
    excluded, rest = (1, 4), (0, 2, 3, 5)
    for k in OUT:
        assert _same_bits(got[k][list(excluded)], gen[k][list(excluded)]), k
    eo = _err(got, _oracle(oracle, b), rest)
    print("mixed: vs oracle", " ".join(f"{k} {v:.2e}" for k, v in eo.items()))
    assert (got["info"] == 0).all() and (gen["info"] == 0).all()
    assert max(eo.values()) <= TOL_ORACLE, eo
    assert not _same_bits(got["K"][list(rest)], gen["K"][list(rest)])


def test_non_spd_info(runs, oracle):
    got, gen, b = runs["canon"]["nonspd"], runs["generic"]["nonspd"], runs["cases"]["nonspd"][0]
    assert got["rc"] == 1 and np.array_equal(got["info"], gen["info"]), (got["info"], gen["info"])
    assert list(got["info"]) == [0, b.N - 1, 0]
    eo = _err(got, _oracle(oracle, b), (0, 2))
    assert max(eo.values()) <= TOL_ORACLE, eo


@pytest.mark.parametrize("case", ["pmode1", "linear"])
def test_other_calls_keep_their_path(runs, case):
    got, gen = runs["canon"][case], runs["generic"][case]
    for k in [k for k in got if k != "rc"]:
        assert _same_bits(got[k], gen[k]), (case, k)


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
    t, second = _device_problem(lqrx, N, bt, 21), _device_problem(lqrx, N, bt, 22)
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

    N, bt = 5, 3
    t = _device_problem(lqrx, N, bt, 23)
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
