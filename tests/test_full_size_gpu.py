"""Full-size GPU parity at BASELINE.json's own configs (VERDICT r1 "next" item 1).

cfg4: n=32 m=16 N=256 B=65536 fp64 (the headline) and cfg5: n=64 m=32 N=512 B=8192 fp32,
each solved in ONE lqrx_dp_solve launch at the full batch on the device, then
  * the whole batch is scanned on the device for non-finite K, P₁, X, U and info ≠ 0;
  * a strided sample of trajectories — always including the last one, whose K offset
    (65535·255·16·32 elements) is past 2³² — is copied back and compared per knot with the
    CPU oracle (oracle/lqr_oracle.c, restating dynamic_programming.jl:54-72) on the same
    inputs.
Tolerances: fp64 1e-10 relative per knot (north star).  fp32 (cfg5) is compared against the
fp64 oracle run on the same fp32-rounded inputs; over 511 knots the measured error is
K 3.0e-5, P 3.8e-6, X 2.0e-5, U 1.9e-5 (MI355X, 48 sampled trajectories, round 2), held
here to TOL32_N512 = 1e-4, the fp32 bar SURVEY §8(d) suggests.  Measured cfg4 (256
samples incl. index 65535): K 2.4e-12, P 2.4e-13, X 1.0e-12, U 1.3e-12.
"""
import os

import numpy as np
import pytest

from dp_truth import relerr_per_knot

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL32_N512 = 1e-4


def sample_index(batch, k):
    """k strided trajectory indices in [0, batch), always including 0 and batch − 1."""
    idx = np.unique(np.linspace(0, batch - 1, k).round().astype(np.int64))
    assert idx[0] == 0 and idx[-1] == batch - 1
    return idx


def traj_err(a, b):
    """max over trajectories of max|a − b| / max(1, max|b|) (the rollout decays towards 0,
    so late knots are compared on the trajectory's scale, as tests/test_dp_gpu.py does)."""
    a = a.reshape(a.shape[0], -1)
    b = b.reshape(b.shape[0], -1)
    return float((np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(b).max(axis=1))).max())


def full_size_case(lqrx, oracle, n, m, N, B, f64, nsample, seed):
    import torch
    from lqrx.dp import from_abi

    dev = torch.device("cuda", 0)
    host = lqrx.random_batch(n, m, N, B, seed=seed, dtype=lqrx.F64 if f64 else lqrx.F32)
    t = {k: torch.from_numpy(host[k]).to(dev) for k in ("A", "B", "Q", "R", "Qf", "x0")}
    t.update(n=n, m=m, batch=B)
    out = lqrx.dp_solve_device(t, N, p_mode=0)
    torch.cuda.synchronize(dev)
    # whole-batch scan on the device
    for k in ("K", "P", "X", "U"):
        assert bool(torch.isfinite(out[k]).all()), f"non-finite {k} in the full batch"
    assert int((out["info"] != 0).sum()) == 0 and out["rc"] == 0

    idx = sample_index(B, nsample)
    ti = torch.from_numpy(idx).to(dev)
    pick = lambda x, w: x.view(B, w).index_select(0, ti).cpu().numpy().astype(np.float64)
    got = dict(K=from_abi(pick(out["K"], (N - 1) * m * n), (len(idx), N - 1, m, n)),
               P=from_abi(pick(out["P"], n * n), (len(idx), n, n)),
               X=pick(out["X"], N * n).reshape(len(idx), N, n),
               U=pick(out["U"], (N - 1) * m).reshape(len(idx), N - 1, m))
    del out, t
    torch.cuda.empty_cache()
    widths = dict(A=n * n, B=n * m, Q=n * n, R=m * m, Qf=n * n, x0=n)
    sub = {k: host[k].reshape(B, w)[idx].astype(np.float64).ravel() for k, w in widths.items()}
    sub.update(n=n, m=m, N=N, batch=len(idx))
    ref = oracle.dp_solve_abi(sub, N, nthreads=max(1, min(16, os.cpu_count() or 1)))
    assert (ref["info"] == 0).all()
    refK = from_abi(ref["K"], (len(idx), N - 1, m, n))
    refP = from_abi(ref["P"], (len(idx), n, n))
    errs = dict(K=relerr_per_knot(got["K"], refK),
                P=relerr_per_knot(got["P"][:, None], refP[:, None]),
                X=traj_err(got["X"], ref["X"].reshape(len(idx), N, n)),
                U=traj_err(got["U"], ref["U"].reshape(len(idx), N - 1, m)))
    print(f"\nfull-size n={n} m={m} N={N} B={B} {'f64' if f64 else 'f32'}: sample {len(idx)} "
          f"(last {idx[-1]}) rel err " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    return errs


def test_cfg4_full_batch_parity(lqrx, oracle, gpu_ok):
    """BASELINE configs[3]: n=32 m=16 N=256 B=65536 fp64, 256 sampled trajectories."""
    errs = full_size_case(lqrx, oracle, 32, 16, 256, 65536, True, 256, seed=20260104)
    assert errs["K"] <= TOL64 and errs["P"] <= TOL64
    assert errs["X"] <= TOL64 and errs["U"] <= TOL64


def test_cfg5_full_batch_parity_f32(lqrx, oracle, gpu_ok):
    """BASELINE configs[4]: n=64 m=32 N=512 B=8192 fp32 against the fp64 oracle."""
    errs = full_size_case(lqrx, oracle, 64, 32, 512, 8192, False, 48, seed=20260105)
    assert max(errs.values()) <= TOL32_N512


def test_dp64_wg4_full_batch_parity(lqrx, oracle, gpu_ok):
    """fp64 n=64 m=32 N=512 at the bench batch B=8192 on the four-wave kernel
    (dp_wg4_kernel<double, 2>): whole-batch device scan, 24 strided
    trajectories (0 and 8191 included) against the fp64 oracle."""
    errs = full_size_case(lqrx, oracle, 64, 32, 512, 8192, True, 24, seed=20260106)
    assert max(errs.values()) <= TOL64, errs


def kkt_full_size_case(lqrx, oracle, f64, B, nsample, seed):
    """configs[4]'s KKT half at its full batch: the trajectory structure n=64 m=32 N=512
    generated in HBM (206 GB of Y at B=8192 fp32 / B=4096 fp64 — past host memory), solved
    in ONE lqrx_kkt_solve call on the library's own scratch (no caller workspace: the default
    slab cap splits the batch into chunks), then a whole-batch device scan for non-finite δz, λ
    and info ≠ 0, and a strided sample (first and last trajectory included: the last
    trajectory's Y offset is B·1.26e7 elements, past 2³²) copied back as the kernel saw it and
    solved by the fp64 C oracle (cholesky_solver.jl _solve!)."""
    import torch
    import lqrx.kkt as K

    dev = torch.device("cuda", 0)
    n, m, N = 64, 32, 512
    st = K.trajectory_structure(n, m, N)
    tdt = torch.float64 if f64 else torch.float32
    t = K.random_kkt_device(st, B, seed, dev, tdt)
    assert t["Y"].numel() > 2 ** 32
    out = K.kkt_solve_device(st, t, K.H_DIAG, 1)
    torch.cuda.synchronize(dev)
    assert out["rc"] == 0 and int((out["info"] != 0).sum()) == 0
    assert bool(torch.isfinite(out["dz"]).all()) and bool(torch.isfinite(out["lam"]).all())
    idx = sample_index(B, nsample)
    ti = torch.from_numpy(idx).to(dev)
    pick = lambda x: x.view(B, -1).index_select(0, ti).double().cpu().numpy()
    Y, y, H, g = (pick(t[k]) for k in ("Y", "y", "H", "g"))
    dz, lam = pick(out["dz"]), pick(out["lam"])
    del out, t
    torch.cuda.empty_cache()
    ref = oracle.kkt_solve_batch(oracle.KktStructure(n, m, N, st.p), len(idx), Y, y, H, g, h_mode=2,
                                 nthreads=max(1, min(16, os.cpu_count() or 1)))
    assert (ref["info"] == 0).all()
    rel = lambda a, b: float((np.abs(a - b.reshape(a.shape)).max(axis=1)
                              / np.abs(b.reshape(a.shape)).max(axis=1)).max())
    e = dict(dz=rel(dz, ref["dz"]), lam=rel(lam, ref["lam"]))
    print(f"\nfull-size KKT n={n} m={m} N={N} B={B} {'f64' if f64 else 'f32'}: sample {len(idx)} "
          f"(last {idx[-1]}) rel err dz {e['dz']:.2e} lam {e['lam']:.2e}")
    return e


def test_cfg5_kkt_full_batch_parity_f32(lqrx, oracle, gpu_ok):
    """BASELINE configs[4]'s banded KKT: n=64 m=32 N=512 B=8192 fp32, 8 sampled trajectories
    against the fp64 oracle on the same fp32 inputs (1e-4, tests/test_kkt_big_gpu.py)."""
    e = kkt_full_size_case(lqrx, oracle, False, 8192, 8, seed=4242)
    assert max(e.values()) <= TOL32_N512


def test_cfg5_kkt_full_batch_parity_f64(lqrx, oracle, gpu_ok):
    """The same KKT shape in fp64 at B=4096 (the same 206 GB of Y), 1e-10."""
    e = kkt_full_size_case(lqrx, oracle, True, 4096, 8, seed=4243)
    assert max(e.values()) <= TOL64
