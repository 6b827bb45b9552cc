"""bench.py's plain run and `--dump-outputs DIR`.

CPU: the writer itself (bench.dump_outputs) on host tensors — row layout, the batch-fastest
layout, the dtypes written, and the fixed seeded sample once the outputs pass the size budget.
GPU: one plain `bench.py --dump-outputs` run as a child process: the line carries the headline
fields and none of the `--full` work, and the files hold exactly what lqrx_dp_solve returns for
the same counter-generated inputs.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_whole_batch_layouts_and_dtypes(tmp_path):
    import torch
    import bench

    bt = 7
    a = torch.arange(bt * 5, dtype=torch.float64)
    b = torch.arange(bt * 3, dtype=torch.float32)
    info = torch.arange(bt, dtype=torch.int32)
    rec = bench.dump_outputs(str(tmp_path / "rows"), {"a": a, "b": b, "info": info}, bt)
    got = _load(tmp_path / "rows")
    assert rec["trajectories"] == rec["of"] == bt and rec["sample"] is None
    assert got["a"].dtype == np.float64 and got["b"].dtype == np.float32 and got["info"].dtype == np.float64
    assert np.array_equal(got["a"], a.numpy().reshape(bt, 5))
    assert np.array_equal(got["b"], b.numpy().reshape(bt, 3))
    assert np.array_equal(got["info"], np.arange(bt, dtype=np.float64).reshape(bt, 1))
    # [element][batch] buffers come out as the same rows
    soa = a.view(bt, 5).t().contiguous().view(-1)
    bench.dump_outputs(str(tmp_path / "soa"), {"a": soa}, bt, soa=True)
    assert np.array_equal(_load(tmp_path / "soa")["a"], got["a"])


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    import torch
    import bench

    bt, w = 1000, 16
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100 * (w * 8 + 8))     # room for 100 trajectories
    x = torch.arange(bt * w, dtype=torch.float64)
    info = torch.arange(bt, dtype=torch.int32)
    rec = bench.dump_outputs(str(tmp_path / "one"), {"x": x, "info": info}, bt)
    bench.dump_outputs(str(tmp_path / "two"), {"x": x, "info": info}, bt)
    one, two = _load(tmp_path / "one"), _load(tmp_path / "two")
    assert rec["trajectories"] == 100 and rec["of"] == bt and rec["sample"]
    assert sum(v.nbytes for v in one.values()) <= bench.DUMP_BUDGET_BYTES
    rows = one["info"][:, 0].astype(np.int64)                      # info[i] = i: the rows taken
    assert len(set(rows)) == 100 and (np.diff(rows) > 0).all()
    assert np.array_equal(one["x"], x.numpy().reshape(bt, w)[rows])   # the same rows in every array
    assert all(np.array_equal(one[k], two[k]) for k in one)           # and in every run
    assert bench.DUMP_BUDGET_BYTES < 64e6


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_timed_outputs(lqrx, gpu_ok, tmp_path):
    import torch

    N, bt, seed = 16, 37, 5
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--N", str(N), "--batch", str(bt), "--seed", str(seed),
                        "--dump-outputs", str(tmp_path / "out")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["dtype"] == "f64"
    assert line["unit"] == "trajectories/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(bt / (line["ms_per_step"] * 1e-3), rel=1e-9)
    # a plain run does none of the --full work
    assert line["full"] is False and line["cpu_baseline"] is None and line["check"] is None
    assert line["dump_outputs"]["trajectories"] == bt

    n, m = 32, 16
    got = _load(tmp_path / "out")
    assert sorted(got) == ["K", "P", "U", "X", "info"]
    d = lqrx.random_batch(n, m, N, bt, seed=seed)
    t = {k: torch.from_numpy(d[k]).cuda() for k in ("A", "B", "Q", "R", "Qf", "x0")}
    t.update(n=n, m=m, batch=bt)
    ref = lqrx.dp_solve_device(t, N, p_mode=0)
    torch.cuda.synchronize()
    for k, w in (("K", (N - 1) * m * n), ("P", n * n), ("X", N * n), ("U", (N - 1) * m), ("info", 1)):
        assert got[k].dtype == np.float64 and got[k].shape == (bt, w), k
        assert np.array_equal(got[k], ref[k].double().view(bt, w).cpu().numpy()), k
    assert (got["info"] == 0).all()
