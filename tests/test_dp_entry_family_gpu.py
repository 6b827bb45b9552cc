"""Characterization of the DP entry family: each kind of solve (plain, linear, affine, cross, value)
gives the same bits through its `_host` entry (lqrx.solve_batch on host arrays) and through its
device entry (lqrx.dp_solve_device on torch tensors, null stream), in layout 0 and layout 1.

Both paths hand the same ABI bytes to the same kernel, which works one wave or lane per trajectory
with no arithmetic across trajectories, so the results are equal exactly (tests/test_devices_gpu.py
relies on the same fact); there is no tolerance and no oracle here.  Two shapes: (3, 2, 5, 5) runs
the lane kernel, which reads layout 1 natively; (6, 3, 5, 3) runs the MFMA kernel, which stages
layout 1 through layout-0 scratch.  fp64, fixed seeds, p_mode 0 for every kind and p_mode 1 for the
value kind (s then holds every s_k and is staged like p).
"""
import numpy as np
import pytest

from dp_truth import cross_problem, to_batch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 5, 5), (6, 3, 5, 3)]
# kind → the optional inputs it passes, in the order the kinds nest
KINDS = {"plain": (), "linear": ("q", "r", "qf"), "affine": ("q", "r", "qf", "c"),
         "cross": ("q", "r", "qf", "c", "M"), "value": ("q", "r", "qf", "c", "M")}
CASES = [(k, lay, sh, 0) for k in KINDS for lay in (0, 1) for sh in SHAPES] + \
        [("value", lay, sh, 1) for lay in (0, 1) for sh in SHAPES]


@pytest.fixture(scope="module")
def problems(lqrx):
    """One cross problem per shape, shared by every case and left unchanged."""
    return {sh: cross_problem(lqrx, *sh, 8100 + sh[0]) for sh in SHAPES}


@pytest.mark.parametrize("kind,layout,shape,p_mode", CASES,
                         ids=[f"{k}-l{lay}-n{sh[0]}-p{pm}" for k, lay, sh, pm in CASES])
def test_host_and_device_entries_agree_bitwise(lqrx, gpu_ok, problems, kind, layout, shape, p_mode):
    import torch
    from lqrx.dp import from_abi, from_soa, to_soa

    n, m, N, bt = shape
    d = problems[shape]
    opt = KINDS[kind]
    value = kind == "value"

    b = to_batch(d, N)
    for k in ("q", "r", "qf", "c", "M"):
        if k not in opt:
            setattr(b, k, None)
    host = lqrx.solve_batch(b, all_P=bool(p_mode), layout=layout, value=value)

    dev = torch.device("cuda:0")
    lay = (lambda a: to_soa(a, bt)) if layout == 1 else (lambda a: a)
    t = {k: torch.from_numpy(lay(np.ascontiguousarray(d[k], np.float64)).reshape(-1)).to(dev)
         for k in ("A", "B", "Q", "R", "Qf", "x0") + opt}
    t.update(n=n, m=m, batch=bt)
    out = lqrx.dp_solve_device(t, N, p_mode=p_mode, layout=layout, value=value)
    assert out["rc"] == host["rc"] == 0
    unlay = (lambda a: from_soa(a, bt)) if layout == 1 else (lambda a: a)
    got = {k: unlay(out[k].cpu().numpy()) for k in out if k not in ("rc", "info", "dV", "J")}
    got["K"] = from_abi(got["K"], (bt, N - 1, m, n))
    got["P"] = from_abi(got["P"], (bt, N, n, n) if p_mode else (bt, n, n))
    keys = ["K", "P", "X", "U", "info"] + (["d", "p"] if opt else []) + (["s", "dV", "J"] if value else [])
    assert sorted(k for k in host if k != "rc") == sorted(keys)
    for k in keys:
        g = out[k].cpu().numpy() if k in ("info", "dV", "J") else got[k]
        assert np.isfinite(host[k]).all(), k
        assert np.array_equal(np.asarray(g).reshape(host[k].shape), host[k]), (k, kind, layout, shape, p_mode)
