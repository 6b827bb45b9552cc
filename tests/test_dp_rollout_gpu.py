"""GPU tests of the scenario rollout (lqrx_dp_rollout[_host], include/lqrx.h).

K and d come from lqrx_dp_solve_cross on cross_problem (tests/dp_truth.py), so every E is positive
definite; the truth is the numpy checker tests/dp_rollout_truth.py on the same K, d (and, in fp32, on the
fp32-rounded problem), so only the rollout's rounding is measured.  X and U are measured as
max|a − b| / max(1, max|b|) (dp_truth.check's measure), J relative to max(1, Σ_k|terms|) (value_errors'
convention), against the project's TOL64 = 1e-10 and TOL32 = 1e-4.  Every figure is printed before it
is asserted.

Observed on an MI355X (profiles/r10/rollout/rollout_gpu_tests.log: the file's cases in about 3 s):
worst fp64 X 2.9e-15, U 6.2e-14, J 1.0e-14; fp32 X 9.0e-7, U 6.5e-7, J 4.7e-7; the clamped runs have
11.8 – 20.6 % of U exactly at a bound; no guard touched, no output element left unwritten.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from dp_rollout_truth import (check_clamp_condition, clamp_bounds, cross_problem, j_error, rollout_np,
                              scenarios, xu_error)
from dp_truth import F32_SHAPES
from guarded import check as guard_check, guard_all, pattern_filled

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL32 = 1e-4
# (n, m, N, batch, tv)
SHAPES = [(1, 1, 6, 3, False), (4, 1, 40, 8, False), (6, 3, 30, 7, False), (17, 5, 12, 3, True),
          (32, 16, 40, 4, False), (24, 18, 10, 3, False), (64, 32, 12, 2, False), (48, 16, 10, 2, True),
          (65, 4, 8, 2, False), (70, 8, 9, 3, True)]
PARITY = [(sh, S) for sh in SHAPES for S in (1, 5, 16, 21)] + [((32, 16, 256, 2, True), 3)]
CLAMP = [(4, 1, 40, 8, False), (6, 3, 30, 7, False), (32, 16, 40, 4, False), (64, 32, 12, 2, False),
         (65, 4, 8, 2, False)]
MFMA_SHAPE, WG_SHAPE = (17, 5, 12, 3, True), (65, 4, 8, 2, False)
PROBLEM = ("A", "B", "c", "Q", "R", "Qf", "M", "q", "r", "qf", "x0")
sid = lambda sh: "x".join(map(str, sh))


def dev(a, npdt):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=npdt)).reshape(-1)).to("cuda:0")


def host(x):
    return x.cpu().numpy().astype(np.float64)


def bits(x):
    import torch

    return x.view({8: torch.int64, 4: torch.int32}[x.element_size()])


def same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Case:
    """A solved problem on the device, its scenarios, and (lazily) the checker's result for them."""

    def __init__(self, lqrx, shape, prec, S):
        self.lqrx, self.shape, self.prec, self.S = lqrx, shape, prec, S
        n, m, N, bt, tv = shape
        self.npdt = np.float64 if prec == "f64" else np.float32
        self.tol = TOL64 if prec == "f64" else TOL32
        d = cross_problem(lqrx, n, m, N, bt, 3, tv_QR=tv, tv_AB=tv)
        for k in PROBLEM:   # the problem as the device sees it
            d[k] = np.asarray(d[k], self.npdt).astype(np.float64)
        self.d = d
        self.t = {k: dev(d[k], self.npdt) for k in PROBLEM}
        self.t.update(n=n, m=m, batch=bt, tv_AB=int(tv), tv_QR=int(tv))
        self.sol = lqrx.dp_solve_device(self.t, N)
        assert (self.sol["info"] == 0).all().item()
        self.K, self.dd = host(self.sol["K"]), host(self.sol["d"])
        sc = scenarios(n, m, N, bt, S, seed=11)
        self.sc_np = {k: np.asarray(v, self.npdt).astype(np.float64) for k, v in sc.items()}
        self.sc = {k: dev(v, self.npdt) for k, v in self.sc_np.items()}

    @functools.cached_property
    def ref(self):
        return rollout_np(self.d, self.shape[2], self.K, self.dd, **self.sc_np)

    def run(self, outputs=("X", "U", "J"), out=None, t=None, K=None, d=None, stream=None, **sc):
        """the device entry on this case's scenarios; sc overrides / removes (None) scenario fields"""
        s = dict(self.sc, S=self.S, outputs=outputs)
        s.update(sc)
        return self.lqrx.dp_rollout_device(t or self.t, self.shape[2], self.sol["K"] if K is None else K,
                                           self.sol["d"] if d is None else d, s, stream=stream, out=out)

    def logical(self, r):
        n, m, N, bt, _ = self.shape
        sh = dict(X=(bt, self.S, N, n), U=(bt, self.S, N - 1, m), J=(bt, self.S))
        return {k: host(r[k]).reshape(sh[k]) for k in ("X", "U", "J") if k in r}

    def check(self, r, ref, what):
        got = self.logical(r)
        e = dict(X=xu_error(got["X"], ref["X"]), U=xu_error(got["U"], ref["U"]), J=j_error(got["J"], ref))
        print(f"PARITY rollout {what} {self.shape} S={self.S} {self.prec}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            assert v <= self.tol, (k, v)
        return got


@functools.lru_cache(maxsize=None)
def case(lqrx, shape, prec="f64", S=21):
    return Case(lqrx, shape, prec, S)


@pytest.mark.parametrize("shape,S", PARITY, ids=[f"{sid(sh)}-S{S}" for sh, S in PARITY])
def test_parity_f64(lqrx, gpu_ok, shape, S):
    c = case(lqrx, shape, "f64", S)
    c.check(c.run(), c.ref, "parity")


@pytest.mark.parametrize("shape", F32_SHAPES, ids=[sid(sh) for sh in F32_SHAPES])
def test_parity_f32(lqrx, gpu_ok, shape):
    c = case(lqrx, shape, "f32", 21)
    c.check(c.run(), c.ref, "parity")


def test_grid_of_many_tiles(lqrx, gpu_ok):
    """batch = 3, S = 1000: 63 tiles per problem, the last one partial"""
    c = case(lqrx, (6, 3, 5, 3, False), "f64", 1000)
    c.check(c.run(), c.ref, "grid")


@pytest.mark.parametrize("shape", CLAMP, ids=[sid(sh) for sh in CLAMP])
def test_clamp(lqrx, gpu_ok, shape):
    """Bounds at ±(0.9 quantile of |u| per control row of the unclamped reference rollout): parity at
    the same tolerances, every returned U inside [u_lo, u_hi] exactly, and at least 5 % of U at a
    bound and 5 % strictly inside, on the reference and on the result."""
    c = case(lqrx, shape, "f64", 21)
    lo, hi = clamp_bounds(c.ref["U"])
    ref = rollout_np(c.d, shape[2], c.K, c.dd, **c.sc_np, u_lo=lo, u_hi=hi)
    check_clamp_condition(ref["U"], lo, hi, f"reference {shape}")
    got = c.check(c.run(u_lo=dev(lo, c.npdt), u_hi=dev(hi, c.npdt)), ref, "clamp")
    assert (got["U"] >= lo[:, None, None, :]).all() and (got["U"] <= hi[:, None, None, :]).all()
    check_clamp_condition(got["U"], lo, hi, f"device {shape}")


@pytest.mark.parametrize("shape", [(6, 3, 30, 7, False), (32, 16, 40, 4, True), (65, 4, 8, 2, False)], ids=sid)
def test_identities_against_the_solve(lqrx, gpu_ok, shape):
    """S = 1, α = 1 and the solve's own x0: X and U of lqrx_dp_solve_cross, J of lqrx_dp_solve_value;
    and J(α) = J(1) + ½(1 − α)² dV for α ∈ {0, ½, 1} with the library's dV."""
    n, m, N, bt, tv = shape
    c = case(lqrx, shape, "f64", 1)
    val = lqrx.dp_solve_device(c.t, N, value=True)
    r = c.run(x0=c.t["x0"], alpha=None, w=None)
    eX = xu_error(host(r["X"]), host(c.sol["X"]))
    eU = xu_error(host(r["U"]), host(c.sol["U"]))
    ref = rollout_np(c.d, N, c.K, c.dd, c.d["x0"].reshape(bt, 1, n))
    eJ = j_error(host(val["J"]), ref)
    eJr = j_error(host(r["J"]), dict(J=host(val["J"]).reshape(bt, 1), T=ref["T"]))
    print(f"IDENTITY rollout {shape}: X {eX:.2e} U {eU:.2e} J vs value {eJr:.2e} (value vs checker {eJ:.2e})")
    assert eX <= TOL64 and eU <= TOL64 and eJr <= TOL64
    al = np.array([0.0, 0.5, 1.0])
    c3 = Case(lqrx, shape, "f64", 3)
    x3 = np.repeat(c.d["x0"].reshape(bt, 1, n), 3, axis=1)
    r3 = c3.run(outputs=("J",), K=c.sol["K"], d=c.sol["d"], x0=dev(x3, np.float64), alpha=dev(np.tile(al, (bt, 1)), np.float64), w=None)
    J3 = host(r3["J"]).reshape(bt, 3)
    T3 = rollout_np(c.d, N, c.K, c.dd, x3, alpha=np.tile(al, (bt, 1)))["T"]
    want = J3[:, 2:3] + 0.5 * (1 - al) ** 2 * host(val["dV"])[:, None]
    e3 = float((np.abs(J3 - want) / np.maximum(1, T3)).max())
    print(f"IDENTITY rollout {shape}: three-α {e3:.2e}")
    assert e3 <= TOL64


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", [MFMA_SHAPE, WG_SHAPE], ids=sid)
def test_bits_do_not_depend_on_S_or_position(lqrx, gpu_ok, shape, prec):
    """Scenario j of an S = 21 call is, bit for bit, the S = 1 call on that scenario alone."""
    n, m, N, bt, tv = shape
    c = case(lqrx, shape, prec, 21)
    full = c.run()
    view = lambda x, per: x.view(bt, 21, per)
    c1 = Case(lqrx, shape, prec, 1)
    for j in (0, 3, 15, 16, 20):
        pick = lambda k, per: view(c.sc[k], per)[:, j].contiguous().view(-1)
        one = c1.run(K=c.sol["K"], d=c.sol["d"], x0=pick("x0", n), alpha=pick("alpha", 1), w=pick("w", (N - 1) * n))
        for k, per in (("X", N * n), ("U", (N - 1) * m), ("J", 1)):
            assert same_bits(view(full[k], per)[:, j].contiguous().view(-1), one[k]), (k, j)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", [MFMA_SHAPE, WG_SHAPE], ids=sid)
def test_bits_of_defaults_and_reruns(lqrx, gpu_ok, shape, prec):
    """alpha = NULL is an all-ones alpha, NULL bounds are −inf / +inf, and two runs are equal."""
    import torch

    n, m, N, bt, tv = shape
    c = case(lqrx, shape, prec, 21)
    a, b = c.run(), c.run()
    ones = torch.ones_like(c.sc["alpha"])
    an, a1 = c.run(alpha=None), c.run(alpha=ones)
    inf = torch.full((bt * m,), float("inf"), dtype=ones.dtype, device=ones.device)
    bi, bl, bh = c.run(u_lo=-inf, u_hi=inf), c.run(u_lo=-inf), c.run(u_hi=inf)
    for k in ("X", "U", "J"):
        assert same_bits(a[k], b[k]), k
        assert same_bits(an[k], a1[k]), k
        assert same_bits(a[k], bi[k]) and same_bits(a[k], bl[k]) and same_bits(a[k], bh[k]), k


def _filled(like, sizes):
    return {k: pattern_filled(like, sz) for k, sz in sizes.items()}


@pytest.mark.parametrize("shape,S", [(MFMA_SHAPE, 21), (WG_SHAPE, 5)], ids=["mfma", "wg"])
def test_option_subsets_and_extents_device(lqrx, gpu_ok, shape, S):
    """Only J, only X, X + U, and all three, each on guarded buffers (inputs guarded as well): every
    output element written, no guard touched, and the tensors asked for are the bits of the
    all-outputs run on plain tensors."""
    n, m, N, bt, tv = shape
    c = case(lqrx, shape, "f64", S)
    sizes = dict(X=bt * S * N * n, U=bt * S * (N - 1) * m, J=bt * S)
    plain = c.run(out=_filled(c.t["A"], sizes))
    c.check(plain, c.ref, "plain")
    lo, hi = clamp_bounds(c.ref["U"])
    for outputs in (("J",), ("X",), ("X", "U"), ("X", "U", "J")):
        for bounded in (False, True):
            hs = []
            tg = guard_all(c.t, "in", bt, hs)
            kd = guard_all(dict(K=c.sol["K"], d=c.sol["d"]), "in", bt, hs)
            extra = dict(u_lo=dev(lo, np.float64), u_hi=dev(hi, np.float64)) if bounded else {}
            sg = guard_all(dict(c.sc, **extra), "in", bt, hs)
            og = guard_all(_filled(c.t["A"], {k: sizes[k] for k in outputs}), "out", bt, hs)
            r = c.run(outputs=outputs, out=og, t=tg, K=kd["K"], d=kd["d"], **sg)
            guard_check(hs)
            assert set(r) == set(outputs) | {"rc"}
            if bounded:
                want = c.run(**extra)
            for k in outputs:
                assert same_bits(r[k], (want if bounded else plain)[k]), (outputs, bounded, k)


@pytest.mark.parametrize("shape,S", [(MFMA_SHAPE, 21), (WG_SHAPE, 5)], ids=["mfma", "wg"])
def test_extents_host_entry(lqrx, gpu_ok, shape, S):
    """lqrx_dp_rollout_host on guarded host arrays: D2H of exactly the outputs asked for, every
    element written, no guard touched; the bits of the device entry."""
    from lqrx import _lib

    n, m, N, bt, tv = shape
    c = case(lqrx, shape, "f64", S)
    devr = c.run()
    sizes = dict(X=bt * S * N * n, U=bt * S * (N - 1) * m, J=bt * S)
    desc = _lib.DpDesc(n, m, N, _lib.F64, bt, 0, 0, int(tv), int(tv))
    p = lambda a: None if a is None else a.ctypes.data
    for outputs in (("X", "U", "J"), ("U",)):
        hs = []
        ins = {k: np.ascontiguousarray(c.d[k]).reshape(-1) for k in PROBLEM if k != "x0"}
        ins.update(K=c.K.reshape(-1), d=c.dd.reshape(-1))
        ins.update({k: np.ascontiguousarray(v).reshape(-1) for k, v in c.sc_np.items()})
        ig = guard_all(ins, "in", bt, hs)
        og = guard_all(_filled(ins["A"], {k: sizes[k] for k in outputs}), "out", bt, hs)
        cost = _lib.DpCost(*[p(ig[k]) for k in ("Q", "R", "Qf", "M", "q", "r", "qf")])
        sc = _lib.DpScenarios(S, p(ig["x0"]), p(ig["alpha"]), p(ig["w"]), None, None,
                              *[p(og.get(k)) for k in ("X", "U", "J")])
        rc = lqrx.load().lqrx_dp_rollout_host(C.byref(desc), *[C.c_void_p(p(ig[k])) for k in ("A", "B", "c", "K", "d")],
                                              C.byref(cost) if "J" in outputs else None, C.byref(sc))
        assert rc == 0, lqrx.load().lqrx_last_error().decode()
        guard_check(hs)
        for k in outputs:
            assert np.array_equal(og[k].view(np.int64), devr[k].cpu().numpy().view(np.int64)), (outputs, k)


def test_rollout_batch_host_arrays(lqrx, gpu_ok):
    """lqrx.rollout_batch on logical host arrays: the checker's result."""
    from dp_truth import to_batch
    from lqrx.dp import from_abi

    shape = (6, 3, 30, 7, False)
    n, m, N, bt, tv = shape
    c = case(lqrx, shape, "f64", 5)
    r = lqrx.rollout_batch(to_batch(c.d, N), from_abi(c.K, (bt, N - 1, m, n)), c.dd.reshape(bt, N - 1, m),
                           c.sc_np["x0"], alpha=c.sc_np["alpha"], w=c.sc_np["w"])
    e = dict(X=xu_error(r["X"], c.ref["X"]), U=xu_error(r["U"], c.ref["U"]), J=j_error(r["J"], c.ref))
    print("PARITY rollout_batch " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= TOL64
    rj = lqrx.rollout_batch(to_batch(c.d, N), from_abi(c.K, (bt, N - 1, m, n)), c.dd.reshape(bt, N - 1, m),
                            c.sc_np["x0"], alpha=c.sc_np["alpha"], w=c.sc_np["w"], outputs=("J",))
    assert set(rj) == {"J", "rc"} and np.array_equal(rj["J"], r["J"])


@pytest.mark.parametrize("shape", [MFMA_SHAPE, WG_SHAPE], ids=sid)
def test_rollout_is_capturable(lqrx, gpu_ok, shape):
    """The device entry takes no library scratch and never synchronises on a caller's stream: one
    call captured in a hipGraph (tests/test_graph_gpu.py's procedure), replayed on a second set of
    scenarios, gives the bits of an eager call on them."""
    from test_graph_gpu import _capture_and_replay

    n, m, N, bt, tv = shape
    c = case(lqrx, shape, "f64", 21)
    ins = {k: v.clone() for k, v in c.sc.items()}
    second = {k: dev(v, np.float64) for k, v in scenarios(n, m, N, bt, 21, seed=12).items()}
    got, ref = _capture_and_replay(lambda s: c.run(stream=s, **ins), ins, second)
    for k in ("X", "U", "J"):
        assert same_bits(got[k], ref[k]), k
    assert not same_bits(got["X"], c.run()["X"])     # the replay saw the second set
