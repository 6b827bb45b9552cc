"""GPU tests of the re-solve (lqrx_dp_factor[_host], lqrx_dp_resolve[_host], include/lqrx.h).

P and K come from lqrx_dp_solve_cross (p_mode 1) on cross_problem (tests/dp_truth.py), so every E is
positive definite.  The factor is compared with float64 numpy on the device's own P (per knot,
relative to max|·|); the sweep with the numpy checker tests/dp_resolve_truth.py in float64 on the
device's own K, E⁻¹, Pc (and, in fp32, on the fp32-rounded problem and right-hand sides), so only the
sweep's rounding is measured: d and p with dp_truth.relerr_traj, X and U as
max|a − b| / max(1, max|b|), against the project's TOL64 = 1e-10 and TOL32 = 1e-4.  Every figure is
printed before it is asserted.

Observed on an MI355X (profiles/r13/resolve/resolve_gpu_tests.log: the file's 75 cases in about 3 s):
worst fp64 factor E⁻¹ 7.2e-15, Pc 1.0e-15, sweep d 2.1e-14, p 4.2e-15, X 1.4e-14, U 1.8e-14, end to end
d 5.0e-13, X 6.1e-14, U 1.1e-13, adjoint identity 1.0e-15; fp32 factor 7.8e-7, sweep d 4.2e-6, U 4.6e-6;
no guard touched, no output element left unwritten, one kernel node in the captured graph.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from dp_resolve_truth import F32_SHAPES, SHAPES, factor_np, random_rhs, resolve_np, xu_error
from dp_truth import cross_problem, relerr_per_knot, relerr_traj
from guarded import check as guard_check, guard_all, pattern_filled

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL32 = 1e-4
S_ALL = (1, 5, 16, 21)
PARITY = [(sh, S) for sh in SHAPES for S in S_ALL]
PARITY32 = [(sh, S) for sh in F32_SHAPES for S in S_ALL]
BITS_SHAPE = (17, 5, 12, 3, True)
PROBLEM = ("A", "B", "c", "Q", "R", "Qf", "M", "q", "r", "qf", "x0")
RHS = ("q", "r", "qf", "x0")
OUT = ("d", "p", "X", "U")
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


class Solved:
    """A cross problem solved on the device with every P_k, and its factors from lqrx_dp_factor."""

    def __init__(self, lqrx, shape, prec):
        self.lqrx, self.shape, self.prec = lqrx, shape, prec
        n, m, N, bt, tv = shape
        self.npdt = np.float64 if prec == "f64" else np.float32
        self.tol = TOL64 if prec == "f64" else TOL32
        d = cross_problem(lqrx, n, m, N, bt, 3, tv_QR=tv, tv_AB=tv)
        for k in PROBLEM:   # the problem as the device sees it
            d[k] = np.asarray(d[k], self.npdt).astype(np.float64)
        self.d = d
        self.t = {k: dev(d[k], self.npdt) for k in PROBLEM}
        self.t.update(n=n, m=m, batch=bt, tv_AB=int(tv), tv_QR=int(tv))
        self.sol = lqrx.dp_solve_device(self.t, N, p_mode=1)
        assert (self.sol["info"] == 0).all().item()
        self.fac = lqrx.dp_factor_device(self.t, N, self.sol["P"])
        self.facd = dict(K=self.sol["K"], Einv=self.fac["Einv"], Pc=self.fac["Pc"])
        self.K, self.Einv, self.Pc = host(self.sol["K"]), host(self.fac["Einv"]), host(self.fac["Pc"])


@functools.lru_cache(maxsize=None)
def solved(lqrx, shape, prec="f64"):
    return Solved(lqrx, shape, prec)


class Case:
    """S right-hand sides per problem on a Solved, and (lazily) the checker's result for them."""

    def __init__(self, sv, S, seed=11):
        self.sv, self.S = sv, S
        n, m, N, bt, tv = sv.shape
        rhs = random_rhs(n, m, N, bt, S, seed, tv)
        self.rhs_np = {k: np.asarray(v, sv.npdt).astype(np.float64) for k, v in rhs.items()}
        self.rhs = {k: dev(v, sv.npdt) for k, v in self.rhs_np.items()}

    @functools.cached_property
    def ref(self):
        sv = self.sv
        return resolve_np(sv.d, sv.shape[2], sv.K, sv.Einv, sv.Pc, self.S, tv_QR=int(sv.shape[4]), **self.rhs_np)

    def run(self, outputs=OUT, out=None, t=None, fac=None, stream=None, p_mode=1, **rhs):
        """the device entry on this case's right-hand sides; rhs overrides / removes (None) fields"""
        sv = self.sv
        r = dict(self.rhs, S=self.S, outputs=outputs, tv_QR=int(sv.shape[4]), p_mode=p_mode)
        r.update(rhs)
        return sv.lqrx.dp_resolve_device(t or sv.t, sv.shape[2], fac or sv.facd, r, stream=stream, out=out)

    def sizes(self, p_mode=1):
        n, m, N, bt, _ = self.sv.shape
        S = self.S
        return dict(d=bt * S * (N - 1) * m, p=bt * S * (N if p_mode else 1) * n, X=bt * S * N * n, U=bt * S * (N - 1) * m)

    def check(self, r, ref, what):
        n, m, N, bt, _ = self.sv.shape
        flat = lambda a: np.asarray(a, np.float64).reshape(bt * self.S, -1)
        e = dict(d=relerr_traj(flat(host(r["d"])), flat(ref["d"])), p=relerr_traj(flat(host(r["p"])), flat(ref["p"])),
                 X=xu_error(host(r["X"]), ref["X"].ravel()), U=xu_error(host(r["U"]), ref["U"].ravel()))
        print(f"PARITY resolve {what} {self.sv.shape} S={self.S} {self.sv.prec}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            assert v <= self.sv.tol, (k, v)


@functools.lru_cache(maxsize=None)
def case(lqrx, shape, prec="f64", S=21):
    return Case(solved(lqrx, shape, prec), S)


# ---- the factor ----
def _factor_parity(sv):
    n, m, N, bt, tv = sv.shape
    ref = factor_np(dict(sv.d, tv_AB=int(tv), tv_QR=int(tv)), N, host(sv.sol["P"]))
    eE = relerr_per_knot(sv.Einv.reshape(bt, N - 1, m * m), ref["Einv"].reshape(bt, N - 1, m * m))
    eP = relerr_per_knot(sv.Pc.reshape(bt, N - 1, n), ref["Pc"].reshape(bt, N - 1, n))
    Ei = sv.Einv.reshape(bt * (N - 1), m, m)
    print(f"PARITY factor {sv.shape} {sv.prec}: Einv {eE:.2e} Pc {eP:.2e}")
    assert (ref["info"] == 0).all() and (sv.fac["info"] == 0).all().item()
    assert eE <= sv.tol and eP <= sv.tol
    assert np.array_equal(Ei, np.swapaxes(Ei, -1, -2))          # exactly symmetric


@pytest.mark.parametrize("shape", SHAPES, ids=[sid(sh) for sh in SHAPES])
def test_factor_parity_f64(lqrx, gpu_ok, shape):
    _factor_parity(solved(lqrx, shape, "f64"))


@pytest.mark.parametrize("shape", F32_SHAPES, ids=[sid(sh) for sh in F32_SHAPES])
def test_factor_parity_f32(lqrx, gpu_ok, shape):
    _factor_parity(solved(lqrx, shape, "f32"))


def test_factor_reports_the_largest_indefinite_knot(lqrx, gpu_ok):
    """A time-varying R made negative definite (−10⁶·I, far past BᵀPB) at chosen knots, on the P of the
    valid problem: info is the largest such knot of each problem, every output element is written and
    finite, and the knots left alone keep the bits of the valid run (the knots are independent)."""
    sv = solved(lqrx, BITS_SHAPE, "f64")
    n, m, N, bt, tv = sv.shape
    bad = {0: (), 1: (4,), 2: (3, 9)}
    R = sv.t["R"].clone().view(bt, N - 1, m * m)
    neg = dev(-1e6 * np.eye(m), np.float64)
    for b, ks in bad.items():
        for k0 in ks:
            R[b, k0 - 1] = neg
    hs = []
    og = guard_all(dict(Einv=pattern_filled(sv.t["A"], bt * (N - 1) * m * m), Pc=pattern_filled(sv.t["A"], bt * (N - 1) * n),
                        info=pattern_filled(sv.sol["info"], bt)), "out", bt, hs)
    r = lqrx.dp_factor_device(dict(sv.t, R=R.view(-1)), N, sv.sol["P"], out=og)
    guard_check(hs)
    info = r["info"].cpu().numpy()
    print(f"FACTOR info {info.tolist()} for indefinite knots {bad}")
    assert info.tolist() == [max(ks, default=0) for ks in bad.values()]
    assert same_bits(r["Pc"], sv.fac["Pc"])
    E, E0 = bits(r["Einv"]).view(bt, N - 1, m * m), bits(sv.fac["Einv"]).view(bt, N - 1, m * m)
    for b, ks in bad.items():
        for k in range(1, N):
            assert (k in ks) != bool((E[b, k - 1] == E0[b, k - 1]).all().item()), (b, k)


# ---- the sweep ----
@pytest.mark.parametrize("shape,S", PARITY, ids=[f"{sid(sh)}-S{S}" for sh, S in PARITY])
def test_sweep_parity_f64(lqrx, gpu_ok, shape, S):
    c = case(lqrx, shape, "f64", S)
    c.check(c.run(), c.ref, "sweep")


@pytest.mark.parametrize("shape,S", PARITY32, ids=[f"{sid(sh)}-S{S}" for sh, S in PARITY32])
def test_sweep_parity_f32(lqrx, gpu_ok, shape, S):
    c = case(lqrx, shape, "f32", S)
    c.check(c.run(), c.ref, "sweep")


@pytest.mark.parametrize("shape", [(6, 3, 30, 7, False), (32, 16, 40, 4, True), (64, 32, 12, 2, False)], ids=sid)
def test_end_to_end_against_the_replicated_solve(lqrx, gpu_ok, shape):
    """lqrx_dp_solve_cross on the batch·S replicated problems with the same q, r, qf, x0."""
    import torch

    n, m, N, bt, tv = shape
    S = 5
    c = case(lqrx, shape, "f64", S)
    sv = c.sv
    per = lambda k: sv.t[k].numel() // bt
    t = {k: sv.t[k].view(bt, 1, per(k)).expand(bt, S, per(k)).contiguous().view(-1) for k in ("A", "B", "c", "Q", "R", "Qf", "M")}
    t.update(c.rhs)
    t.update(n=n, m=m, batch=bt * S, tv_AB=int(tv), tv_QR=int(tv))
    full = lqrx.dp_solve_device(t, N, p_mode=1)
    assert (full["info"] == 0).all().item()
    torch.cuda.synchronize()
    ref = {k: host(full[k]) for k in OUT}
    c.check(c.run(), ref, "end to end")


def test_adjoint_identity(lqrx, gpu_ok):
    """q = gX, r = gU, x0 = 0, c = NULL, knot_stride_QR = 1: X' and U' of lqrx_dp_solve_adjoint, which it
    returns as the gradients with respect to q (and qf at knot N) and r."""
    sv = solved(lqrx, BITS_SHAPE, "f64")
    n, m, N, bt, tv = sv.shape
    rng = np.random.default_rng(41)
    gX, gU = rng.standard_normal((bt, N, n)), rng.standard_normal((bt, N - 1, m))
    fwd = lqrx.dp_solve_device(sv.t, N, costates=True)
    adj = lqrx.dp_adjoint_device(sv.t, fwd, dev(gX, np.float64), dev(gU, np.float64), want=("q", "r", "qf"), N=N)
    assert (adj["info"] == 0).all().item()
    t = {k: v for k, v in sv.t.items() if k != "c"}
    fac = lqrx.dp_factor_device(t, N, sv.sol["P"])
    assert fac["Pc"] is None and same_bits(fac["Einv"], sv.fac["Einv"])
    r = lqrx.dp_resolve_device(t, N, dict(K=sv.sol["K"], Einv=fac["Einv"], Pc=None),
                               dict(S=1, q=dev(gX[:, :N - 1], np.float64), r=dev(gU, np.float64),
                                    qf=dev(gX[:, N - 1], np.float64), tv_QR=1, outputs=("d", "X", "U")))
    X = host(r["X"]).reshape(bt, N, n)
    e = dict(gq=xu_error(X[:, :N - 1], host(adj["q"]).reshape(bt, N - 1, n)), gqf=xu_error(X[:, N - 1], host(adj["qf"]).reshape(bt, n)),
             gr=xu_error(host(r["U"]), host(adj["r"])))
    print("IDENTITY resolve adjoint: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= TOL64


def test_grid_of_many_tiles(lqrx, gpu_ok):
    """batch = 3, S = 1000: 63 tiles per problem, the last one partial"""
    c = case(lqrx, (6, 3, 5, 3, False), "f64", 1000)
    c.check(c.run(), c.ref, "grid")


# ---- bit equality ----
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bits_do_not_depend_on_S_or_position(lqrx, gpu_ok, prec):
    """Right-hand side j of an S = 21 call is, bit for bit, that right-hand side alone (S = 1) and in
    another position of an S = 5 call."""
    sv = solved(lqrx, BITS_SHAPE, prec)
    n, m, N, bt, tv = sv.shape
    c = case(lqrx, BITS_SHAPE, prec, 21)
    full = c.run()
    per = dict(q=(N - 1) * n, r=(N - 1) * m, qf=n, x0=n, d=(N - 1) * m, p=N * n, X=N * n, U=(N - 1) * m)
    view = lambda x, k, S: x.view(bt, S, per[k])
    c1, c5 = Case(sv, 1), Case(sv, 5)
    for j in (0, 3, 15, 16, 20):
        one = c1.run(**{k: view(c.rhs[k], k, 21)[:, j].contiguous().view(-1) for k in RHS})
        for k in OUT:
            assert same_bits(view(full[k], k, 21)[:, j].contiguous().view(-1), one[k]), (k, j)
    js = (20, 0, 16, 3, 15)   # positions 0 … 4 of the S = 5 call
    five = c5.run(**{k: view(c.rhs[k], k, 21)[:, list(js)].contiguous().view(-1) for k in RHS})
    for pos, j in enumerate(js):
        for k in OUT:
            assert same_bits(view(full[k], k, 21)[:, j], view(five[k], k, 5)[:, pos]), (k, j, pos)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bits_of_subsets_defaults_and_reruns(lqrx, gpu_ok, prec):
    """Output subsets, NULL against zero-filled q, r, qf, x0, p_mode 0 against 1, and two runs."""
    import torch

    sv = solved(lqrx, BITS_SHAPE, prec)
    n, m, N, bt, tv = sv.shape
    c = case(lqrx, BITS_SHAPE, prec, 21)
    a, b = c.run(), c.run()
    for k in OUT:
        assert same_bits(a[k], b[k]), k
    for outputs in (("d",), ("d", "p"), ("d", "X"), ("p",), OUT):
        r = c.run(outputs=outputs)
        assert set(r) == set(outputs) | {"rc"}
        for k in outputs:
            assert same_bits(r[k], a[k]), (outputs, k)
    p1 = c.run(outputs=("p",), p_mode=0)["p"]
    assert same_bits(p1.view(bt * 21, n), a["p"].view(bt * 21, N, n)[:, 0].contiguous())
    for k in RHS:
        nul, zero = c.run(**{k: None}), c.run(**{k: torch.zeros_like(c.rhs[k])})
        for o in OUT:
            assert same_bits(nul[o], zero[o]), (k, o)
        assert not all(same_bits(nul[o], a[o]) for o in OUT), k    # the field is read
    f2 = lqrx.dp_factor_device(sv.t, N, sv.sol["P"])
    assert same_bits(f2["Einv"], sv.fac["Einv"]) and same_bits(f2["Pc"], sv.fac["Pc"])


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(17, 5, 12, 3, True), (24, 18, 10, 3, False), (64, 32, 12, 2, False)], ids=sid)
def test_rollout_of_the_resolved_policy_has_its_bits(lqrx, gpu_ok, shape, prec):
    """S = 1: lqrx_dp_rollout of (K, the re-solve's own d) from the same x0, with no alpha, w or bounds, gives the
    bits of the re-solve's X and U: the two kernels compute one and the same forward pass.  α = 1 multiplies exactly,
    the clamp against ±∞ is the identity, c + 0 is c (the random c holds no −0), and the kernels' one-knot-ahead
    policies, which differ at fp64 2×2 tiles, do not reach the bits."""
    c = case(lqrx, shape, prec, 1)
    r = c.run(outputs=("d", "X", "U"))
    ro = lqrx.dp_rollout_device(c.sv.t, shape[2], c.sv.facd["K"], r["d"], dict(S=1, x0=c.rhs["x0"], outputs=("X", "U")))
    for k in ("X", "U"):
        assert same_bits(ro[k], r[k]), k


# ---- guard zones ----
def _filled(like, sizes):
    return {k: pattern_filled(like, sz) for k, sz in sizes.items()}


@pytest.mark.parametrize("shape,S", [(BITS_SHAPE, 21), ((24, 18, 10, 3, False), 5)], ids=["2x1-tv", "2x2"])
def test_extents_device(lqrx, gpu_ok, shape, S):
    """Both device entries on guarded buffers (inputs guarded as well): every output element written,
    no guard touched, and the bits of the run on plain tensors."""
    c = case(lqrx, shape, "f64", S)
    sv = c.sv
    n, m, N, bt, tv = shape
    hs = []
    tg = guard_all(sv.t, "in", bt, hs)
    Pg = guard_all(dict(P=sv.sol["P"]), "in", bt, hs)["P"]
    og = guard_all(dict(Einv=pattern_filled(sv.t["A"], bt * (N - 1) * m * m), Pc=pattern_filled(sv.t["A"], bt * (N - 1) * n),
                        info=pattern_filled(sv.sol["info"], bt)), "out", bt, hs)
    f = lqrx.dp_factor_device(tg, N, Pg, out=og)
    guard_check(hs)
    assert same_bits(f["Einv"], sv.fac["Einv"]) and same_bits(f["Pc"], sv.fac["Pc"])
    plain = c.run()
    for p_mode, outputs in ((1, OUT), (0, ("d", "p")), (1, ("d",)), (0, ("d", "X", "U")), (1, ("p",))):
        hs = []
        tg = guard_all(sv.t, "in", bt, hs)
        fg = guard_all(sv.facd, "in", bt, hs)
        rg = guard_all(c.rhs, "in", bt * S, hs)
        sizes = c.sizes(p_mode)
        og = guard_all(_filled(sv.t["A"], {k: sizes[k] for k in outputs}), "out", bt * S, hs)
        r = c.run(outputs=outputs, out=og, t=tg, fac=fg, p_mode=p_mode, **rg)
        guard_check(hs)
        assert set(r) == set(outputs) | {"rc"}
        for k in outputs:
            if k == "p" and p_mode == 0:
                assert same_bits(r[k].view(bt * S, n), plain[k].view(bt * S, N, n)[:, 0].contiguous())
            else:
                assert same_bits(r[k], plain[k]), (outputs, k)


def test_extents_host_entries(lqrx, gpu_ok):
    """lqrx_dp_factor_host and lqrx_dp_resolve_host on guarded host arrays: D2H of exactly the outputs
    asked for, every element written, no guard touched; the bits of the device entries."""
    from lqrx import _lib

    shape, S = BITS_SHAPE, 5
    n, m, N, bt, tv = shape
    c = case(lqrx, shape, "f64", S)
    sv = c.sv
    p = lambda a: None if a is None else a.ctypes.data
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    flat = lambda a: np.ascontiguousarray(a).reshape(-1)
    lib = lqrx.load()
    hs = []
    ins = {k: flat(sv.d[k]) for k in ("A", "B", "c", "R")}
    ins.update(P=flat(host(sv.sol["P"])))
    ig = guard_all(ins, "in", bt, hs)
    og = guard_all(dict(Einv=pattern_filled(ins["A"], bt * (N - 1) * m * m), Pc=pattern_filled(ins["A"], bt * (N - 1) * n),
                        info=pattern_filled(np.zeros(1, np.int32), bt)), "out", bt, hs)
    desc = _lib.DpDesc(n, m, N, _lib.F64, bt, 0, 1, int(tv), int(tv))
    rc = lib.lqrx_dp_factor_host(C.byref(desc), vp(ig["B"]), vp(ig["R"]), vp(ig["c"]), vp(ig["P"]), vp(og["Einv"]),
                                 vp(og["Pc"]), vp(og["info"]))
    assert rc == 0, lib.lqrx_last_error().decode()
    guard_check(hs)
    assert np.array_equal(og["Einv"].view(np.int64), sv.fac["Einv"].cpu().numpy().view(np.int64))
    assert np.array_equal(og["Pc"].view(np.int64), sv.fac["Pc"].cpu().numpy().view(np.int64))
    assert (og["info"] == 0).all()
    devr = c.run()
    sizes = c.sizes(1)
    for outputs in (OUT, ("d", "U")):
        hs = []
        ins = {k: flat(sv.d[k]) for k in ("A", "B", "c")}
        ins.update(K=flat(sv.K), Einv=flat(sv.Einv), Pc=flat(sv.Pc))
        ins.update({k: flat(v) for k, v in c.rhs_np.items()})
        ig = guard_all(ins, "in", bt, hs)
        og = guard_all(_filled(ins["A"], {k: sizes[k] for k in outputs}), "out", bt * S, hs)
        fac = _lib.DpFactors(p(ig["K"]), p(ig["Einv"]), p(ig["Pc"]))
        rhs = _lib.DpRhs(S, *[p(ig[k]) for k in RHS], *[p(og.get(k)) for k in OUT])
        rc = lib.lqrx_dp_resolve_host(C.byref(desc), vp(ig["A"]), vp(ig["B"]), vp(ig["c"]), C.byref(fac), C.byref(rhs))
        assert rc == 0, lib.lqrx_last_error().decode()
        guard_check(hs)
        for k in outputs:
            assert np.array_equal(og[k].view(np.int64), devr[k].cpu().numpy().view(np.int64)), (outputs, k)


def test_batch_wrappers_host_arrays(lqrx, gpu_ok):
    """lqrx.factor_batch and lqrx.resolve_batch on logical host arrays: the checker's result."""
    from dp_truth import to_batch
    from lqrx.dp import from_abi

    shape = (6, 3, 30, 7, False)
    n, m, N, bt, tv = shape
    c = case(lqrx, shape, "f64", 5)
    sv = c.sv
    b = to_batch(sv.d, N)
    f = lqrx.factor_batch(b, from_abi(host(sv.sol["P"]), (bt, N, n, n)))
    assert (f["info"] == 0).all()
    assert np.array_equal(f["Einv"], from_abi(sv.Einv, (bt, N - 1, m, m))) and np.array_equal(f["Pc"].ravel(), sv.Pc)
    sh = dict(q=(bt, 5, n), r=(bt, 5, m), qf=(bt, 5, n), x0=(bt, 5, n))
    r = lqrx.resolve_batch(b, from_abi(sv.K, (bt, N - 1, m, n)), f, all_p=True,
                           **{k: c.rhs_np[k].reshape(sh[k]) for k in RHS})
    e = dict(d=relerr_traj(r["d"].reshape(bt * 5, -1), c.ref["d"].reshape(bt * 5, -1)),
             p=relerr_traj(r["p"].reshape(bt * 5, -1), c.ref["p"].reshape(bt * 5, -1)),
             X=xu_error(r["X"], c.ref["X"]), U=xu_error(r["U"], c.ref["U"]))
    print("PARITY resolve_batch " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= TOL64
    r1 = lqrx.resolve_batch(b, from_abi(sv.K, (bt, N - 1, m, n)), f, outputs=("p",),
                            **{k: c.rhs_np[k].reshape(sh[k]) for k in RHS})
    assert set(r1) == {"p", "rc"} and np.array_equal(r1["p"], r["p"][:, :, 0])


def test_resolve_is_capturable(lqrx, gpu_ok):
    """The device entry takes no library scratch and never synchronises on a caller's stream: one
    call captured in a hipGraph on a side stream (tests/test_graph_gpu.py's procedure), replayed on a
    second set of right-hand sides, gives the bits of an eager call on them; the graph is one kernel node."""
    import torch

    from test_graph_gpu import _capture_and_replay

    sv = solved(lqrx, BITS_SHAPE, "f64")
    c = case(lqrx, BITS_SHAPE, "f64", 21)
    ins = {k: v.clone() for k, v in c.rhs.items()}
    second = Case(sv, 21, seed=12).rhs
    got, ref = _capture_and_replay(lambda s: c.run(stream=s, **ins), ins, second)
    for k in OUT:
        assert same_bits(got[k], ref[k]), k
    assert not same_bits(got["X"], c.run()["X"])     # the replay saw the second set
    # one kernel node: the call alone, captured into a graph that torch keeps
    g = torch.cuda.CUDAGraph(keep_graph=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        c.run(stream=side.cuda_stream, **ins)
    torch.cuda.current_stream().wait_stream(side)
    count, kinds = _graph_nodes(g)
    print(f"GRAPH resolve: {count} node(s), types {kinds}")
    assert count == 1 and kinds == [0]               # hipGraphNodeTypeKernel


def _graph_nodes(g):
    """(number of nodes, their hipGraphNodeType values) of a torch graph captured with keep_graph=True,
    through the HIP runtime this process has already loaded."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    raw = C.c_void_p(g.raw_cuda_graph())
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, C.byref(count)) == 0
    nodes = (C.c_void_p * max(1, count.value))()
    assert hip.hipGraphGetNodes(raw, nodes, C.byref(count)) == 0
    kinds = []
    for i in range(count.value):
        kind = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(kind)) == 0
        kinds.append(kind.value)
    return count.value, kinds
