"""GPU tests of the input-bounds entry (lqrx_dp_resolve_box[_host], include/lqrx.h).

K, E⁻¹, Pc come from lqrx_dp_solve_cross (p_mode 1) and lqrx_dp_factor on cross_problem (tests/dp_truth.py)
with R + ρI, ρ = 1.  At fixed iteration counts (eps = 0) the kernel is compared with the numpy checker
tests/dp_box_truth.py in float64 on the device's own K, E⁻¹, Pc (and, in fp32, on the fp32-rounded problem
and right-hand sides), so only the iteration's rounding is measured: d with dp_truth.relerr_traj, Z, W, X, U
and the residuals as max|a − b| / max(1, max|b|), against the project's TOL64 = 1e-10 and TOL32 = 1e-4.
Bounds sit at half the unconstrained peak control of each problem, the lower side of input 0 left open.
Every figure is printed before it is asserted.

Observed on an MI355X (profiles/r14/box/box_gpu_tests.log: the file's 60 cases in about 7 s): worst fp64 after 1, 7
and 30 iterations d 2.4e-14, Z 4.2e-14, W 1.5e-14, X 1.2e-14, U 2.5e-14, residuals 6.1e-13; fp32 d 4.3e-6, Z 9.8e-6,
W 3.7e-6, X 2.6e-6, U 6.4e-6, residuals 6.2e-5; at eps = 1e-9 the checker's iteration count in every instance
(53 – 451 and 92 – 250) and its natural residual, Z 1.8e-10 from the BVLS truth; one tile with instances that
stop after 1, 10 – 11, 41 – 42 iterations and never (max_iter = 60), each bit for bit the instance run alone; no
guard touched, no output element left unwritten, one kernel node in the captured graph.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from dp_box_truth import SHAPES, box_np, bvls_truth, half_peak_bounds, natural_residual
from dp_resolve_truth import F32_SHAPES, random_rhs, xu_error
from dp_truth import cross_problem, relerr_traj
from guarded import check as guard_check, guard_all, pattern_filled

pytestmark = pytest.mark.gpu

TOL64 = 1e-10
TOL32 = 1e-4
RHO, RELAX = 1.0, 1.6
S_ALL = (1, 5, 16, 21)
ITERS = (1, 7, 30)
PARITY = [(sh, S) for sh in SHAPES for S in S_ALL]
PARITY32 = [(sh, S) for sh in F32_SHAPES for S in S_ALL]
BITS_SHAPE = (17, 5, 12, 3, True)
PROBLEM = ("A", "B", "c", "Q", "R", "Qf", "M", "q", "r", "qf", "x0")
RHS = ("q", "r", "qf", "x0")
STATE = ("Z", "W", "d", "X", "U", "iters", "res")
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
    """A cross problem as the device sees it, its factors with R + ρI (what the box entry runs on) and with R
    (for the unconstrained controls that set the bounds), all from the device."""

    def __init__(self, lqrx, shape, prec):
        self.lqrx, self.shape, self.prec = lqrx, shape, prec
        n, m, N, bt, tv = shape
        self.npdt = np.float64 if prec == "f64" else np.float32
        self.tol = TOL64 if prec == "f64" else TOL32
        d = cross_problem(lqrx, n, m, N, bt, 3, tv_QR=tv, tv_AB=tv)
        for k in PROBLEM:
            d[k] = np.asarray(d[k], self.npdt).astype(np.float64)
        self.d = d
        self.t = {k: dev(d[k], self.npdt) for k in PROBLEM}
        self.t.update(n=n, m=m, batch=bt, tv_AB=int(tv), tv_QR=int(tv))
        Rr = d["R"].reshape(-1, m, m) + RHO * np.eye(m)
        self.facd, self.sol = self._factors(dict(self.t, R=dev(Rr, self.npdt)))
        self.facd0, self.sol0 = self._factors(self.t)
        self.K, self.Einv, self.Pc = (host(self.facd[k]) for k in ("K", "Einv", "Pc"))

    def _factors(self, t):
        N = self.shape[2]
        sol = self.lqrx.dp_solve_device(t, N, p_mode=1)
        assert (sol["info"] == 0).all().item()
        fac = self.lqrx.dp_factor_device(t, N, sol["P"])
        assert (fac["info"] == 0).all().item()
        return dict(K=sol["K"], Einv=fac["Einv"], Pc=fac["Pc"]), sol


@functools.lru_cache(maxsize=None)
def solved(lqrx, shape, prec="f64"):
    return Solved(lqrx, shape, prec)


class Case:
    """S instances per problem on a Solved: right-hand sides, bounds at half the unconstrained peak, and
    (lazily, chained: continuation is exact in the checker) the checker's state after 1, 7 and 30 iterations."""

    def __init__(self, sv, S, seed=11, rhs=None):
        self.sv, self.S = sv, S
        n, m, N, bt, tv = sv.shape
        rhs = random_rhs(n, m, N, bt, S, seed, tv) if rhs is None else rhs
        self.rhs_np = {k: np.asarray(v, sv.npdt).astype(np.float64) for k, v in rhs.items()}
        self.rhs = {k: dev(v, sv.npdt) for k, v in self.rhs_np.items()}
        self.U_unc = sv.lqrx.dp_resolve_device(sv.t, N, sv.facd0, dict(self.rhs, S=S, tv_QR=int(tv), outputs=("d", "U")))["U"]
        lo, hi = half_peak_bounds(host(self.U_unc), bt, m)
        self.lo_np, self.hi_np = (np.asarray(v, sv.npdt).astype(np.float64) for v in (lo, hi))
        self.lo, self.hi = dev(self.lo_np, sv.npdt), dev(self.hi_np, sv.npdt)
        self.size = bt * S * (N - 1) * m

    def zeros(self):
        import torch

        return torch.zeros(self.size, dtype=self.sv.t["A"].dtype, device="cuda:0")

    def np_run(self, max_iter, eps=0.0, Z=None, W=None, **kw):
        sv = self.sv
        args = dict(tv_QR=int(sv.shape[4]), u_lo=self.lo_np, u_hi=self.hi_np, rho=RHO, relax=RELAX, eps_prim=eps,
                    eps_dual=eps, max_iter=max_iter, Z=Z, W=W, **self.rhs_np)
        args.update(kw)
        return box_np(sv.d, sv.shape[2], sv.K, sv.Einv, sv.Pc, self.S, **args)

    @functools.cached_property
    def refs(self):
        out, prev, at = {}, None, 0
        for it in ITERS:
            prev = self.np_run(it - at, Z=None if prev is None else prev["Z"], W=None if prev is None else prev["W"])
            assert (prev["iters"] == it - at).all()          # eps = 0: nobody stops early
            out[it], at = dict(prev, iters=np.full_like(prev["iters"], it)), it
        return out

    def run(self, max_iter, eps=0.0, Z=None, W=None, outputs=("d", "X", "U"), box_out=("iters", "res"), out=None, t=None,
            fac=None, stream=None, relax=RELAX, bounds=True, **rhs):
        """the device entry; Z, W default to a cold start and are updated in place; rhs overrides / removes fields"""
        sv = self.sv
        r = dict(self.rhs, S=self.S, outputs=outputs, tv_QR=int(sv.shape[4]))
        r.update(rhs)
        box = dict(rho=RHO, relax=relax, eps_prim=eps, eps_dual=eps, max_iter=max_iter, outputs=box_out,
                   Z=self.zeros() if Z is None else Z, W=self.zeros() if W is None else W)
        if bounds is True:
            box.update(u_lo=self.lo, u_hi=self.hi)
        elif bounds:
            box.update(bounds)
        return sv.lqrx.dp_box_device(t or sv.t, sv.shape[2], fac or sv.facd, r, box, stream=stream, out=out)

    def check(self, r, ref, what):
        n, m, N, bt, _ = self.sv.shape
        flat = lambda a: np.asarray(a, np.float64).reshape(bt * self.S, -1)
        e = dict(d=relerr_traj(flat(host(r["d"])), flat(ref["d"])))
        e.update({k: xu_error(host(r[k]), ref[k].ravel()) for k in ("Z", "W", "X", "U", "res")})
        it = r["iters"].cpu().numpy()
        print(f"PARITY box {what} {self.sv.shape} S={self.S} {self.sv.prec}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items())
              + f" iters {it.min()} .. {it.max()}")
        assert np.array_equal(it, ref["iters"].ravel())
        for k, v in e.items():
            assert v <= self.sv.tol, (k, v)


@functools.lru_cache(maxsize=None)
def case(lqrx, shape, prec="f64", S=21):
    return Case(solved(lqrx, shape, prec), S)


# ---- parity at fixed iteration counts ----
def _parity(c):
    for it in ITERS:
        r = c.run(it)
        assert (r["iters"] == it).all().item()
        c.check(r, c.refs[it], f"{it} iterations")


@pytest.mark.parametrize("shape,S", PARITY, ids=[f"{sid(sh)}-S{S}" for sh, S in PARITY])
def test_parity_f64(lqrx, gpu_ok, shape, S):
    _parity(case(lqrx, shape, "f64", S))


@pytest.mark.parametrize("shape,S", PARITY32, ids=[f"{sid(sh)}-S{S}" for sh, S in PARITY32])
def test_parity_f32(lqrx, gpu_ok, shape, S):
    _parity(case(lqrx, shape, "f32", S))


def test_grid_of_many_tiles(lqrx, gpu_ok):
    """batch = 3, S = 1000: 63 tiles per problem, the last one partial"""
    c = case(lqrx, (6, 3, 5, 3, False), "f64", 1000)
    c.check(c.run(7), c.refs[7], "grid, 7 iterations")


# ---- convergence ----
@pytest.mark.parametrize("shape", [(6, 3, 30, 5, False), (32, 16, 40, 4, False)], ids=sid)
def test_convergence(lqrx, gpu_ok, shape):
    """eps = 1e-9: the iteration counts of the checker (one more or less in at most a tenth of the instances), a
    natural residual no worse than twice the checker's, Z inside the bounds exactly, and on (6, 3, 30) within 1e-8
    of the BVLS truth.  (6, 3, 30) runs the five plants of dp_box_truth.TRUTH_SHAPES: ρ = 1 does not finish the sixth.)"""
    n, m, N, bt, tv = shape
    S = 5
    c = case(lqrx, shape, "f64", S)
    r = c.run(1000, eps=1e-9)
    ref = c.np_run(1000, eps=1e-9)
    it, it_ref = r["iters"].cpu().numpy().reshape(bt, S), ref["iters"]
    Z = host(r["Z"]).reshape(bt, S, N - 1, m)
    nat, _ = natural_residual(c.sv.d, N, S, Z, c.lo_np, c.hi_np, tv_QR=int(tv), **c.rhs_np)
    nat_ref, _ = natural_residual(c.sv.d, N, S, ref["Z"], c.lo_np, c.hi_np, tv_QR=int(tv), **c.rhs_np)
    differ = (it != it_ref).mean()
    print(f"CONVERGENCE box {shape}: iters {it.min()} .. {it.max()} (checker {it_ref.min()} .. {it_ref.max()}), "
          f"{100 * differ:.0f} % differ, natural residual {nat.max():.2e} (checker {nat_ref.max():.2e}), "
          f"res {host(r['res']).max():.2e}")
    assert (it < 1000).all() and np.abs(it - it_ref).max() <= 1 and differ <= 0.10
    assert (nat <= 2 * nat_ref + 1e-12).all()
    assert ((Z >= c.lo_np[:, None, None]) & (Z <= c.hi_np[:, None, None])).all()
    if shape == (6, 3, 30, 5, False):
        truth = bvls_truth(c.sv.d, N, S, c.lo_np, c.hi_np, tv_QR=int(tv), **c.rhs_np)
        e = np.abs(Z - truth).max() / max(1.0, np.abs(truth).max())
        active = ((truth == c.lo_np[:, None, None]) | (truth == c.hi_np[:, None, None])).mean()
        print(f"CONVERGENCE box {shape}: |Z - truth| {e:.2e}, {100 * active:.1f} % of the entries active")
        assert 0.02 <= active <= 0.60 and e <= 1e-8


def test_inactive_bounds_warm_start_stops_at_once(lqrx, gpu_ok):
    """Bounds no control reaches, Z = the unconstrained U, W = 0: one iteration, and U is lqrx_dp_solve_cross's."""
    import torch

    sv = solved(lqrx, (6, 3, 30, 7, False), "f64")
    n, m, N, bt, tv = sv.shape
    own = {k: sv.d[k] for k in RHS}
    c = Case(sv, 1, rhs=own)
    U = sv.sol0["U"]
    wide = dict(u_lo=torch.full((bt * m,), -1e6, dtype=torch.float64, device="cuda:0"),
                u_hi=torch.full((bt * m,), 1e6, dtype=torch.float64, device="cuda:0"))
    r = c.run(50, eps=1e-9, Z=U.clone(), bounds=wide)
    e = xu_error(host(r["U"]), host(U))
    print(f"INACTIVE box: iters {r['iters'].cpu().numpy().tolist()} U against the cross solve {e:.2e} res {host(r['res']).max():.2e}")
    assert (r["iters"] == 1).all().item() and e <= TOL64


# ---- bit equality ----
MASK_ITER = 60


@functools.lru_cache(maxsize=None)
def masked(lqrx, prec):
    """S = 21 instances of different difficulty under one pair of bounds per problem: bounds just past the peak of
    the easy instances (right-hand sides scaled by 1 or less), so that those are unconstrained; some of them start
    at their own unconstrained U (they stop at once), some at it plus a small disturbance, some cold; the
    right-hand sides of the rest are scaled by 4 … 12, start cold and run into the bounds."""
    sv = solved(lqrx, BITS_SHAPE, prec)
    n, m, N, bt, tv = sv.shape
    S = 21
    scale = np.array([1, 8, 0.5, 1, 12, 1, 0.3, 4, 1, 1, 6, 0.7, 1, 10, 1, 5, 1, 9, 1, 0.2, 7], np.float64)
    kind = ["own", "cold", "near", "cold", "cold", "near", "own", "cold", "cold", "own", "cold", "near", "cold", "cold",
            "own", "cold", "own", "cold", "near", "cold", "cold"]
    rhs = random_rhs(n, m, N, bt, S, 17, tv)
    per = dict(q=(N - 1) * n, r=(N - 1) * m, qf=n, x0=n)
    rhs = {k: (v.reshape(bt, S, per[k]) * scale[None, :, None]).ravel() for k, v in rhs.items()}
    c = Case(sv, S, rhs=rhs)
    U = host(c.U_unc).reshape(bt, S, N - 1, m)
    easy = scale <= 1
    peak = np.abs(U[:, easy]).max(axis=(1, 2, 3))
    hi = np.repeat(1.05 * peak[:, None], m, axis=1)
    lo = -hi.copy()
    lo[:, 0] = -np.inf
    c.lo_np, c.hi_np = (np.asarray(v, sv.npdt).astype(np.float64) for v in (lo, hi))
    c.lo, c.hi = dev(c.lo_np, sv.npdt), dev(c.hi_np, sv.npdt)
    rng = np.random.default_rng(23)
    Z0 = np.zeros_like(U)
    for j, kd in enumerate(kind):
        assert kd == "cold" or easy[j]
        if kd != "cold":
            Z0[:, j] = U[:, j] + (1e-7 * rng.standard_normal(U[:, j].shape) if kd == "near" else 0.0)
    c.Z0 = dev(Z0, sv.npdt)
    c.kind = kind
    c.eps = 1e-9 if prec == "f64" else 1e-4
    c.full = c.run(MASK_ITER, eps=c.eps, Z=c.Z0.clone())
    return c


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_instances_stop_alone_and_bits_do_not_depend_on_the_neighbours(lqrx, gpu_ok, prec):
    """One tile holds instances that stop at iteration 1, in between, and never; each is, bit for bit, that
    instance alone (S = 1) and in another position of an S = 5 call."""
    c = masked(lqrx, prec)
    sv = c.sv
    n, m, N, bt, tv = sv.shape
    it = c.full["iters"].cpu().numpy().reshape(bt, 21)
    print(f"MASKING box {prec}: iters of problem 0 {it[0].tolist()} kinds {c.kind}")
    for b in range(bt):
        first = set(it[b, :16].tolist())
        assert len(first) >= 3 and 1 in first and MASK_ITER in first, (b, sorted(first))
    per = dict(q=(N - 1) * n, r=(N - 1) * m, qf=n, x0=n, d=(N - 1) * m, X=N * n, U=(N - 1) * m, Z=(N - 1) * m, W=(N - 1) * m,
               iters=1, res=2)
    view = lambda x, k, S: x.view(bt, S, per[k])
    pick = lambda x, k, js: view(x, k, 21)[:, list(js)].contiguous().view(-1)
    c1, c5 = Case(sv, 1), Case(sv, 5)
    for cc in (c1, c5):
        cc.lo, cc.hi = c.lo, c.hi
    for j in (0, 1, 2, 3, 15, 16, 20):
        one = c1.run(MASK_ITER, eps=c.eps, Z=pick(c.Z0, "Z", [j]), **{k: pick(c.rhs[k], k, [j]) for k in RHS})
        for k in STATE:
            assert same_bits(pick(c.full[k], k, [j]), one[k]), (k, j)
    js = (20, 0, 16, 1, 2)   # positions 0 … 4 of the S = 5 call
    five = c5.run(MASK_ITER, eps=c.eps, Z=pick(c.Z0, "Z", js), **{k: pick(c.rhs[k], k, js) for k in RHS})
    for k in STATE:
        assert same_bits(pick(c.full[k], k, js), five[k]), k


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bits_of_subsets_defaults_and_reruns(lqrx, gpu_ok, prec):
    """Two runs, the optional outputs asked for or not, NULL bounds against ±inf arrays, NULL against zero-filled
    q, r, qf, x0."""
    import torch

    c = masked(lqrx, prec)
    a = c.full
    b = c.run(MASK_ITER, eps=c.eps, Z=c.Z0.clone())
    for k in STATE:
        assert same_bits(a[k], b[k]), k
    for outputs, box_out in ((("d",), ()), (("d", "X"), ("iters",)), (("d", "U"), ("res",)), (("d",), ("iters", "res"))):
        r = c.run(MASK_ITER, eps=c.eps, Z=c.Z0.clone(), outputs=outputs, box_out=box_out)
        assert set(r) == set(outputs) | set(box_out) | {"Z", "W", "rc"}
        for k in outputs + box_out + ("Z", "W"):
            assert same_bits(r[k], a[k]), (outputs, box_out, k)
    inf = torch.full_like(c.lo, float("inf"))
    for nul, arr in ((dict(u_hi=c.hi), dict(u_lo=-inf, u_hi=c.hi)), (dict(u_lo=c.lo), dict(u_lo=c.lo, u_hi=inf)),
                     ({}, dict(u_lo=-inf, u_hi=inf))):
        rn, ra = (c.run(30, Z=c.Z0.clone(), bounds=bd or None) for bd in (nul, arr))
        for k in STATE:
            assert same_bits(rn[k], ra[k]), (sorted(nul), k)
        assert not all(same_bits(rn[k], c.run(30, Z=c.Z0.clone())[k]) for k in ("Z", "W"))    # the bound is read
    for k in RHS:
        nul, zero = c.run(7, **{k: None}), c.run(7, **{k: torch.zeros_like(c.rhs[k])})
        for o in STATE:
            assert same_bits(nul[o], zero[o]), (k, o)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_continuation_is_exact(lqrx, gpu_ok, prec):
    """eps = 0: 7 iterations, then 23 on the returned Z, W, are the bits of 30."""
    c = case(lqrx, BITS_SHAPE, prec, 21)
    a = c.run(7)
    ab = c.run(23, Z=a["Z"], W=a["W"])
    full = c.run(30)
    assert (a["iters"] == 7).all().item() and (ab["iters"] == 23).all().item() and (full["iters"] == 30).all().item()
    for k in ("Z", "W", "d", "X", "U", "res"):
        assert same_bits(ab[k], full[k]), k


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(17, 5, 12, 3, True), (24, 18, 10, 3, False), (64, 32, 12, 2, False)], ids=sid)
def test_first_cold_iteration_has_the_bits_of_the_resolve(lqrx, gpu_ok, shape, prec):
    """Z = W = 0, max_iter = 1, eps = 0: r̂ = r − ρ·0 is r exactly, so d, X and U are the bits of lqrx_dp_resolve on
    the same factors and right-hand sides: the two kernels compute one and the same pair of passes."""
    c = case(lqrx, shape, prec, 21)
    r = c.run(1)
    ref = lqrx.dp_resolve_device(c.sv.t, shape[2], c.sv.facd,
                                 dict(c.rhs, S=21, tv_QR=int(shape[4]), outputs=("d", "X", "U")))
    assert (r["iters"] == 1).all().item()
    for k in ("d", "X", "U"):
        assert same_bits(r[k], ref[k]), k


# ---- guard zones ----
def _filled(like, sizes):
    return {k: pattern_filled(like, sz) for k, sz in sizes.items()}


@pytest.mark.parametrize("shape,S", [(BITS_SHAPE, 21), ((24, 18, 10, 3, False), 5)], ids=["2x1-tv", "2x2"])
def test_extents_device(lqrx, gpu_ok, shape, S):
    """The device entry on guarded buffers, Z and W included: every output element written, no guard touched, and
    the bits of the run on plain tensors."""
    import torch

    c = case(lqrx, shape, "f64", S)
    sv = c.sv
    n, m, N, bt, tv = shape
    plain = c.run(7)
    sizes = dict(d=c.size, X=bt * S * N * n, U=c.size, res=2 * bt * S)
    for outputs, box_out in ((("d", "X", "U"), ("iters", "res")), (("d",), ()), (("d", "U"), ("iters",))):
        hs = []
        tg = guard_all(sv.t, "in", bt, hs)
        fg = guard_all(sv.facd, "in", bt, hs)
        rg = guard_all(c.rhs, "in", bt * S, hs)
        bg = guard_all(dict(u_lo=c.lo, u_hi=c.hi), "in", bt, hs)
        zw = guard_all(dict(Z=c.zeros(), W=c.zeros()), "inout", bt * S, hs)
        og = guard_all(_filled(sv.t["A"], {k: sizes[k] for k in outputs + box_out if k != "iters"}), "out", bt * S, hs)
        if "iters" in box_out:
            og.update(guard_all(dict(iters=pattern_filled(torch.zeros(1, dtype=torch.int32, device="cuda:0"), bt * S)), "out",
                                bt * S, hs))
        r = c.run(7, outputs=outputs, box_out=box_out, out=og, t=tg, fac=fg, Z=zw["Z"], W=zw["W"], bounds=bg, **rg)
        guard_check(hs)
        for k in outputs + box_out + ("Z", "W"):
            assert same_bits(r[k], plain[k]), (outputs, box_out, k)


def test_extents_host_entry_and_its_bits(lqrx, gpu_ok):
    """lqrx_dp_resolve_box_host on guarded host arrays: Z and W copied in and out, D2H of exactly the outputs asked
    for, every element written, no guard touched; the bits of the device entry (warm start included)."""
    from lqrx import _lib

    shape, S = BITS_SHAPE, 5
    n, m, N, bt, tv = shape
    c = case(lqrx, shape, "f64", S)
    sv = c.sv
    p = lambda a: None if a is None else a.ctypes.data
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    flat = lambda a: np.ascontiguousarray(a).reshape(-1)
    lib = lqrx.load()
    first = c.run(7)
    devr = c.run(23, Z=first["Z"].clone(), W=first["W"].clone())
    desc = _lib.DpDesc(n, m, N, _lib.F64, bt, 0, 0, int(tv), int(tv))
    sizes = dict(d=c.size, X=bt * S * N * n, U=c.size, res=2 * bt * S)
    for outputs in (("d", "X", "U", "iters", "res"), ("d", "res")):
        hs = []
        ins = {k: flat(sv.d[k]) for k in ("A", "B", "c")}
        ins.update(K=flat(sv.K), Einv=flat(sv.Einv), Pc=flat(sv.Pc), u_lo=flat(c.lo_np), u_hi=flat(c.hi_np))
        ins.update({k: flat(v) for k, v in c.rhs_np.items()})
        ig = guard_all(ins, "in", bt, hs)
        zw = guard_all(dict(Z=first["Z"].cpu().numpy(), W=first["W"].cpu().numpy()), "inout", bt * S, hs)
        og = guard_all(_filled(ins["A"], {k: sizes[k] for k in outputs if k != "iters"}), "out", bt * S, hs)
        if "iters" in outputs:
            og.update(guard_all(dict(iters=pattern_filled(np.zeros(1, np.int32), bt * S)), "out", bt * S, hs))
        fac = _lib.DpFactors(p(ig["K"]), p(ig["Einv"]), p(ig["Pc"]))
        rhs = _lib.DpRhs(S, *[p(ig[k]) for k in RHS], p(og["d"]), None, p(og.get("X")), p(og.get("U")))
        box = _lib.DpBox(RHO, RELAX, 0.0, 0.0, 23, p(ig["u_lo"]), p(ig["u_hi"]), p(zw["Z"]), p(zw["W"]), p(og.get("iters")),
                         p(og.get("res")))
        rc = lib.lqrx_dp_resolve_box_host(C.byref(desc), vp(ig["A"]), vp(ig["B"]), vp(ig["c"]), C.byref(fac), C.byref(rhs),
                                          C.byref(box))
        assert rc == 0, lib.lqrx_last_error().decode()
        guard_check(hs)
        got = dict(og, Z=zw["Z"], W=zw["W"])
        for k in outputs + ("Z", "W"):
            iv = np.int32 if k == "iters" else np.int64
            assert np.array_equal(got[k].view(iv), devr[k].cpu().numpy().view(iv)), (outputs, k)


def test_box_batch_against_the_truth(lqrx, gpu_ok):
    """lqrx.box_batch end to end on logical host arrays (the solve with R + ρI, the factor, the iteration) on
    (6, 3, 30): within 1e-8 of the BVLS truth, Z inside the bounds, Y = ρW signed like the active side."""
    from dp_truth import to_batch

    shape, S = (6, 3, 30, 5, False), 5
    n, m, N, bt, tv = shape
    c = case(lqrx, shape, "f64", S)
    b = to_batch(c.sv.d, N)
    sh = dict(q=(bt, S, n), r=(bt, S, m), qf=(bt, S, n), x0=(bt, S, n))
    r = lqrx.box_batch(b, c.lo_np, c.hi_np, rho=RHO, relax=RELAX, eps=(1e-10, 1e-10), max_iter=2000,
                       **{k: c.rhs_np[k].reshape(sh[k]) for k in RHS})
    truth = bvls_truth(c.sv.d, N, S, c.lo_np, c.hi_np, tv_QR=int(tv), **c.rhs_np)
    e = np.abs(r["Z"] - truth).max() / max(1.0, np.abs(truth).max())
    lo, hi = c.lo_np[:, None, None], c.hi_np[:, None, None]
    print(f"BOX_BATCH {shape}: iters {r['iters'].min()} .. {r['iters'].max()} |Z - truth| {e:.2e} res {r['res'].max():.2e}")
    assert r["rc"] == 0 and (r["info"] == 0).all() and (r["iters"] < 2000).all()
    assert r["X"].shape == (bt, S, N, n) and r["U"].shape == r["Z"].shape == r["Y"].shape == (bt, S, N - 1, m)
    assert ((r["Z"] >= lo) & (r["Z"] <= hi)).all() and e <= 1e-8
    assert (r["Y"][r["Z"] == hi] >= -1e-9).all() and (r["Y"][r["Z"] == lo] <= 1e-9).all()
    assert np.array_equal(r["Y"], RHO * r["W"])


# ---- graph capture ----
def test_box_is_capturable(lqrx, gpu_ok):
    """The device entry takes no library scratch and never synchronises on a caller's stream: one call captured
    on a side stream, replayed on a second set of right-hand sides (from the same start), gives the bits of an
    eager call on them; the graph is one kernel node."""
    import torch

    from test_dp_resolve_gpu import _graph_nodes
    from test_graph_gpu import _capture_and_replay

    sv = solved(lqrx, BITS_SHAPE, "f64")
    c = case(lqrx, BITS_SHAPE, "f64", 21)
    ins = {k: v.clone() for k, v in c.rhs.items()}
    ins.update(Z=c.zeros(), W=c.zeros())
    second = dict(Case(sv, 21, seed=12).rhs, Z=c.zeros(), W=c.zeros())

    def call(s):
        for k in ("Z", "W"):          # every call starts cold: the in/out state is reset outside the library's kernel
            ins[k].zero_()
        return c.run(7, stream=s, Z=ins["Z"], W=ins["W"], **{k: ins[k] for k in RHS})

    got, ref = _capture_and_replay(call, ins, second)
    for k in STATE:
        assert same_bits(got[k], ref[k]), k
    assert not same_bits(got["Z"], c.run(7)["Z"])     # the replay saw the second set
    g = torch.cuda.CUDAGraph(keep_graph=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    Z, W = c.zeros(), c.zeros()
    with torch.cuda.graph(g, stream=side):
        c.run(7, stream=side.cuda_stream, Z=Z, W=W)
    torch.cuda.current_stream().wait_stream(side)
    count, kinds = _graph_nodes(g)
    print(f"GRAPH box: {count} node(s), types {kinds}")
    assert count == 1 and kinds == [0]               # hipGraphNodeTypeKernel


# ---- argument errors, on device pointers ----
def test_argument_errors_name_the_member(lqrx, gpu_ok):
    from lqrx import _lib

    c = case(lqrx, BITS_SHAPE, "f64", 5)
    sv = c.sv
    n, m, N, bt, tv = sv.shape
    lib = lqrx.load()
    Z, W, d = c.zeros(), c.zeros(), c.zeros()
    p = lambda x: None if x is None else x.data_ptr()

    def call(desc=True, A=sv.t["A"], B=sv.t["B"], fac=True, rhs=True, box=True, fkw={}, rkw={}, bkw={}, dkw={}):
        de = _lib.DpDesc(**{**dict(n=n, m=m, N=N, dtype=_lib.F64, batch=bt, layout=0, p_mode=0, knot_stride_AB=int(tv),
                                   knot_stride_QR=int(tv)), **dkw})
        fc = _lib.DpFactors(**{**{k: p(sv.facd[k]) for k in ("K", "Einv", "Pc")}, **fkw})
        rs = _lib.DpRhs(**{**dict(S=5, d=p(d), p=None, X=None, U=None, **{k: p(c.rhs[k]) for k in RHS}), **rkw})
        bx = _lib.DpBox(**{**dict(rho=RHO, relax=RELAX, eps_prim=0.0, eps_dual=0.0, max_iter=3, u_lo=p(c.lo), u_hi=p(c.hi),
                                  Z=p(Z), W=p(W), iters=None, res=None), **bkw})
        vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        rc = lib.lqrx_dp_resolve_box(C.byref(de) if desc else None, vp(A), vp(B), vp(sv.t["c"]), C.byref(fc) if fac else None,
                                     C.byref(rs) if rhs else None, C.byref(bx) if box else None, None)
        return rc, lib.lqrx_last_error().decode()

    assert call()[0] == 0
    assert call(desc=False)[0] == -1
    for kw, code, text in ((dict(A=None), -2, "A"), (dict(B=None), -3, "B"), (dict(fac=False), -5, "fac"),
                           (dict(fkw=dict(Einv=None)), -5, "fac->Einv"), (dict(rhs=False), -6, "rhs"),
                           (dict(rkw=dict(d=None)), -6, "rhs->d"), (dict(rkw=dict(p=p(d))), -6, "rhs->p"),
                           (dict(box=False), -7, "box"), (dict(bkw=dict(rho=0.0)), -7, "box->rho"),
                           (dict(bkw=dict(relax=2.0)), -7, "box->relax"), (dict(bkw=dict(eps_dual=-1.0)), -7, "box->eps_dual"),
                           (dict(bkw=dict(max_iter=0)), -7, "box->max_iter"), (dict(bkw=dict(Z=None)), -7, "box->Z"),
                           (dict(bkw=dict(W=None)), -7, "box->W")):
        rc, msg = call(**kw)
        assert rc == code and text in msg, (kw, rc, msg)
    assert call(dkw=dict(layout=1))[0] == _lib.ERR_UNSUPPORTED
