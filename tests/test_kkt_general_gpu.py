"""GPU parity of every KKT kernel family on general inputs: Y = [D2; C; D1] with every row random
(tests/kkt_general.py: D2 unsymmetric with non-zero input columns, boundary stage rows no identity
rows) and per-knot structures in which n1, p, n2 and w all change from knot to knot — what
include/lqrx.h promises and lqrx.kkt.random_kkt, the generator of every other KKT test, never builds.
All through lqrx.kkt.kkt_solve, the host entry, against the C oracle (oracle/lqr_oracle.c).

Tolerances: fp64 dz and lam within 1e-10 of the oracle, fp32 within 1e-4 of the fp64 oracle on the
fp32-rounded inputs; relative per trajectory (tests/test_kkt_big_gpu.py's traj_rel), table A on the
batch's scale (tests/test_kkt_gpu.py's rel).  No refined-truth fallback: tests/test_kkt_general.py holds
the oracle within 1e-11 of the truth on exactly these inputs.

Tables (tests/kkt_general.py CASES; modes are (h_mode, ginv) in (2,1), (0,1), (1,1), (2,0), table C
without (1,1)):
  A  general Y on the uniform structures of the compile-time kernels (Dubins N = 4 and 101, cartpole
     N = 7 and 101, DoubleIntegrator(3) N = 6, DoubleIntegrator(2) N = 12, (5,2), (7,3), (6,2), (8,4) at
     N = 9) and of the padded bins ((3,1) N = 12, (5,1) N = 9, (7,2) N = 6 with one stage row at knots
     1..4 and no goal rows: with a goal block it has 53 rows for 52 variables).  Layout 1 gives layout 0's
     bits on the natively-SoA shapes (Dubins, cartpole with a diagonal H) and on a staged one ((5,1)).
  B  irregular structures on the run-time-shaped small kernels, one per class of kkt_generic_class,
     real (max part, max w, max rows) = class 1 (3, 5, 6) launch_staged<3,3,3,5,6>, class 2 (4, 7, 8)
     launch_lane<4,4,4,8,8>, class 3 (8, 10, 15) launch_lane<8,8,8,12,16>: class 3 goes to the
     large-block kernels by default and to its lane kernel under LQRX_KKT_FORCE_LANE=1 (a child).
  C  the large-block family, fp64: (i) stage rows at interior knots and parts in different 16-bins (three
     parts at knot 2: the unsplit kkt_big_fwd/bwd_kernel); (ii) state widths 32,32,32,20,32,32,32, p = 0
     inside: the fused run is knots 1..5, starts on a full knot and holds a ragged one; (iii) widths
     24,17,30,32,20,31,18,25, one bin, the run's first knot ragged; (iv) 16,16,40,36,40,44,40,16,16: the
     run is knots 2..5, strictly inside the horizon, head and tail on kb_factor_kernel; (v) is (ii) with
     the input widths changing per knot.
  D  the workgroup kernel: parts up to 72 rows, one stage block of 70, w up to 132.
  E  fp32: (iii), a stage-row structure of the large-block kernels, and a workgroup structure.
  F  info on an irregular structure, on each class of table B (staged, lane, and class 3's default
     large-block route) and on C-i: a negated dense H_k at an interior knot whose offset is no multiple
     of a uniform stride gives info = −(k+1) as the oracle does, neighbours untouched.
  G  guard zones (tests/guarded.py) on C-ii and D-wg, through lqrx_kkt_solve and lqrx_kkt_solve_ws.

Child processes (the library reads its routing switches once): LQRX_KKT_FUSE=0, LQRX_KKT_MID=0,
LQRX_KKT_SPLIT=0 and LQRX_KKT_WG=1 each solve table C, LQRX_KKT_BIG=1 solves tables A and B on the
large-block kernels, LQRX_KKT_FORCE_LANE=1 solves B-class3.  Every child meets the oracle as the
parent does and is within 1e-10 of the parent.  Which switch changes the bits follows from kb_plan
(lqrx_kkt_big.hip): C-i has three non-empty parts at knot 2, so it is not split and FUSE, MID and SPLIT
leave its launches, and therefore its bits, unchanged; C-ii .. C-v are split with a fused interior run
(mid1 < N), so FUSE=0 (kb_factor_mid_kernel on Schur images), MID=0 (kb_factor_kernel over every knot)
and SPLIT=0 (kkt_big_fwd_kernel) each take another path and must NOT give the parent's bits — the
evidence that the switched path ran.  B-class3 under BIG=1 is the parent's route (same bits), under
FORCE_LANE=1 another kernel (other bits).  WG=1 on table C and BIG=1 on table A and B-class1/2 run
another family than the parent's and must not give its bits either — except (8,4) with a dense or
block-diagonal H, which kkt_route sends to the large-block kernels by default (w = 12 > FILH_WM, class 3):
BIG=1 is the parent's route there and gives its bits.

The defect these inputs found: kb_plan set midfull — kb_fuse_mid_kernel<T, NT, true>, whose fu_schur2
reads whole 16-row blocks and D1 at row 16·NT at EVERY knot of the run — from the run's first knot
alone.  On C-ii and C-v (n2 of knot 1 is 32, knots 2 and 3 have 20-row parts) that read D1 rows as D2
rows.  midfull now needs n1 = n2 = 16·NT at every knot of the run; uniform structures plan as before.

Observed on an MI355X (230 cases, 17 s wall; a case with a child's first use 2.2–2.6 s, every other under
0.2 s), worst of dz, lam against the oracle per family:
  default routing   A 1.8e-12 ((5,1) N = 9, dense H; the oracle is itself 1.8e-12 from the truth there),
                    B 2.3e-13, C-i 3.8e-14, C-ii 6.8e-14, C-iii 4.3e-14, C-iv 4.7e-14, C-v 8.8e-14,
                    D 4.2e-13 (dense H), fp32 E-iii 1.4e-5, E-stage 9.3e-6, E-wg 7.6e-6
  children          FUSE=0 and MID=0 9.2e-14, SPLIT=0 4.1e-14, WG=1 5.5e-14 (all on table C),
                    BIG=1 3.0e-12 on A (cartpole N = 7, dense H) and 2.0e-13 on B, FORCE_LANE=1 1.7e-13
  info cases        neighbours 2.3e-13 (B-class1), 3.0e-14 (B-class2), 1.2e-13 (B-class3), 3.8e-14 (C-i);
                    guard runs, both entries, 4.7e-14 (C-ii), 8.3e-14 (D-wg), no guard touched.
The bits changed exactly where kb_plan says: FUSE=0, MID=0 and SPLIT=0 changed them on every run of
C-ii .. C-v and on none of C-i; FORCE_LANE=1 changed B-class3's, BIG=1 did not; WG=1 changed every run
of table C and BIG=1 every run of A and B-class1/2 but the two of (8,4) that are its route anyway.
Before the midfull fix, default routing on C-ii and C-v (every other case passed, and the four table-C
children were 1e-14 from the oracle on both): (2,1) and (2,0) returned rc = 1 with info ≠ 0 on
well-posed problems, and (0,1) returned info = 0 with dz 1.19e+01 and lam 3.7e+00 (C-ii), dz 1.19e+01 and
lam 1.6e+00 (C-v) from the oracle.  After it: C-ii 6.8e-14, C-v 8.8e-14.
"""
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), os.path.join(os.path.dirname(_HERE), "lqr.jl_amd"), _HERE):   # (a child has no conftest)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import kkt_general as G  # noqa: E402

pytestmark = pytest.mark.gpu

TOL, F32_TOL = 1e-10, 1e-4
ID = lambda r: f"{r[0]}-h{r[1]}-g{r[2]}"
# child → (environment, runs it solves)
CHILDREN = {
    "fuse0": ({"LQRX_KKT_FUSE": "0"}, G.runs("C")),
    "mid0": ({"LQRX_KKT_MID": "0"}, G.runs("C")),
    "split0": ({"LQRX_KKT_SPLIT": "0"}, G.runs("C")),
    "wg": ({"LQRX_KKT_WG": "1"}, G.runs("C")),
    "big": ({"LQRX_KKT_BIG": "1"}, G.runs("AB")),
    "lane": ({"LQRX_KKT_FORCE_LANE": "1"}, [r for r in G.runs("B") if r[0] == "B-class3"]),
}
PLAN_SWITCHES = ("fuse0", "mid0", "split0")
# (8,4) with a dense or block-diagonal H: w = 12 is past the dense-H passes of the compile-time kernels
# (FILH_WM = 10) and the structure is class 3, so kkt_route sends it to the large-block kernels by default
PARENT_IS_BIG = (("A-t84-N9", 0, 1), ("A-t84-N9", 1, 1))


def solve(run, layout=0):
    import lqrx
    import lqrx.kkt as K

    cid, hm, gi = run
    dt = lqrx.F32 if G.CASES[cid].prec == "f32" else lqrx.F64
    return K.kkt_solve(G.problem(cid, hm), ginv=gi, layout=layout, dtype=dt)


if __name__ == "__main__":          # a child: its runs under the switch of its environment, dumped to argv[2]
    env, todo = CHILDREN[sys.argv[1]]
    assert all(os.environ.get(k) == v for k, v in env.items())
    import lqrx as L

    L.load()
    np.savez(sys.argv[2], **{f"{ID(r)}/{k}": np.asarray(v) for r in todo for k, v in solve(r).items()})
    sys.exit(0)


@functools.lru_cache(maxsize=None)
def parent(run):
    """The default-routing solve of a run in this process; computed once, never modified."""
    return solve(run)


_children = {}


@pytest.fixture
def child(lqrx, gpu_ok, tmp_path_factory):
    """name → the child's results.  A child starts at most once per session: one that failed or ran into
    its time limit is recorded as such, and every later case of that switch fails from the record."""
    def run_once(name):
        env, todo = CHILDREN[name]
        path = str(tmp_path_factory.mktemp("kktgen") / f"{name}.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name, path], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.returncode, r.stdout + r.stderr)
        z = np.load(path)
        return {ID(t): {k: z[f"{ID(t)}/{k}"] for k in ("dz", "lam", "info", "rc")} for t in todo}

    def get(name):
        if name not in _children:
            try:
                _children[name] = run_once(name)
            except Exception as e:              # (AssertionError, subprocess.TimeoutExpired, a missing dump)
                _children[name] = e
        if isinstance(_children[name], Exception):
            raise _children[name]
        return _children[name]
    return get


def _err(cid, got, ref):
    f = G.batch_rel if G.CASES[cid].rel == "batch" else G.traj_rel
    return {k: f(got[k], np.asarray(ref[k], np.float64)) for k in ("dz", "lam")}


def _check(run, got, what):
    cid, hm, gi = run
    ref = G.oracle_solve(cid, hm, gi)
    assert int(got["rc"]) == 0 and (got["info"] == 0).all() and (ref["info"] == 0).all()
    assert np.isfinite(got["dz"]).all() and np.isfinite(got["lam"]).all()
    e = _err(cid, got, ref)
    print(f"PARITY kktgen {what} {ID(run)} worst {max(e.values()):.2e} : dz {e['dz']:.2e} lam {e['lam']:.2e}")
    assert max(e.values()) <= (F32_TOL if G.CASES[cid].prec == "f32" else TOL), e


def _same_bits(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in ("dz", "lam"))


@pytest.mark.parametrize("run", G.runs(), ids=ID)
def test_parity(lqrx, gpu_ok, run):
    got = parent(run)
    if G.CASES[run[0]].prec == "f32":
        assert got["dz"].dtype == np.float32 and got["lam"].dtype == np.float32
    _check(run, got, "default")


LAYOUT1 = [("A-dubins-N4", hm, gi) for hm, gi in G.MODES4] + [("A-cartpole-N7", 2, 1), ("A-cartpole-N7", 2, 0),
                                                               ("A-pad51-N9", 2, 1)]


@pytest.mark.parametrize("run", LAYOUT1, ids=ID)
def test_layout1_gives_layout0_bits(lqrx, gpu_ok, run):
    got = solve(run, layout=1)
    assert got["rc"] == 0 and _same_bits(got, parent(run))


@pytest.mark.parametrize("name,run", [(n, r) for n, (_, rs) in CHILDREN.items() for r in rs],
                         ids=lambda v: v if isinstance(v, str) else ID(v))
def test_switched_route(lqrx, gpu_ok, child, name, run):
    got, par = child(name)[ID(run)], parent(run)
    _check(run, got, name)
    e = _err(run[0], got, par)
    assert max(e.values()) <= TOL, e
    if name in PLAN_SWITCHES:
        assert _same_bits(got, par) == (run[0] == "C-i"), (name, ID(run))
    if run[0] == "B-class3":
        assert _same_bits(got, par) == (name == "big"), (name, ID(run))
    elif run in PARENT_IS_BIG:
        assert _same_bits(got, par), (name, ID(run))
    elif name in ("wg", "big"):             # another family than the parent's: it did run on these inputs
        assert not _same_bits(got, par), (name, ID(run))


@pytest.mark.parametrize("cid,knot", [("B-class1", 4), ("B-class2", 4), ("B-class3", 4), ("C-i", 3)])
def test_info_on_an_irregular_structure(lqrx, gpu_ok, cid, knot):
    import lqrx.kkt as K

    pb0 = G.problem(cid, 0)
    w = pb0.st.w.astype(int)
    o = int(np.sum(w[:knot] ** 2))
    assert all(o != knot * s * s for s in set(w.tolist())) and 0 < knot < pb0.st.N - 1
    bad, H = 1, pb0.H.copy()
    H[bad, o:o + w[knot] ** 2] *= -1.0
    pb = dataclasses.replace(pb0, H=H)
    ref = G.reference(pb, 1)
    got = K.kkt_solve(pb)
    assert ref["info"][bad] == -(knot + 1) and got["rc"] == 1
    assert list(got["info"]) == list(ref["info"]) and (np.delete(got["info"], bad) == 0).all()
    ok = [t for t in range(pb.batch) if t != bad]
    e = max(G.traj_rel(got[k][ok], ref[k][ok]) for k in ("dz", "lam"))
    print(f"PARITY kktgen info {cid} neighbours {e:.2e}")
    assert e <= TOL
    assert _same_bits({k: got[k][ok] for k in ("dz", "lam")}, {k: parent((cid, 0, 1))[k][ok] for k in ("dz", "lam")})


@pytest.mark.parametrize("entry", ["solve", "solve_ws"])
@pytest.mark.parametrize("run", [("C-ii", 2, 1), ("D-wg", 2, 1)], ids=ID)
def test_guard_zones(lqrx, gpu_ok, run, entry):
    """As tests/test_guard_kkt_gpu.py, both entries (solve_ws with a guarded workspace of exactly the reported
    size): the guards stay intact, every output element is written, and the guarded run gives the plain
    run's bits, which meet the oracle."""
    import torch
    import lqrx.kkt as K
    from guarded import check as guard_check, guard_all, guard_bytes, guarded, pattern_filled

    cid, hm, gi = run
    pb = G.problem(cid, hm)
    st, bt = pb.st, pb.batch
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(pb, k)).reshape(-1)).to("cuda:0") for k in ("Y", "y", "H", "g")}
    t["batch"] = bt
    sY, sy, sH, sg = st.sizes(hm)
    sizes = dict(dz=bt * sg, lam=bt * sy, info=bt)
    like_i = torch.empty(1, dtype=torch.int32, device="cuda:0")
    outs = lambda: {k: pattern_filled(like_i if k == "info" else t["Y"], sz) for k, sz in sizes.items()}
    plain = K.kkt_solve_device(st, t, hm, ginv=gi, out=outs())
    torch.cuda.synchronize()
    hs, ws = [], None
    if entry == "solve_ws":
        nb = K.workspace_size(st, bt, hm, gi, 0, lqrx.F64)
        ws, h = guarded(torch.empty(nb, dtype=torch.uint8, device="cuda:0"), "ws", guard_bytes(nb, bt), "workspace")
        assert ws.numel() == nb
        hs.append(h)
    got = K.kkt_solve_device(st, guard_all(t, "in", bt, hs), hm, ginv=gi, out=guard_all(outs(), "out", bt, hs),
                             workspace=ws)
    assert plain["rc"] == 0 and got["rc"] == 0
    guard_check(hs)
    host = {k: plain[k].cpu().numpy().reshape(bt, -1) for k in ("dz", "lam")}
    assert all(torch.equal(got[k], plain[k]) for k in sizes) and (plain["info"] == 0).all().item()
    _check(run, dict(host, rc=plain["rc"], info=plain["info"].cpu().numpy()), "guard")
