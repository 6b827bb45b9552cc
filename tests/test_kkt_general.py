"""CPU checks of the general KKT inputs (tests/kkt_general.py) that tests/test_kkt_general_gpu.py
runs on the kernels: no GPU, the library is not loaded.

  * Oracle bound.  For every run of the tables — case × (h_mode, ginv), on the inputs rounded to the
    case's precision — the C oracle's dz and lam are within 1e-11 of tests/kkt_truth.py's refined truth
    (the full KKT system, five refinements with longdouble residuals), relative per trajectory.  1e-11
    is a tenth of the GPU file's tolerance (the rule of tests/test_dp_ns_regimes_gpu.py), which is why
    that file holds every trajectory to a flat 1e-10 against the oracle with no fallback.
  * Generator guard.  The generator has not degenerated to lqrx.kkt.random_kkt's special case: some D2
    block differs from its transpose by more than 0.01 on its square part, some D2 block has an input
    column of norm above 0.01, and the boundary stage blocks are not rows of a permutation matrix.
  * Structure plumbing.  irregular() reproduces lqrx.kkt.ConstraintBlocks on the uniform structures,
    oracle.KktStructure.from_blocks reproduces the oracle's uniform constructor and refuses arrays that
    do not chain, the committed class-1/2/3 structures have the block maxima the GPU file's docstring
    states, and every large-block case respects KB_PMAX = 64, KB_WMAX = 128 and KB_RMAX = 128.
  * fp32 yardstick.  For every fp32 case, float32_run (the Schur solve of oracle.kkt_dense's matrices in
    numpy.float32) is within 2.5e-5 of the truth: a factor 4 (kkt_truth.C) under the 1e-4 the GPU file
    asks of the fp32 kernels.

Measured with the committed generator (scale 0.3 everywhere), worst over the trajectories and over
dz, lam of each family; cond(D H⁻¹ Dᵀ) of trajectory 0 in brackets:
  oracle vs truth   A uniform, general D2/C   1.8e-12 ((5,1) N = 9, dense H)  [1.8e2 .. 6.2e3]
                      (cartpole N = 7 1.7e-12, DoubleIntegrator(2) 6.0e-13, (3) 4.9e-13, Dubins 2.8e-13)
                    B irregular small         1.3e-13 (class 1, ginv 0)   [2.8e2 .. 4.6e3]
                    C large-block             5.7e-14 (C-v)               [2.2e2 .. 4.7e3]
                    D workgroup               3.3e-13 (dense H)           [2.2e4 .. 1.3e5]
                    E fp32-rounded inputs     3.5e-14                     [6.2e2 .. 5.1e3]
  float32_run vs truth   E-iii 1.3e-5, E-stage 9.2e-6 (diagonal H) and 1.3e-5 (dense H), E-wg 9.3e-6.
"""
import numpy as np
import pytest

import kkt_general as G
from oracle import oracle as orc

ORACLE_TOL = 1e-11
F32_YARD = 2.5e-5
RUNS = G.runs()
ID = lambda r: f"{r[0]}-h{r[1]}-g{r[2]}"


@pytest.mark.parametrize("run", RUNS, ids=ID)
def test_oracle_within_a_tenth_of_the_gpu_tolerance(run):
    cid, hm, gi = run
    pb, ref = G.problem(cid, hm), G.oracle_solve(cid, hm, gi)
    assert (ref["info"] == 0).all()
    tr = G.truth(pb, gi)
    e = {k: G.traj_rel(ref[k], tr[k]) for k in ("dz", "lam")}
    print(f"ORACLE {ID(run)} dz {e['dz']:.2e} lam {e['lam']:.2e}")
    assert max(e.values()) <= ORACLE_TOL, e


@pytest.mark.parametrize("cid", list(G.CASES))
def test_generator_is_not_the_structural_special_case(cid):
    c = G.CASES[cid]
    st, pb = c.st, G.problem(cid, 2)
    asym = incol = 0.0
    for k, blk in enumerate(G.blocks(st, pb)):
        n1, nk = int(st.n1[k]), int(c.ns[k])
        if n1:
            D2 = blk[:n1]
            asym = max(asym, np.abs(D2[:, :n1] - D2[:, :n1].T).max())
            if blk.shape[1] > nk:
                incol = max(incol, np.linalg.norm(D2[:, nk:], axis=0).max())
    assert asym > 0.01 and incol > 0.01, (asym, incol)
    for k in (0, st.N - 1):
        Cb = G.blocks(st, pb)[k][int(st.n1[k]):int(st.n1[k]) + int(st.p[k])]
        if Cb.size:
            perm = np.isin(Cb, (0.0, 1.0)).all() and (Cb.sum(axis=1) == 1).all()
            assert not perm and np.abs(Cb - np.eye(*Cb.shape)).max() > 0.01 and (np.abs(Cb) > 1e-3).mean() > 0.9


@pytest.mark.parametrize("n,m,N,ps", [(3, 2, 5, [3, 0, 0, 0, 3]), (6, 3, 7, [6, 1, 1, 1, 1, 1, 6]), (7, 2, 4, [7, 1, 1, 0])])
def test_uniform_structures_are_the_special_case(n, m, N, ps):
    import lqrx.kkt as K

    a, b = G.irregular([n] * N, [m] * (N - 1) + [0], ps), K.ConstraintBlocks(n, m, N, ps)
    o, u = G.oracle_structure(a), orc.KktStructure(n, m, N, ps)
    for f in ("n1", "p", "n2", "w"):
        assert np.array_equal(getattr(a, f), getattr(b, f)) and np.array_equal(getattr(o, f), getattr(u, f)), f
        assert getattr(o, f).dtype == np.int32
    assert (a.n, a.m, a.N) == (n, m, N)
    assert (o.sY, o.sy, o.sg, o.P, o.sH(0), o.sH(2)) == (u.sY, u.sy, u.sg, u.P, u.sH(0), u.sH(2))
    assert a.sizes(0) == (o.sY, o.sy, o.sH(0), o.sg)


def test_from_blocks_refuses_arrays_that_do_not_chain():
    for n1, p, n2, w in (([1, 3], [0, 0], [3, 0], [2, 3]), ([0, 3], [0, 0], [2, 0], [2, 3]),
                         ([0, 3], [0, 0], [3, 1], [2, 3]), ([0, 3], [0], [3, 0], [2, 3])):
        with pytest.raises(ValueError):
            orc.KktStructure.from_blocks(n1, p, n2, w)


def _maxima(st):
    return int(max(st.n1.max(), st.p.max(), st.n2.max())), int(st.w.max()), int(st.rows.max())


def test_small_irregular_structures_land_in_their_class():
    """kkt_generic_class (lqrx_kkt.hip): 1 is parts ≤ 3, w ≤ 5, rows ≤ 6; 2 is ≤ 4, ≤ 8, ≤ 8; 3 is ≤ 8,
    ≤ 12, ≤ 16 — and each structure is irregular in the way the GPU file relies on."""
    want = {"B-class1": (3, 5, 6), "B-class2": (4, 7, 8), "B-class3": (8, 10, 15)}
    lim = {"B-class1": (3, 5, 6), "B-class2": (4, 8, 8), "B-class3": (8, 12, 16)}
    for cid, mx in want.items():
        c = G.CASES[cid]
        assert _maxima(c.st) == mx
        assert all(a <= b for a, b in zip(mx, lim[cid]))
        if cid != "B-class1":
            prev = lim[{"B-class2": "B-class1", "B-class3": "B-class2"}[cid]]
            assert any(a > b for a, b in zip(mx, prev))
        ps = np.asarray(c.ps)
        assert len(set(c.ns)) > 2 and len(set(c.ms[:-1])) > 2 and len(set(c.ps)) > 2
        assert any(ps[k] == 0 and ps[k - 1] > 0 and ps[k + 1] > 0 for k in range(1, len(ps) - 1))
        assert 0 < ps[0] < c.ns[0]


def test_large_block_cases_are_inside_the_large_block_limits():
    r16 = lambda x: (np.asarray(x) + 15) // 16 * 16
    for cid, c in G.CASES.items():
        st = c.st
        big = max(st.n1.max(), st.p.max(), st.n2.max()) <= 64 and st.w.max() <= 128
        if c.table == "C" or cid in ("E-iii", "E-stage"):
            assert big and (r16(st.n1) + r16(st.p) + r16(st.n2)).max() <= 128, cid
        if c.table == "D" or cid == "E-wg":
            assert not big, cid
    st = G.CASES["D-wg"].st
    assert max(st.n1.max(), st.p.max(), st.n2.max()) > 64 and st.w.max() > 128


@pytest.mark.parametrize("run", G.runs("E"), ids=ID)
def test_fp32_yardstick(run):
    cid, hm, gi = run
    pb = G.problem(cid, hm)
    assert all(np.array_equal(getattr(pb, k), np.asarray(getattr(pb, k), np.float32)) for k in ("Y", "y", "H", "g"))
    tr = G.truth(pb, gi)
    worst = 0.0
    for t in range(pb.batch):
        dz, lam = G.float32_run(pb, t, gi)
        worst = max(worst, G.traj_rel(dz[None], tr["dz"][t][None]), G.traj_rel(lam[None], tr["lam"][t][None]))
    print(f"F32 YARDSTICK {ID(run)} {worst:.2e}")
    assert worst <= F32_YARD
