"""General KKT inputs (test helper, no GPU): every row of Y = [D2; C; D1] random, and per-knot
structures with nothing uniform about them.

lqrx.kkt.random_kkt builds D2 = [−I 0] and boundary stage rows [I 0] on a first / uniform
interior / last structure; the C ABI (include/lqrx.h) takes n1, p, n2, w as four free per-knot
arrays and Y as data.  This module supplies what that promise covers and random_kkt does not:

  irregular(ns, ms, ps)   the structure of per-knot state widths, input widths and stage rows
  general_kkt(...)        a problem on it with every block entry random plus a structural part
  oracle_structure(st)    the same four arrays for the oracle (oracle.KktStructure.from_blocks)
  reference / truth       the C oracle's solve and tests/kkt_truth.py's refined truth, per batch
  float32_run(...)        the Schur-complement solve of oracle.kkt_dense's matrices carried out
                          in numpy.float32: the working-precision yardstick of the fp32 cases
  CASES, problem(...)     the case tables shared by tests/test_kkt_general.py (CPU) and
                          tests/test_kkt_general_gpu.py, each problem built once and left unchanged
"""
import dataclasses
import functools

import numpy as np

import kkt_truth
from oracle import oracle as orc

SCALE = 0.3
MODES4 = ((2, 1), (0, 1), (1, 1), (2, 0))          # (h_mode, ginv)
MODES3 = ((2, 1), (0, 1), (2, 0))


def irregular(ns, ms, ps):
    """KktStructure of per-knot state widths ns, input widths ms and stage rows ps: n1[k] = ns[k]
    (0 at k = 0), n2[k] = ns[k+1] (0 at the last knot), w[k] = ns[k] + ms[k]."""
    import lqrx.kkt as K

    ns, ms, ps = (np.asarray(a, np.int32) for a in (ns, ms, ps))
    N = len(ns)
    assert len(ms) == N and len(ps) == N
    n1 = np.concatenate([[0], ns[1:]]).astype(np.int32)
    n2 = np.concatenate([ns[1:], [0]]).astype(np.int32)
    return K.KktStructure(int(ns.max()), int(ms.max()), N, n1, ps.copy(), n2, (ns + ms).astype(np.int32))


def general_kkt(st, ns, batch, seed, h_mode=2, scale=SCALE):
    """A KktProblem on st whose every block entry is scale/√w · N(0,1) plus the structural part:
    −I on the D2 rows, +I on the first min(p, ns[k]) stage rows of the first and last knot, +I on
    the D1 rows over the state columns.  H, g and y as lqrx.kkt.random_kkt draws them (h_mode 1
    splits x/u at ns[k])."""
    import lqrx.kkt as K

    rng = np.random.default_rng(seed)
    N = st.N
    sY, sy, sH, sg = st.sizes(h_mode)
    Y, y, H = np.zeros((batch, sY)), np.zeros((batch, sy)), np.zeros((batch, sH))
    g = rng.standard_normal((batch, sg))
    oY = oy = oH = 0
    for k in range(N):
        n1, p, n2, w, nk = int(st.n1[k]), int(st.p[k]), int(st.n2[k]), int(st.w[k]), int(ns[k])
        rows = n1 + p + n2
        blk = (scale / np.sqrt(w)) * rng.standard_normal((batch, rows, w))
        blk[:, :n1, :nk] -= np.eye(n1, nk)
        if k in (0, N - 1):
            q = min(p, nk)
            blk[:, n1:n1 + q, :nk] += np.eye(q, nk)
        blk[:, n1 + p:, :nk] += np.eye(n2, nk)
        Y[:, oY:oY + rows * w] = np.swapaxes(blk, 1, 2).reshape(batch, -1)
        y[:, oy:oy + p + n2] = 0.1 * rng.standard_normal((batch, p + n2))
        if h_mode == K.H_DIAG:
            H[:, oH:oH + w] = 0.1 + rng.random((batch, w))
            oH += w
        else:
            M = rng.standard_normal((batch, w, w)) * 0.3
            Hk = np.einsum("bij,bkj->bik", M, M) + np.eye(w)
            if h_mode == K.H_BLOCKDIAG and w > nk:
                Hk[:, :nk, nk:] = 0.0
                Hk[:, nk:, :nk] = 0.0
            H[:, oH:oH + w * w] = np.swapaxes(Hk, 1, 2).reshape(batch, -1)
            oH += w * w
        oY += rows * w
        oy += p + n2
    return K.KktProblem(st, batch, h_mode, Y, y, H, g)


def blocks(st, pb, t=0):
    """The knot blocks of trajectory t as (rows × w) arrays."""
    out, o = [], 0
    Yt = np.asarray(pb.Y).reshape(pb.batch, -1)[t]
    for k in range(st.N):
        rows, w = int(st.rows[k]), int(st.w[k])
        out.append(Yt[o:o + rows * w].reshape(w, rows).T)
        o += rows * w
    return out


def round32(pb):
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return dataclasses.replace(pb, Y=f(pb.Y), y=f(pb.y), H=f(pb.H), g=f(pb.g))


def oracle_structure(st):
    return orc.KktStructure.from_blocks(st.n1, st.p, st.n2, st.w)


def reference(pb, ginv):
    """The C oracle on the whole batch: dz, lam (batch, ·), info."""
    r = orc.kkt_solve_batch(oracle_structure(pb.st), pb.batch, pb.Y, pb.y, pb.H, pb.g, h_mode=pb.h_mode,
                            ginv=ginv, nthreads=8)
    return dict(dz=r["dz"].reshape(pb.batch, -1), lam=r["lam"].reshape(pb.batch, -1), info=r["info"])


def truth(pb, ginv):
    """kkt_truth._truth_one of every trajectory: dz, lam (batch, ·)."""
    os_ = oracle_structure(pb.st)
    z = [kkt_truth._truth_one(os_, pb, t, ginv) for t in range(pb.batch)]
    return dict(dz=np.stack([a for a, _ in z]), lam=np.stack([b for _, b in z]))


def float32_run(pb, t, ginv):
    """λ = −S⁻¹r, δz = −H⁻¹(Dᵀλ + g) with S = D H⁻¹ Dᵀ, r = D H⁻¹ g − d on oracle.kkt_dense's H, D,
    g, d of trajectory t, every operation in numpy.float32 (H = I, g = 0 without ginv)."""
    sl = lambda a: np.asarray(a).reshape(pb.batch, -1)[t]
    dd = orc.kkt_dense(oracle_structure(pb.st), sl(pb.Y), sl(pb.y), sl(pb.H), sl(pb.g), h_mode=pb.h_mode)
    f = lambda a: np.asarray(a, np.float32)
    H, D, g, d = f(dd["H"]), f(dd["D"]), f(dd["g"]), f(dd["d"])
    if not ginv:
        H, g = np.eye(H.shape[0], dtype=np.float32), np.zeros_like(g)
    S = D @ np.linalg.solve(H, D.T)
    r = D @ np.linalg.solve(H, g) - d
    lam = -np.linalg.solve(S, r)
    dz = -np.linalg.solve(H, D.T @ lam + g)
    assert dz.dtype == np.float32 and lam.dtype == np.float32
    return dz, lam


def traj_rel(a, b):
    a = np.asarray(a, np.float64).reshape(b.shape)
    return float((np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-300)).max())


def batch_rel(a, b):
    a = np.asarray(a, np.float64).reshape(b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------ the case tables
@dataclasses.dataclass(frozen=True)
class Case:
    table: str                  # A uniform, B small irregular, C large-block, D workgroup, E fp32
    ns: tuple
    ms: tuple
    ps: tuple
    batch: int
    modes: tuple = MODES4
    prec: str = "f64"
    rel: str = "traj"           # "batch": errors over the batch-wide max (tests/test_kkt_gpu.py's rel)

    @property
    def st(self):
        return irregular(self.ns, self.ms, self.ps)


def _uni(n, m, N, ps, batch):
    return Case("A", (n,) * N, (m,) * (N - 1) + (0,), tuple(ps), batch, rel="batch")


def _traj(n, m, N, batch):
    return _uni(n, m, N, [n] + [0] * (N - 2) + [n], batch)


II = dict(ns=(32, 32, 32, 20, 32, 32, 32), ps=(20, 0, 0, 0, 0, 0, 24))
III = dict(ns=(24, 17, 30, 32, 20, 31, 18, 25), ms=(12,) * 7 + (0,), ps=(15, 0, 0, 0, 0, 0, 0, 14))

CASES = {
    # A: general Y on the uniform structures of the compile-time and padded kernels
    "A-dubins-N4": _traj(3, 2, 4, 130),
    "A-dubins-N101": _traj(3, 2, 101, 67),
    "A-cartpole-N7": _traj(4, 1, 7, 67),
    "A-cartpole-N101": _traj(4, 1, 101, 5),
    "A-di3-N6": _uni(6, 3, 6, [6, 1, 1, 1, 1, 6], 37),
    "A-di2-N12": _uni(4, 2, 12, [4] + [1] * 10 + [4], 37),
    "A-t52-N9": _traj(5, 2, 9, 67),
    "A-t73-N9": _traj(7, 3, 9, 33),
    "A-t62-N9": _traj(6, 2, 9, 65),
    "A-t84-N9": _traj(8, 4, 9, 33),
    "A-pad31-N12": _traj(3, 1, 12, 67),
    "A-pad51-N9": _traj(5, 1, 9, 33),
    "A-pad72-N6-stage": _uni(7, 2, 6, [7, 1, 1, 1, 1, 0], 31),
    # B: irregular structures on the run-time-shaped small kernels, one per class of kkt_generic_class
    "B-class1": Case("B", (2, 3, 2, 1, 3, 2, 2), (2, 2, 2, 3, 1, 2, 0), (1, 0, 1, 0, 1, 0, 2), 70),
    "B-class2": Case("B", (3, 4, 2, 4, 3, 4, 3), (3, 2, 4, 3, 4, 2, 0), (2, 0, 1, 0, 1, 0, 3), 70),
    "B-class3": Case("B", (5, 7, 4, 6, 8, 5, 7, 6), (4, 3, 5, 4, 2, 5, 3, 0), (3, 0, 2, 0, 1, 0, 2, 4), 70),
    # C: large-block family, fp64
    "C-i": Case("C", (16, 33, 20, 17, 40, 64, 31, 18), (9, 17, 30, 16, 24, 32, 8, 0), (10, 0, 17, 3, 0, 20, 1, 12), 5,
                MODES3),
    "C-ii": Case("C", II["ns"], (16,) * 6 + (0,), II["ps"], 5, MODES3),
    "C-iii": Case("C", batch=5, modes=MODES3, **III),
    "C-iv": Case("C", (16, 16, 40, 36, 40, 44, 40, 16, 16), (12, 30, 20, 20, 20, 20, 12, 12, 0),
                 (10, 0, 0, 0, 0, 0, 0, 0, 12), 5, MODES3),
    "C-v": Case("C", II["ns"], (16, 20, 9, 24, 12, 17, 0), II["ps"], 5, MODES3),
    # D: workgroup kernel, parts past 64 rows and w past 128
    "D-wg": Case("D", (40, 70, 66, 30, 72, 50), (30, 36, 20, 60, 60, 0), (20, 0, 9, 70, 0, 33), 3),
    # E: fp32 (inputs rounded to fp32), two large-block cases and one workgroup case
    "E-iii": Case("E", batch=5, modes=((2, 1),), prec="f32", **III),
    "E-stage": Case("E", (16, 20, 12, 24, 18, 16), (10, 8, 12, 9, 11, 0), (8, 3, 0, 5, 2, 10), 5, ((2, 1), (0, 1)), "f32"),
    "E-wg": Case("E", (30, 70, 24, 66, 30), (24, 30, 20, 30, 0), (12, 0, 5, 0, 20), 3, ((2, 1),), "f32"),
}


@functools.lru_cache(maxsize=None)
def problem(cid, h_mode):
    """The case's problem at h_mode (fp32 cases: rounded to fp32); shared and never modified."""
    import zlib

    c = CASES[cid]
    pb = general_kkt(c.st, c.ns, c.batch, zlib.crc32(cid.encode()) % 100000 + 7 * h_mode, h_mode)
    return round32(pb) if c.prec == "f32" else pb


@functools.lru_cache(maxsize=None)
def oracle_solve(cid, h_mode, ginv):
    return reference(problem(cid, h_mode), ginv)


def runs(table=None):
    """(cid, h_mode, ginv) of every run of the tables, or of those named."""
    return [(cid, hm, gi) for cid, c in CASES.items() if table is None or c.table in table for hm, gi in c.modes]
