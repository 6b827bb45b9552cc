"""Shared SQP test cases: one builder for tests/test_sqp_matrix.py (CPU: oracle pinning and the
conditions every GPU case must meet), tests/test_sqp_matrix_gpu.py (device parity) and the
guard-zone cases of tests/test_guard_ls_sqp_gpu.py.

case(name) → (lqrx.sqp.SQPProblem, [oracle TrajSQP per trajectory], Z0, x0, xf): the same
problem stated for the device and for oracle/sqp_oracle.py.  Every case has weights Q, R, Qf with
pairwise different entries (so Q[j] read for Q[i], or Q for Qf, changes the answer), every
stage-constrained case a nonzero stage_b, the two-row stage matrices differ from their
transposes' packing, and the cartpole cases change all four model parameters.

reference(name) solves every trajectory once with the oracle (cached) and keeps its trace
(oracle.sqp_oracle.new_trace: decision margins, per-step multipliers).  Seeds and μ are chosen
so that the conditions asserted in tests/test_sqp_matrix.py hold: no decision of a case's oracle
run is closer than 1e-6 relative to a tie, the constraint Jacobian at Z0 has σ_min/σ_max ≥ 1e-4,
and every trajectory accepts a step.
"""
from dataclasses import dataclass, replace
from functools import lru_cache

import numpy as np

from oracle import sqp_oracle as S

TOL = {"dubins": 1e-9, "cartpole": 1e-8, "di": 1e-8}   # the bounds of tests/test_sqp.py per model
CARTPOLE_PARAMS = (1.3, 0.25, 0.6, 9.0)                 # mc, mp, l, g: none the default


@dataclass(frozen=True)
class Spec:
    model: str                 # dubins | cartpole | di1 | di2 | di3
    N: int
    pk: int = 0
    mu: float = 10.0
    seed: int = 0
    batch: int = 3
    max_iters: int = 10
    tol_p: float = 1e-5
    tol_d: float = 1e-5
    tf: float = 0.0            # 0: the model's default horizon
    row: tuple = (0.6, -0.5, 0.05)   # dubins with a stage row: A_s

    @property
    def family(self):
        return "di" if self.model.startswith("di") else self.model


SPECS = {
    # model × stage rows (the KKT routes no other SQP test takes)
    "dubins_pk1_N4": Spec("dubins", 4, 1, mu=100.0, seed=1, tol_d=1e-2),
    "dubins_pk1_N11": Spec("dubins", 11, 1, mu=100.0, seed=2, tol_d=1e-2),
    "di1_pk0_N4": Spec("di1", 4, seed=3),
    "di1_pk0_N12": Spec("di1", 12, seed=4),
    "di2_pk0_N12": Spec("di2", 12, seed=5),
    "di3_pk0_N12": Spec("di3", 12, seed=6),
    "di3_pk2_N8": Spec("di3", 8, 2, seed=7),
    "di3_pk2_N12": Spec("di3", 12, 2, seed=8),
    # data: weights, cartpole parameters, stage_b on the already-tested routes
    "dubins_pk0_N11": Spec("dubins", 11, seed=9, batch=4, tol_d=1e-2),
    "cartpole_N6": Spec("cartpole", 6, mu=1.0, seed=10, tol_d=1e-2),
    "di2_pk1_N12": Spec("di2", 12, 1, seed=11),
    # knot-count edges (lanes take knots lane, lane + 64, …; Y is copied out per 64-knot chunk)
    "dubins_pk0_N3": Spec("dubins", 3, seed=12, batch=4, mu=100.0, tol_d=1e-2),
    "dubins_pk0_N64": Spec("dubins", 64, seed=13, batch=2, tol_d=1e-2),
    "dubins_pk0_N65": Spec("dubins", 65, seed=14, batch=2, tol_d=1e-2),
    "dubins_pk0_N128": Spec("dubins", 128, seed=15, batch=2, max_iters=3, tol_d=1e-2),
    "dubins_pk0_N129": Spec("dubins", 129, seed=16, batch=2, max_iters=3, tol_d=1e-2),
    # 64 short steps: the row above makes the Newton systems ill-conditioned on the way (A H⁻¹ Aᵀ at
    # cond 1e8, status 2).  This row and horizon keep it at 4e5, the level of the other Dubins cases
    "dubins_pk1_N65": Spec("dubins", 65, 1, mu=100.0, seed=17, batch=2, tol_d=1e-2, tf=48.0, row=(0.3, 0.3, 0.3)),
    "cartpole_N65": Spec("cartpole", 65, mu=1.0, seed=18, batch=2, tol_d=1e-3),
    "di1_pk0_N65": Spec("di1", 65, seed=19, batch=2),
    "di2_pk1_N65": Spec("di2", 65, 1, seed=20, batch=2, tf=16.0),
    # ragged batches with loose tolerances: trajectories stop at different iterations.  tol_d is
    # above ‖∇f‖ at the solutions, so a converged trajectory is also converged for a second call
    # (which starts from λ = 0), and tol_p decides when each one stops
    "dubins_pk1_ragged": Spec("dubins", 11, 1, mu=100.0, seed=21, batch=70, tol_p=1e-4, tol_d=50.0),
    "di3_pk2_ragged": Spec("di3", 8, 2, seed=22, batch=70, tol_p=1e-4, tol_d=1e3),
}
GPU_CASES = tuple(SPECS)
PINNED = ("dubins_pk1_N11", "di1_pk0_N12", "di2_pk0_N12", "di3_pk0_N12", "di3_pk2_N12")   # new (model, pk)
NONLINEAR = tuple(n for n, s in SPECS.items() if s.family in ("dubins", "cartpole"))
# the KKT routes that ignore the SQP's trajectory subset and solve the whole batch
WHOLE_BATCH = {"generic (N = 3)": ("dubins_pk0_N3",), "DI(3) pk 2": ("di3_pk2_ragged",)}


def _weights(n, m, base_q, base_r, base_qf):
    """pairwise different diagonal weights around the reference's values"""
    Q = tuple(base_q[i] * (1.0 + 0.5 * i) for i in range(n))
    R = tuple(base_r[i] * (1.0 + 0.5 * i) for i in range(m))
    Qf = tuple(base_qf[i] * (1.0 + 0.2 * i) for i in range(n))
    return Q, R, Qf


def _stack(probs, z0s, x0s, xfs):
    return probs, np.stack(z0s), np.stack(x0s), np.stack(xfs)


def _dubins(sp):
    import lqrx.sqp as L

    rng = np.random.default_rng(sp.seed)
    N, dt = sp.N, (sp.tf or 3.0) / (sp.N - 1)
    Q, R, Qf = _weights(3, 2, [1e-2] * 3, [1e-1] * 2, [100.0] * 3)
    # a stage row the straight line from x0 ≈ 0 to xf ≈ (3, 3, π/2) nearly satisfies
    SA = np.array([sp.row]) if sp.pk else np.zeros((0, 3))
    Sb = np.array([0.04]) if sp.pk else np.zeros(0)
    probs, z0s, x0s, xfs = [], [], [], []
    for _ in range(sp.batch):
        x0 = 0.1 * rng.standard_normal(3)
        xf = np.array([3.0, 3.0, np.pi / 2]) + 0.2 * rng.standard_normal(3)
        z0 = S.initial_guess(N, dt, x0, xf)
        z0 += 0.05 * rng.standard_normal(z0.shape)
        probs.append(S.TrajSQP(N, dt, Q, R, Qf, x0, xf, sp.mu, S.DUBINS, (SA, Sb) if sp.pk else None))
        z0s.append(z0), x0s.append(x0), xfs.append(xf)
    prob = replace(L.DubinsSQP(N, dt, Q, R, Qf, sp.mu, sp.max_iters, sp.tol_p, sp.tol_d),
                   stage_A=tuple(SA.ravel()), stage_b=tuple(Sb))
    return (prob, *_stack(probs, z0s, x0s, xfs))


def _cartpole(sp):
    import lqrx.sqp as L

    rng = np.random.default_rng(sp.seed)
    N, tf = sp.N, sp.tf or 2.0
    dt = tf / (N - 1)
    par = CARTPOLE_PARAMS
    model = S.Model("cartpole", 4, 1, lambda x, u: S.cartpole(x, u, par), 1, par)
    Q, R, Qf = _weights(4, 1, [1e-2] * 4, [1e-1], [100.0] * 4)
    prob = L.CartpoleSQP(N, tf, Q, R, Qf, par, sp.mu, sp.max_iters, sp.tol_p, sp.tol_d)
    probs, z0s, x0s, xfs = [], [], [], []
    for _ in range(sp.batch):
        x0 = 0.05 * rng.standard_normal(4)
        xf = np.array([rng.uniform(-1, 1), rng.uniform(-0.5, 0.5), 0.0, 0.0])     # a gentle goal
        X = S.rollout(model, x0, np.full((N - 1, 1), 0.01), dt)
        z0 = np.concatenate([np.concatenate([X[k], [0.01]]) for k in range(N - 1)] + [X[-1]])
        probs.append(S.TrajSQP(N, dt, Q, R, Qf, x0, xf, sp.mu, model))
        z0s.append(z0), x0s.append(x0), xfs.append(xf)
    return (prob, *_stack(probs, z0s, x0s, xfs))


def _di(sp):
    import lqrx.sqp as L

    D = int(sp.model[2])
    rng = np.random.default_rng(sp.seed)
    N, dt = sp.N, (sp.N - 1) / (sp.tf or 2.0)             # as the reference writes it
    Q, R, Qf = _weights(2 * D, D, [10.0] * D + [1.0] * D, [0.1] * D, [100.0] * D + [10.0] * D)
    SA = rng.random((sp.pk, 2 * D))
    Sb = 0.05 * (1.0 + rng.random(sp.pk))
    prob = L.SQPProblem(L.MODEL_DOUBLE_INTEGRATOR[D], N, dt, Q, R, Qf, (0.0,) * 4, sp.mu, sp.max_iters, sp.tol_p,
                        sp.tol_d, tuple(SA.ravel()), tuple(Sb))
    probs, z0s, x0s, xfs = [], [], [], []
    for _ in range(sp.batch):
        x0 = np.concatenate([np.ones(D), np.zeros(D)]) + 0.2 * rng.standard_normal(2 * D)
        xf = 0.1 * rng.standard_normal(2 * D)
        p = S.TrajSQP(N, dt, Q, R, Qf, x0, xf, sp.mu, S.DOUBLE_INTEGRATOR[D], (SA, Sb) if sp.pk else None)
        z0 = 0.1 * rng.standard_normal(p.NN)
        probs.append(p), z0s.append(z0), x0s.append(x0), xfs.append(xf)
    return (prob, *_stack(probs, z0s, x0s, xfs))


@lru_cache(maxsize=None)
def case(name):
    """(SQPProblem, [TrajSQP], Z0, x0, xf) of a named case; cached — treat as read-only."""
    sp = SPECS[name]
    out = {"dubins": _dubins, "cartpole": _cartpole, "di": _di}[sp.family](sp)
    for a in out[2:]:
        a.setflags(write=False)
    return out


def tol(name):
    return TOL[SPECS[name].family]


def structure(name):
    """(nx, nu, N, p) of the case's KKT structure: knot 0 and the last carry nx rows, interior pk."""
    prob = case(name)[0]
    return prob.n, prob.m, prob.N, [prob.n] + [prob.stage_rows] * (prob.N - 2) + [prob.n]


@lru_cache(maxsize=None)
def reference(name, b):
    """The oracle's solve of trajectory b with the case's options, and its trace; cached."""
    prob, probs, Z0, _, _ = case(name)
    tr = S.new_trace()
    r = S.solve(probs[b], Z0[b], iters=prob.max_iters, tol_p=prob.tol_p, tol_d=prob.tol_d, trace=tr)
    return r, tr


def spot(name):
    """the trajectories a test compares: all of a small batch, the wave edges of a ragged one"""
    bt = SPECS[name].batch
    return tuple(range(bt)) if bt <= 8 else (0, 1, 63, 64, bt - 1)


def sigma_ratio(name, b):
    """σ_min/σ_max of the constraint Jacobian at Z0"""
    _, probs, Z0, _, _ = case(name)
    s = np.linalg.svd(probs[b].jac(Z0[b]), compute_uv=False)
    return s[-1] / s[0]
