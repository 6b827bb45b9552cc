"""Checker for lqrx_dp_rollout (include/lqrx.h): the closed-loop rollout of a policy (K_k, d_k) over S
scenarios per problem, written plainly in numpy float64, and the helpers its tests share.

Per problem b and scenario j:

    x_1 = x0
    u_k = min(max(−K_k x_k − α d_k, u_lo_b), u_hi_b)
    x_{k+1} = A_k x_k + B_k u_k + c_k + w_k
    J = Σ_k (½xᵀQ_k x + uᵀM_k x + ½uᵀR_k u + q_kᵀx + r_kᵀu) + ½x_NᵀQf x_N + qfᵀx_N

The problem is the flat ABI dict of tests/dp_truth.py (A, B, Q, R, Qf and, where present, c, M, q, r, qf;
n, m, batch, tv_AB, tv_QR); K and d are flat ABI arrays as a solve returns them.  J is a sum of terms of
either sign, so its error is measured on the scale of the terms, T = Σ|term| per trajectory (value_errors'
convention): relative to max(1, T).

Pinned on the CPU, with no library compute, against tests/dp_truth.py in tests/test_dp_rollout.py.
"""
import numpy as np

from dp_truth import _mats, cross_problem


def rollout_np(d: dict, N: int, K, dd, x0, alpha=None, w=None, u_lo=None, u_hi=None) -> dict:
    """x0 (batch, S, n); alpha (batch, S) or None (1); w (batch, S, N−1, n) or None (0); u_lo, u_hi
    (batch, m) or None (no bound).  Returns X (batch, S, N, n), U (batch, S, N−1, m), J (batch, S) and
    T (batch, S), the sum of the absolute values of J's terms; everything in float64."""
    n, m, bt = d["n"], d["m"], d["batch"]
    f8 = np.float64
    kab = N - 1 if d.get("tv_AB") else 1
    kqr = N - 1 if d.get("tv_QR") else 1
    vec = lambda key, k, r: (np.asarray(d[key], f8).reshape(bt, k, r) if d.get(key) is not None
                             else np.zeros((bt, k, r)))
    A = _mats(d["A"], bt, kab, n, n, f8)
    B = _mats(d["B"], bt, kab, n, m, f8)
    c = vec("c", kab, n)
    Q = _mats(d["Q"], bt, kqr, n, n, f8)
    R = _mats(d["R"], bt, kqr, m, m, f8)
    M = _mats(d["M"], bt, kqr, m, n, f8) if d.get("M") is not None else np.zeros((bt, kqr, m, n))
    Qf = _mats(d["Qf"], bt, 1, n, n, f8)[:, 0]
    q, r, qf = vec("q", kqr, n), vec("r", kqr, m), vec("qf", 1, n)[:, 0]
    Ks = _mats(K, bt, N - 1, m, n, f8)
    ds = np.asarray(dd, f8).reshape(bt, N - 1, m) if dd is not None else np.zeros((bt, N - 1, m))
    x0 = np.asarray(x0, f8)
    S = x0.shape[1]
    al = np.ones((bt, S)) if alpha is None else np.asarray(alpha, f8).reshape(bt, S)
    W = np.zeros((bt, S, N - 1, n)) if w is None else np.asarray(w, f8).reshape(bt, S, N - 1, n)
    lo = np.full((bt, m), -np.inf) if u_lo is None else np.asarray(u_lo, f8).reshape(bt, m)
    hi = np.full((bt, m), np.inf) if u_hi is None else np.asarray(u_hi, f8).reshape(bt, m)
    X = np.zeros((bt, S, N, n))
    U = np.zeros((bt, S, N - 1, m))
    J = np.zeros((bt, S))
    T = np.zeros((bt, S))
    mv = lambda Z, v: np.einsum("bij,bsj->bsi", Z, v)        # one matrix per problem, S columns
    dot = lambda a, b: np.einsum("bsi,bsi->bs", a, b)

    def add(term):
        nonlocal J, T
        J = J + term
        T = T + np.abs(term)

    X[:, :, 0] = x0
    for k in range(1, N):
        ia, iq = (k - 1) % kab, (k - 1) % kqr
        x = X[:, :, k - 1]
        u = -mv(Ks[:, k - 1], x) - al[:, :, None] * ds[:, None, k - 1]
        u = np.minimum(np.maximum(u, lo[:, None]), hi[:, None])
        U[:, :, k - 1] = u
        X[:, :, k] = mv(A[:, ia], x) + mv(B[:, ia], u) + c[:, None, ia] + W[:, :, k - 1]
        add(0.5 * dot(x, mv(Q[:, iq], x)))
        add(dot(u, mv(M[:, iq], x)))
        add(0.5 * dot(u, mv(R[:, iq], u)))
        add(dot(x, np.broadcast_to(q[:, None, iq], x.shape)))
        add(dot(u, np.broadcast_to(r[:, None, iq], u.shape)))
    xN = X[:, :, N - 1]
    add(0.5 * dot(xN, mv(Qf, xN)))
    add(dot(xN, np.broadcast_to(qf[:, None], xN.shape)))
    return dict(X=X, U=U, J=J, T=T)


def xu_error(got, ref) -> float:
    """max|a − b| / max(1, max|b|): dp_truth.check's measure for X and U"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


def j_error(got, ref: dict) -> float:
    """max over the trajectories of |J − J_ref| / max(1, Σ|terms|)"""
    return float((np.abs(np.asarray(got, np.float64).reshape(ref["J"].shape) - ref["J"]) / np.maximum(1.0, ref["T"])).max())


def scenarios(n, m, N, bt, S, seed):
    """x0 ~ N(0, 1), α ~ U[0, 1], w ~ 0.1·N(0, 1) for a case"""
    rng = np.random.default_rng(seed + 101)
    return dict(x0=rng.standard_normal((bt, S, n)), alpha=rng.random((bt, S)),
                w=0.1 * rng.standard_normal((bt, S, N - 1, n)))


def clamp_bounds(U_free):
    """±(the 0.9 quantile of |u| per control row over the case's unclamped rollout U_free
    (batch, S, N−1, m)) → u_lo, u_hi shaped (batch, m)"""
    bt, m = U_free.shape[0], U_free.shape[-1]
    hi = np.quantile(np.abs(U_free).reshape(-1, m), 0.9, axis=0)
    hi = np.ascontiguousarray(np.broadcast_to(hi, (bt, m)))
    return -hi, hi


def clamp_fractions(U, u_lo, u_hi):
    """(fraction of U's entries exactly at a bound, fraction strictly inside)"""
    lo, hi = u_lo[:, None, None, :], u_hi[:, None, None, :]
    at = (U == lo) | (U == hi)
    inside = (U > lo) & (U < hi)
    return float(at.mean()), float(inside.mean())


def check_clamp_condition(U, u_lo, u_hi, what=""):
    at, inside = clamp_fractions(np.asarray(U, np.float64), u_lo, u_hi)
    print(f"CLAMP {what} at a bound {at:.3f} strictly inside {inside:.3f}")
    assert at >= 0.05 and inside >= 0.05, (what, at, inside)
    assert abs(at + inside - 1.0) < 1e-12, (what, at, inside)   # nothing outside the bounds


__all__ = ["rollout_np", "xu_error", "j_error", "scenarios", "clamp_bounds", "clamp_fractions",
           "check_clamp_condition", "cross_problem"]
