// lqrx_dp_box.hip — input bounds u_lo ≤ u_k ≤ u_hi by ADMM on the re-solve factors
// (lqrx_dp_resolve_box; include/lqrx.h).  Layout 0 only, n ≤ 64, m ≤ 32.
//
// With K_k, E_k⁻¹, Pc_k of one solve made with R + ρI, the u-step of ADMM on
//   min Σ_k ℓ_k(x_k, u_k) + ℓ_N(x_N) + I[lo ≤ z ≤ hi] + (ρ/2)‖u − z + w‖²,   x⁺ = Ax + Bu + c
// is the re-solve recursion with r̂_k = r_k − ρ(z_k − w_k) in the place of r_k, and the z- and
// w-steps are element-wise.  Per instance, iteration i = 1 … max_iter:
//
//   r̂_k  = r_k − ρ(z_k − w_k)
//   (d, X, U) = the re-solve recursion (lqrx_dp_resolve.hip) on (q, r̂, qf, x0)
//   û_k  = αu_k + (1 − α)z_k          z⁺_k = min(max(û_k + w_k, lo), hi)          w⁺_k = w_k + û_k − z⁺_k
//   r_prim = max_k ‖u_k − z⁺_k‖∞      r_dual = ρ·max_k ‖z⁺_k − z_k‖∞
//   stop after the first iteration with r_prim ≤ eps_prim and r_dual ≤ eps_dual (both eps > 0)
//
// dp_box_kernel: one wave per (problem, 16 instances), the grid and work items of dp_resolve_kernel,
// with the iteration loop around its two passes.  The backward pass is the re-solve's with r̂ formed
// in registers from r, z, w; the forward pass is the re-solve's with the z, w update and the two
// running maxima done on the U tile in registers: r̂ and û never touch memory.  z, w (and d) go through
// the d_load / d_store map in both passes: the same lane at the same address, in program order, makes
// iteration i's store visible to iteration i + 1's load — the argument the re-solve makes for d.  No
// fence, no LDS.
//
// A column's residuals are a max over the tile's registers and the four lanes that hold the column
// (xor-shuffles by 16 and 32).  Each lane keeps `active` for its column; every store is predicated on
// it.  A finished column rides along on values it no longer stores: its z, w, d in memory are frozen,
// so it recomputes its last iteration — its bits do not depend on how long its neighbours run, nor, as
// in the re-solve, on S, its position, or the outputs asked for.  The wave leaves the loop when no
// column is active (a ballot: a wave-uniform branch); the loop is counted and bounded by max_iter.
// The maxima keep a NaN (nan_max) and the stopping test is false on one, so a NaN never converges.
#include "lqrx_internal.h"
#include "lqrx_resolve_ops.h"
#include "lqrx_scen_ops.h"
#include "lqrx_tile.h"

#include <limits>

namespace lqrx {
namespace {

// max(a, v) that keeps a NaN of either side (fmax would drop it)
template <typename T> __device__ __forceinline__ T nan_max(T a, T v) { return (a != a || v <= a) ? a : v; }

// a bound of `rows` elements along the rows of C-layout tiles (every column the same); `none` past
// it and for a null bound
template <typename T, int IT>
__device__ __forceinline__ void bound_load(typename Tile<T>::acc (&D)[IT], const T *__restrict__ v, int rows, int lane,
                                           T none)
{
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = it * 16 + Tile<T>::row(lane, r);
            const bool ok = row < rows;
            const T x = v ? v[ok ? row : 0] : none;
            D[it][r] = ok ? x : none;
        }
}

// TV, PF as in dp_resolve_kernel; with PF the next knot's z, w ride with its r
template <typename T, int NT, int MT, bool TV, bool PF>
__global__ __launch_bounds__(64) void dp_box_kernel(const DpBoxArgs a)
{
    using acc = typename Tile<T>::acc;
    const int lane = threadIdx.x, n = a.n, m = a.m, N = a.N;
    const int64_t tiles = (a.S + DP_COLS - 1) / DP_COLS, total = a.batch * tiles;
    const int64_t nn = (int64_t)n * n, nm = (int64_t)n * m, mm = (int64_t)m * m;
    const int64_t kab = TV ? N - 1 : 1, kqr = a.tv_QR ? N - 1 : 1;
    const T rho = (T)a.rho, alpha = (T)a.relax, om = T(1) - alpha, eps_p = (T)a.eps_prim, eps_d = (T)a.eps_dual;
    const bool stops = a.eps_prim > 0 && a.eps_dual > 0;   // an eps of 0 never stops early
    const T inf = std::numeric_limits<T>::infinity();
    for (int64_t wi = blockIdx.x; wi < total; wi += gridDim.x) {
        const int64_t b = wi / tiles, j = (wi - b * tiles) * DP_COLS + tcol(lane);
        const bool live = j < a.S;
        const int64_t t = b * a.S + (live ? j : 0);   // a dead column addresses instance 0 and selects zero
        const T *Ab = (const T *)a.A + b * nn * kab, *Bb = (const T *)a.B + b * nm * kab;
        const T *Kb = (const T *)a.K + b * nm * (N - 1), *Eb = (const T *)a.Einv + b * mm * (N - 1);
        const T *gb = a.Pc ? (const T *)a.Pc + b * n * (N - 1) : nullptr;
        const T *cb = a.c ? (const T *)a.c + b * n * kab : nullptr;
        const T *qt = a.q ? (const T *)a.q + t * kqr * n : nullptr;
        const T *rt = a.r ? (const T *)a.r + t * kqr * m : nullptr;
        const T *lob = a.u_lo ? (const T *)a.u_lo + b * m : nullptr;
        const T *hib = a.u_hi ? (const T *)a.u_hi + b * m : nullptr;
        T *dt = (T *)a.d + t * (N - 1) * m, *Zt = (T *)a.Z + t * (N - 1) * m, *Wt = (T *)a.W + t * (N - 1) * m;
        T *Xt = a.X ? (T *)a.X + t * N * n : nullptr;
        T *Ut = a.U ? (T *)a.U + t * (N - 1) * m : nullptr;
        const auto qk = [&](int k) { return qt ? qt + (a.tv_QR ? (int64_t)k * n : 0) : nullptr; };
        const auto rk = [&](int k) { return rt ? rt + (a.tv_QR ? (int64_t)k * m : 0) : nullptr; };
        const auto gk = [&](int k) { return gb ? gb + (int64_t)k * n : nullptr; };

        bool active = live;      // this lane's column still iterates: the predicate of every store
        int iters = 0;
        T res_p = 0, res_d = 0;  // the residuals of the column's last iteration
        for (int iter = 0; iter < a.max_iter; ++iter) {
            // The lane index of this iteration's loads and stores, behind a zero the compiler cannot see
            // (the launcher refuses N < 2): the lane-derived offsets and the time-invariant operands are
            // then formed inside each pass, as in the re-solve, instead of being hoisted out of the
            // iteration loop and kept live across both passes, which spilled every instantiation.
            const int ln = lane + (a.N < 2 ? iter : 0);
            // ---- backward: the re-solve's, on r̂ = r − ρ(z − w) ----
            {
                acc p[NT];
                rows_load<T, NT>(p, a.qf ? (const T *)a.qf + t * n : nullptr, n, ln, live);

                acc At[NT][NT], Bt[NT][MT], Kt[MT][NT], Et[MT][MT], qv[NT], rv[MT], gv[NT], zv[MT], wv[MT];
                if (PF || !TV) {
                    const int64_t k0 = TV ? N - 2 : 0;
                    tiles_load<T, NT, NT>(At, Ab + k0 * nn, n, n, n, ln, false);
                    tiles_load<T, NT, MT>(Bt, Bb + k0 * nm, n, m, n, ln, false);
                }
                if (PF) {
                    tiles_load<T, MT, NT>(Kt, Kb + (int64_t)(N - 2) * nm, m, n, m, ln, false);
                    tiles_load<T, MT, MT>(Et, Eb + (int64_t)(N - 2) * mm, m, m, m, ln, false);
                    rows_load<T, NT>(qv, qk(N - 2), n, ln, live);
                    rows_load<T, MT>(rv, rk(N - 2), m, ln, live);
                    rows_load<T, NT>(gv, gk(N - 2), n, ln);
                    d_load<T, MT>(zv, Zt + (int64_t)(N - 2) * m, m, ln, live);
                    d_load<T, MT>(wv, Wt + (int64_t)(N - 2) * m, m, ln, live);
                }
                for (int k = N - 2; k >= 0; --k) {
                    acc An[NT][NT], Bn[NT][MT], Kn[MT][NT], En[MT][MT], qn[NT], rn[MT], gn[NT], zn[MT], wn[MT];
                    if (PF) {   // the next knot's operands (the last knot loads itself again: unconditional loads)
                        const int k1 = k > 0 ? k - 1 : 0;
                        tiles_load<T, MT, NT>(Kn, Kb + (int64_t)k1 * nm, m, n, m, ln, false);
                        tiles_load<T, MT, MT>(En, Eb + (int64_t)k1 * mm, m, m, m, ln, false);
                        if (TV) {
                            tiles_load<T, NT, NT>(An, Ab + (int64_t)k1 * nn, n, n, n, ln, false);
                            tiles_load<T, NT, MT>(Bn, Bb + (int64_t)k1 * nm, n, m, n, ln, false);
                        }
                        rows_load<T, NT>(qn, qk(k1), n, ln, live);
                        rows_load<T, MT>(rn, rk(k1), m, ln, live);
                        rows_load<T, NT>(gn, gk(k1), n, ln);
                        d_load<T, MT>(zn, Zt + (int64_t)k1 * m, m, ln, live);
                        d_load<T, MT>(wn, Wt + (int64_t)k1 * m, m, ln, live);
                    } else {
                        tiles_load<T, MT, NT>(Kt, Kb + (int64_t)k * nm, m, n, m, ln, false);
                        tiles_load<T, MT, MT>(Et, Eb + (int64_t)k * mm, m, m, m, ln, false);
                        if (TV) {
                            tiles_load<T, NT, NT>(At, Ab + (int64_t)k * nn, n, n, n, ln, false);
                            tiles_load<T, NT, MT>(Bt, Bb + (int64_t)k * nm, n, m, n, ln, false);
                        }
                        rows_load<T, NT>(qv, qk(k), n, ln, live);
                        rows_load<T, MT>(rv, rk(k), m, ln, live);
                        rows_load<T, NT>(gv, gk(k), n, ln);
                        d_load<T, MT>(zv, Zt + (int64_t)k * m, m, ln, live);
                        d_load<T, MT>(wv, Wt + (int64_t)k * m, m, ln, live);
                    }
                    // p̃ = p + g;  h = r̂ + Bᵀp̃ with p_k = q + Aᵀp̃ alongside
                    acc ph[NT], h[MT], pn[NT], d[MT];
#pragma unroll
                    for (int it = 0; it < NT; ++it) ph[it] = p[it] + gv[it];
#pragma unroll
                    for (int it = 0; it < MT; ++it) h[it] = rv[it] - rho * (zv[it] - wv[it]);
                    vec_copy<T, NT>(pn, qv);
                    tn_pair<T, NT, MT, NT, false>(h, Bt, pn, At, ph);
                    // d = E⁻¹h with p_k −= Kᵀh alongside
#pragma unroll
                    for (int it = 0; it < MT; ++it) d[it] = acc{0, 0, 0, 0};
                    tn_pair<T, MT, MT, NT, true>(d, Et, pn, Kt, h);
                    d_store<T, MT>(d, dt + (int64_t)k * m, m, ln, active);
                    vec_copy<T, NT>(p, pn);

                    if (PF) {
                        tiles_copy<T, MT, NT>(Kt, Kn);
                        tiles_copy<T, MT, MT>(Et, En);
                        if (TV) {
                            tiles_copy<T, NT, NT>(At, An);
                            tiles_copy<T, NT, MT>(Bt, Bn);
                        }
                        vec_copy<T, NT>(qv, qn);
                        vec_copy<T, MT>(rv, rn);
                        vec_copy<T, NT>(gv, gn);
                        vec_copy<T, MT>(zv, zn);
                        vec_copy<T, MT>(wv, wn);
                    }
                }
            }

            // ---- forward: the re-solve's rollout, then z, w and the residuals on the U tile ----
            T rp = 0, rd = 0;
            {
                acc X[NT], U[MT], lo[MT], hi[MT];
                bound_load<T, MT>(lo, lob, m, ln, -inf);
                bound_load<T, MT>(hi, hib, m, ln, inf);
                rows_load<T, NT>(X, a.x0 ? (const T *)a.x0 + t * n : nullptr, n, ln, live);
                if (Xt) rows_store<T, NT>(X, Xt, n, ln, active);
                T Kc[MT][NT][4], Ac[NT][NT][4], Bc[NT][MT][4];
                if (PF || !TV) {
                    op_load<T, NT, NT>(Ac, Ab, n, n, ln);
                    op_load<T, NT, MT>(Bc, Bb, n, m, ln);
                }
                if (PF) op_load<T, MT, NT>(Kc, Kb, m, n, ln);
                for (int k = 0; k < N - 1; ++k) {
                    T Kn[MT][NT][4], An[NT][NT][4], Bn[NT][MT][4];
                    if (PF) {
                        const int k1 = k + 1 < N - 1 ? k + 1 : k;
                        op_load<T, MT, NT>(Kn, Kb + k1 * nm, m, n, ln);
                        if (TV) {
                            op_load<T, NT, NT>(An, Ab + k1 * nn, n, n, ln);
                            op_load<T, NT, MT>(Bn, Bb + k1 * nm, n, m, ln);
                        }
                    } else {
                        op_load<T, MT, NT>(Kc, Kb + k * nm, m, n, ln);
                        if (TV) {
                            op_load<T, NT, NT>(Ac, Ab + k * nn, n, n, ln);
                            op_load<T, NT, MT>(Bc, Bb + k * nm, n, m, ln);
                        }
                    }
                    // U = −(K·X + d)
                    acc z[MT], w[MT];
                    d_load<T, MT>(U, dt + (int64_t)k * m, m, ln, live);
                    d_load<T, MT>(z, Zt + (int64_t)k * m, m, ln, live);
                    d_load<T, MT>(w, Wt + (int64_t)k * m, m, ln, live);
                    op_mma<T, MT, NT>(U, Kc, X);
#pragma unroll
                    for (int it = 0; it < MT; ++it) U[it] = -U[it];
                    if (Ut) rows_store<T, MT>(U, Ut + (int64_t)k * m, m, ln, active);
                    // X⁺ = c + A·X + B·U
                    acc Xn[NT];
                    rows_load<T, NT>(Xn, cb ? cb + (TV ? (int64_t)k * n : 0) : nullptr, n, ln);
                    op_mma<T, NT, NT>(Xn, Ac, X);
                    op_mma<T, NT, MT>(Xn, Bc, U);
                    vec_copy<T, NT>(X, Xn);
                    if (Xt) rows_store<T, NT>(X, Xt + (int64_t)(k + 1) * n, n, ln, active);
                    // û = αu + (1 − α)z, z⁺ = clip(û + w), w⁺ = w + û − z⁺; the compares pass a NaN on
#pragma unroll
                    for (int it = 0; it < MT; ++it)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const T u = U[it][r], z0 = z[it][r], w0 = w[it][r];
                            const T uh = alpha * u + om * z0, v = uh + w0;
                            const T vl = v < lo[it][r] ? lo[it][r] : v;
                            const T zp = vl > hi[it][r] ? hi[it][r] : vl;
                            z[it][r] = zp;
                            w[it][r] = w0 + uh - zp;
                            rp = nan_max(rp, fabs(u - zp));
                            rd = nan_max(rd, fabs(zp - z0));
                        }
                    d_store<T, MT>(z, Zt + (int64_t)k * m, m, ln, active);
                    d_store<T, MT>(w, Wt + (int64_t)k * m, m, ln, active);
                    if (PF) {
                        op_copy<T, MT, NT>(Kc, Kn);
                        if (TV) {
                            op_copy<T, NT, NT>(Ac, An);
                            op_copy<T, NT, MT>(Bc, Bn);
                        }
                    }
                }
            }
            // the column's residuals: its rows live in the four lanes l, l ^ 16, l ^ 32, l ^ 48
            rp = nan_max(rp, (T)__shfl_xor(rp, 16));
            rd = nan_max(rd, (T)__shfl_xor(rd, 16));
            rp = nan_max(rp, (T)__shfl_xor(rp, 32));
            rd = nan_max(rd, (T)__shfl_xor(rd, 32));
            rd = rho * rd;
            if (active) {
                iters = iter + 1;
                res_p = rp;
                res_d = rd;
            }
            active = active && !(stops && rp <= eps_p && rd <= eps_d);   // false on a NaN: it never converges
            if (!__any(active)) break;                                      // wave-uniform
        }
        if (live && lane < DP_COLS) {
            if (a.iters) a.iters[t] = iters;
            if (a.res) {
                ((T *)a.res)[2 * t] = res_p;
                ((T *)a.res)[2 * t + 1] = res_d;
            }
        }
    }
}

// PF as resolve_launch_t sets it (fp64 at n = 64 and at 2×2 tiles has no room for a second set of
// per-knot operands), and off at NT = 4 in fp32 as well: with it those four instantiations spill 108 –
// 1092 B per lane, without it only the time-varying 4×2 one does (456 B).  No NT ≤ 2 instantiation
// spills; fp64 NT = 4 spills either way, as in the re-solve (profiles/r14/box/resource_usage.txt).
template <typename T, int NT, int MT, bool TV> constexpr bool box_prefetch()
{
    return !(sizeof(T) == 8 && NT * MT >= 4) && NT < 4;
}

template <typename T>
hipError_t box_launch_t(const DpBoxArgs &a, hipStream_t s)
{
    const unsigned grid = dp_grid(a.batch * ((a.S + DP_COLS - 1) / DP_COLS));
    return with_tiles(a.n, a.m, [&](auto nt, auto mt) {
        return with_bool(a.tv_AB != 0, [&](auto tv) {
            constexpr int NT = decltype(nt)::value, MT = decltype(mt)::value;
            constexpr bool TV = decltype(tv)::value;
            dp_box_kernel<T, NT, MT, TV, box_prefetch<T, NT, MT, TV>()><<<grid, 64, 0, s>>>(a);
            return hipGetLastError();
        });
    });
}

} // namespace

hipError_t dp_box_launch(const DpBoxArgs &a, hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (!dp_resolve_supported(a.n, a.m) || a.N < 2 || a.S < 1) return hipErrorNotSupported;
    if (!a.d || !a.Z || !a.W) return hipErrorInvalidValue;   // d, z, w carry one pass to the next
    if (!(a.rho > 0) || !(a.relax >= 1 && a.relax < 2) || a.max_iter < 1) return hipErrorInvalidValue;
    return a.dtype == 0 ? box_launch_t<double>(a, s) : box_launch_t<float>(a, s);
}

} // namespace lqrx
