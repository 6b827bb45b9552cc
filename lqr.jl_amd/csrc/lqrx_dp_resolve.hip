// lqrx_dp_resolve.hip — factor once, re-solve S right-hand sides per problem (lqrx_dp_factor,
// lqrx_dp_resolve; include/lqrx.h).  Layout 0 only, n ≤ 64, m ≤ 32.
//
// P_k, K_k and E_k = R_k + B_kᵀP_{k+1}B_k of a solve do not depend on q, r, qf, x0.  With K_k, E_k⁻¹ and
// g_k = P_{k+1}c_k kept per problem, a right-hand side (q, r, qf, x0) needs only vector recursions:
//
//   p_N = qf
//   p̃   = p_{k+1} + g_k          h_k = r_k + B_kᵀp̃          d_k = E_k⁻¹h_k
//   p_k = q_k + A_kᵀp̃ − K_kᵀh_k                                       k = N−1 … 1
//   x_1 = x0,  u_k = −K_k x_k − d_k,  x_{k+1} = A_k x_k + B_k u_k + c_k  k = 1 … N−1
//
// (Gᵀd = GᵀE⁻¹h = Kᵀh, E symmetric: no cost matrix is read, the cross term lives in K.)
//
// dp_resolve_kernel: one wave per (problem, 16 right-hand sides), the grid of dp_scen_kernel.  p, h, d
// are C-layout tiles whose columns are the right-hand sides.  The backward pass multiplies by Aᵀ, Bᵀ,
// Kᵀ and the symmetric E⁻¹: a matrix loaded as plain C-layout tiles (tiles_load, coalesced along its
// columns) is the A operand of its transpose (lqrx_tile.h), so all four products are TN chains — no
// transpose, no LDS, no strided load.  Aᵀp̃ shares its B operand with Bᵀp̃ and −Kᵀh with E⁻¹h, so each
// pair is issued interleaved: the products into p_k fill the waits of the h → d chain.  The forward
// pass is the scenario rollout's (lqrx_scen_ops.h) with a d per right-hand side.  d_{t,k} is written
// from the C layout in the backward pass and read back in the forward pass by the same lane at the
// same address, so program order alone makes it visible: no fence.  A column of an MFMA result
// depends on that column of the B operand alone, so a right-hand side's bits do not depend on S, on
// its position, or on which outputs are stored; the columns past S of a last tile run on zeros.
//
// dp_factor_kernel: one workgroup per problem, the knots in descending order on the workgroup
// routines of lqrx_wg.h: P_{k+1}B and E on the MFMA pipe, wg_potrf, and E⁻¹ = U⁻¹U⁻ᵀ by the two
// triangular solves on an identity, all in LDS.  A pivot that is not positive reports the knot (the
// first one met is the largest k) and that knot's E⁻¹ is written as zeros.  No atomics in either
// kernel: the same bits from run to run.
#include "lqrx_internal.h"
#include "lqrx_resolve_ops.h"
#include "lqrx_scen_ops.h"
#include "lqrx_tile.h"
#include "lqrx_wg.h"

namespace lqrx {
namespace {

// TV: A, B, c per knot.  PF: the next knot's K_k, E_k⁻¹ (A_k, B_k with TV) and vectors are loaded one
// knot ahead into a second set of registers; without it they are loaded at the top of their own knot.
template <typename T, int NT, int MT, bool TV, bool PF>
__global__ __launch_bounds__(64) void dp_resolve_kernel(const DpResolveArgs a)
{
    using acc = typename Tile<T>::acc;
    const int lane = threadIdx.x, n = a.n, m = a.m, N = a.N;
    const int64_t tiles = (a.S + DP_COLS - 1) / DP_COLS, total = a.batch * tiles;
    const int64_t nn = (int64_t)n * n, nm = (int64_t)n * m, mm = (int64_t)m * m;
    const int64_t kab = TV ? N - 1 : 1, kqr = a.tv_QR ? N - 1 : 1, kp = a.p_all ? N : 1;
    for (int64_t wi = blockIdx.x; wi < total; wi += gridDim.x) {
        const int64_t b = wi / tiles, j = (wi - b * tiles) * DP_COLS + tcol(lane);
        const bool live = j < a.S;
        const int64_t t = b * a.S + (live ? j : 0);   // a dead column addresses right-hand side 0 and selects zero
        const T *Ab = (const T *)a.A + b * nn * kab, *Bb = (const T *)a.B + b * nm * kab;
        const T *Kb = (const T *)a.K + b * nm * (N - 1), *Eb = (const T *)a.Einv + b * mm * (N - 1);
        const T *gb = a.Pc ? (const T *)a.Pc + b * n * (N - 1) : nullptr;
        const T *cb = a.c ? (const T *)a.c + b * n * kab : nullptr;
        const T *qt = a.q ? (const T *)a.q + t * kqr * n : nullptr;
        const T *rt = a.r ? (const T *)a.r + t * kqr * m : nullptr;
        T *dt = a.d ? (T *)a.d + t * (N - 1) * m : nullptr;
        T *pt = a.p ? (T *)a.p + t * kp * n : nullptr;
        T *Xt = a.X ? (T *)a.X + t * N * n : nullptr;
        T *Ut = a.U ? (T *)a.U + t * (N - 1) * m : nullptr;
        const auto qk = [&](int k) { return qt ? qt + (a.tv_QR ? (int64_t)k * n : 0) : nullptr; };
        const auto rk = [&](int k) { return rt ? rt + (a.tv_QR ? (int64_t)k * m : 0) : nullptr; };
        const auto gk = [&](int k) { return gb ? gb + (int64_t)k * n : nullptr; };

        // ---- backward: p_N = qf, then knots N−1 … 1 (k = N−2 … 0 here) ----
        {
            acc p[NT];
            rows_load<T, NT>(p, a.qf ? (const T *)a.qf + t * n : nullptr, n, lane, live);
            if (pt && a.p_all) rows_store<T, NT>(p, pt + (int64_t)(N - 1) * n, n, lane, live);

            acc At[NT][NT], Bt[NT][MT], Kt[MT][NT], Et[MT][MT], qv[NT], rv[MT], gv[NT];
            if (PF || !TV) {
                const int64_t k0 = TV ? N - 2 : 0;
                tiles_load<T, NT, NT>(At, Ab + k0 * nn, n, n, n, lane, false);
                tiles_load<T, NT, MT>(Bt, Bb + k0 * nm, n, m, n, lane, false);
            }
            if (PF) {
                tiles_load<T, MT, NT>(Kt, Kb + (int64_t)(N - 2) * nm, m, n, m, lane, false);
                tiles_load<T, MT, MT>(Et, Eb + (int64_t)(N - 2) * mm, m, m, m, lane, false);
                rows_load<T, NT>(qv, qk(N - 2), n, lane, live);
                rows_load<T, MT>(rv, rk(N - 2), m, lane, live);
                rows_load<T, NT>(gv, gk(N - 2), n, lane);
            }
            for (int k = N - 2; k >= 0; --k) {
                acc An[NT][NT], Bn[NT][MT], Kn[MT][NT], En[MT][MT], qn[NT], rn[MT], gn[NT];
                if (PF) {   // the next knot's operands (the last knot loads itself again: unconditional loads)
                    const int k1 = k > 0 ? k - 1 : 0;
                    tiles_load<T, MT, NT>(Kn, Kb + (int64_t)k1 * nm, m, n, m, lane, false);
                    tiles_load<T, MT, MT>(En, Eb + (int64_t)k1 * mm, m, m, m, lane, false);
                    if (TV) {
                        tiles_load<T, NT, NT>(An, Ab + (int64_t)k1 * nn, n, n, n, lane, false);
                        tiles_load<T, NT, MT>(Bn, Bb + (int64_t)k1 * nm, n, m, n, lane, false);
                    }
                    rows_load<T, NT>(qn, qk(k1), n, lane, live);
                    rows_load<T, MT>(rn, rk(k1), m, lane, live);
                    rows_load<T, NT>(gn, gk(k1), n, lane);
                } else {
                    tiles_load<T, MT, NT>(Kt, Kb + (int64_t)k * nm, m, n, m, lane, false);
                    tiles_load<T, MT, MT>(Et, Eb + (int64_t)k * mm, m, m, m, lane, false);
                    if (TV) {
                        tiles_load<T, NT, NT>(At, Ab + (int64_t)k * nn, n, n, n, lane, false);
                        tiles_load<T, NT, MT>(Bt, Bb + (int64_t)k * nm, n, m, n, lane, false);
                    }
                    rows_load<T, NT>(qv, qk(k), n, lane, live);
                    rows_load<T, MT>(rv, rk(k), m, lane, live);
                    rows_load<T, NT>(gv, gk(k), n, lane);
                }
                // p̃ = p + g;  h = r + Bᵀp̃ with p_k = q + Aᵀp̃ alongside
                acc ph[NT], h[MT], pn[NT], d[MT];
#pragma unroll
                for (int it = 0; it < NT; ++it) ph[it] = p[it] + gv[it];
                vec_copy<T, MT>(h, rv);
                vec_copy<T, NT>(pn, qv);
                tn_pair<T, NT, MT, NT, false>(h, Bt, pn, At, ph);
                // d = E⁻¹h with p_k −= Kᵀh alongside
#pragma unroll
                for (int it = 0; it < MT; ++it) d[it] = acc{0, 0, 0, 0};
                tn_pair<T, MT, MT, NT, true>(d, Et, pn, Kt, h);
                if (dt) d_store<T, MT>(d, dt + (int64_t)k * m, m, lane, live);
                vec_copy<T, NT>(p, pn);
                if (pt && (a.p_all || k == 0)) rows_store<T, NT>(p, pt + (a.p_all ? (int64_t)k * n : 0), n, lane, live);

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
                }
            }
        }
        if (!Xt && !Ut) continue;   // uniform: kernel arguments

        // ---- forward: the rollout with this right-hand side's d (the launcher has checked that d is there) ----
        acc X[NT], U[MT];
        rows_load<T, NT>(X, a.x0 ? (const T *)a.x0 + t * n : nullptr, n, lane, live);
        if (Xt) rows_store<T, NT>(X, Xt, n, lane, live);
        T Kc[MT][NT][4], Ac[NT][NT][4], Bc[NT][MT][4];
        if (PF || !TV) {
            op_load<T, NT, NT>(Ac, Ab, n, n, lane);
            op_load<T, NT, MT>(Bc, Bb, n, m, lane);
        }
        if (PF) op_load<T, MT, NT>(Kc, Kb, m, n, lane);
        for (int k = 0; k < N - 1; ++k) {
            T Kn[MT][NT][4], An[NT][NT][4], Bn[NT][MT][4];
            if (PF) {
                const int k1 = k + 1 < N - 1 ? k + 1 : k;
                op_load<T, MT, NT>(Kn, Kb + k1 * nm, m, n, lane);
                if (TV) {
                    op_load<T, NT, NT>(An, Ab + k1 * nn, n, n, lane);
                    op_load<T, NT, MT>(Bn, Bb + k1 * nm, n, m, lane);
                }
            } else {
                op_load<T, MT, NT>(Kc, Kb + k * nm, m, n, lane);
                if (TV) {
                    op_load<T, NT, NT>(Ac, Ab + k * nn, n, n, lane);
                    op_load<T, NT, MT>(Bc, Bb + k * nm, n, m, lane);
                }
            }
            // U = −(K·X + d)
            d_load<T, MT>(U, dt + (int64_t)k * m, m, lane, live);
            op_mma<T, MT, NT>(U, Kc, X);
#pragma unroll
            for (int it = 0; it < MT; ++it) U[it] = -U[it];
            if (Ut) rows_store<T, MT>(U, Ut + (int64_t)k * m, m, lane, live);
            // X⁺ = c + A·X + B·U
            acc Xn[NT];
            rows_load<T, NT>(Xn, cb ? cb + (TV ? (int64_t)k * n : 0) : nullptr, n, lane);
            op_mma<T, NT, NT>(Xn, Ac, X);
            op_mma<T, NT, MT>(Xn, Bc, U);
            vec_copy<T, NT>(X, Xn);
            if (Xt) rows_store<T, NT>(X, Xt + (int64_t)(k + 1) * n, n, lane, live);
            if (PF) {
                op_copy<T, MT, NT>(Kc, Kn);
                if (TV) {
                    op_copy<T, NT, NT>(Ac, An);
                    op_copy<T, NT, MT>(Bc, Bn);
                }
            }
        }
    }
}

// One workgroup per problem; per knot k = N−1 … 1 (1-based): PB = P_{k+1}B_k, E = R_k + B_kᵀPB,
// Pc = P_{k+1}c_k, E = UᵀU, E⁻¹ = U⁻¹(U⁻ᵀI).  PB (n×m), E and the identity (m×m each) live in LDS.
template <typename T>
__global__ __launch_bounds__(wg::BT) void dp_factor_kernel(const DpFactorArgs a)
{
    using wg::Mat;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    __shared__ int s_info;
    const int tid = threadIdx.x, n = a.n, m = a.m, N = a.N;
    const size_t nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
    T *PB = reinterpret_cast<T *>(smem_raw), *E = PB + nm, *X = E + mm;
    const size_t kab = a.tv_AB ? N - 1 : 1, kqr = a.tv_QR ? N - 1 : 1;
    for (int64_t b = blockIdx.x; b < a.batch; b += gridDim.x) {
        const T *Pb = (const T *)a.P + (size_t)b * nn * N;
        const T *Bb = (const T *)a.B + (size_t)b * nm * kab, *Rb = (const T *)a.R + (size_t)b * mm * kqr;
        const T *cb = a.c ? (const T *)a.c + (size_t)b * n * kab : nullptr;
        T *Eo = (T *)a.Einv + (size_t)b * mm * (N - 1);
        T *go = a.Pc ? (T *)a.Pc + (size_t)b * n * (N - 1) : nullptr;
        if (tid == 0) s_info = 0;
        __syncthreads();
        for (int k = N - 1; k >= 1; --k) {
            const T *P = Pb + (size_t)k * nn;   // P_{k+1}: knot k + 1 of the p_mode = 1 array sits at index k
            const T *B = Bb + (a.tv_AB ? (size_t)(k - 1) * nm : 0), *R = Rb + (a.tv_QR ? (size_t)(k - 1) * mm : 0);
            const Mat<T> Pt{P, (size_t)n, 1}, Bm{B, 1, (size_t)n}, PBm{PB, 1, (size_t)n}, none{nullptr, 0, 0};
            wg::wg_mm<T, 1, 1>(PB, n, n, m, nullptr, Pt, Bm, n, none, none, 0, tid);
            if (go) {
                const T *c = cb + (a.tv_AB ? (size_t)(k - 1) * n : 0);
                for (int i = tid; i < n; i += wg::BT) {
                    T s = 0;
                    for (int l = 0; l < n; ++l) s = fma(P[i + (size_t)l * n], c[l], s);
                    go[(size_t)(k - 1) * n + i] = s;
                }
            }
            for (int e = tid; e < (int)mm; e += wg::BT) X[e] = (e % m == e / m) ? T(1) : T(0);
            __syncthreads();
            wg::wg_mm<T, 1, 1>(E, m, m, m, R, Bm, PBm, n, none, none, 0, tid);
            __syncthreads();
            const int f = wg::wg_potrf<T>(E, m, m, tid);        // uniform over the workgroup
            T *Ek = Eo + (size_t)(k - 1) * mm;
            if (f) {   // E_k is not positive definite: the first knot met is the largest k; E_k⁻¹ is written as zeros
                if (tid == 0 && s_info == 0) s_info = k;
                for (int e = tid; e < (int)mm; e += wg::BT) Ek[e] = T(0);
            } else {
                wg::wg_trsm_ut<T>(E, m, m, X, m, m, tid);
                wg::wg_trsm_un<T>(E, m, m, X, m, m, tid);
                for (int e = tid; e < (int)mm; e += wg::BT) {   // exactly symmetric
                    const int i = e % m, jj = e / m;
                    Ek[e] = T(0.5) * (X[i + jj * m] + X[jj + i * m]);
                }
            }
            __syncthreads();
        }
        if (tid == 0 && a.info) a.info[b] = s_info;
        __syncthreads();
    }
}

template <typename T>
hipError_t resolve_launch_t(const DpResolveArgs &a, hipStream_t s)
{
    const unsigned grid = dp_grid(a.batch * ((a.S + DP_COLS - 1) / DP_COLS));
    return with_tiles(a.n, a.m, [&](auto nt, auto mt) {
        return with_bool(a.tv_AB != 0, [&](auto tv) {
            constexpr int NT = decltype(nt)::value, MT = decltype(mt)::value;
            constexpr bool TV = decltype(tv)::value;
            // fp64 at n = 64 (A alone is 128 VGPRs in either operand form) and at 2×2 tiles: a second set
            // of per-knot operands does not fit without spilling
            constexpr bool PF = !(sizeof(T) == 8 && NT * MT >= 4);
            dp_resolve_kernel<T, NT, MT, TV, PF><<<grid, 64, 0, s>>>(a);
            return hipGetLastError();
        });
    });
}

template <typename T>
hipError_t factor_launch_t(const DpFactorArgs &a, hipStream_t s)
{
    const size_t lds = ((size_t)a.n * a.m + 2 * (size_t)a.m * a.m) * sizeof(T);   // ≤ 32 768 B (n = 64, m = 32, fp64)
    dp_factor_kernel<T><<<dp_grid(a.batch), wg::BT, lds, s>>>(a);
    return hipGetLastError();
}

} // namespace

bool dp_resolve_supported(int n, int m) { return n >= 1 && m >= 1 && n <= 64 && m <= 32; }

hipError_t dp_resolve_launch(const DpResolveArgs &a, hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (!dp_resolve_supported(a.n, a.m) || a.N < 2 || a.S < 1) return hipErrorNotSupported;
    if ((a.X || a.U) && !a.d) return hipErrorInvalidValue;   // d carries the backward pass to the forward one
    return a.dtype == 0 ? resolve_launch_t<double>(a, s) : resolve_launch_t<float>(a, s);
}

hipError_t dp_factor_launch(const DpFactorArgs &a, hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (!dp_resolve_supported(a.n, a.m) || a.N < 2) return hipErrorNotSupported;
    if ((a.c == nullptr) != (a.Pc == nullptr)) return hipErrorInvalidValue;
    return a.dtype == 0 ? factor_launch_t<double>(a, s) : factor_launch_t<float>(a, s);
}

} // namespace lqrx
