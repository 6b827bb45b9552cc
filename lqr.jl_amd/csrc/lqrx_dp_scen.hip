// lqrx_dp_scen.hip — closed-loop rollout of a solved policy (K_k, d_k) over S scenarios per problem
// (lqrx_dp_rollout; include/lqrx.h).  Layout 0 only.
//
// Per problem b and scenario j (trajectory t = b·S + j):
//
//   x_1 = x0_t
//   u_k = min(max(−K_k x_k − α_t d_k, u_lo_b), u_hi_b)
//   x_{k+1} = A_k x_k + B_k u_k + c_k + w_{t,k}
//   J_t = Σ_k (½xᵀQ_k x + uᵀM_k x + ½uᵀR_k u + q_kᵀx + r_kᵀu) + ½x_NᵀQf x_N + qfᵀx_N
//
// With S scenarios the knot is matrix–matrix work: X⁺[n×S] = A·X + B·U + c + W, U[m×S] = −(K·X + d·αᵀ).
//
// dp_scen_kernel (n ≤ 64, m ≤ 32): one wave per (problem, 16 scenarios).  X and U are C-layout tiles
// (lqrx_tile.h) whose columns are the scenarios: register r of such a tile is the B operand of
// k-slice r, so K_k, A_k, B_k (and Q_k, M_k, R_k for the cost) are loaded from global memory in the
// A-operand map — lane l supplies row l&15 and contraction index Tile<T>::row(l, r), sixteen
// consecutive rows of a column-major matrix per k — and every product is a plain MFMA chain: no
// transpose, no LDS.  A column of an MFMA result depends on that column of the B operand alone, so a
// scenario's bits do not depend on S, on its position in the tile, or on what runs in the other
// columns; the columns past S of a last tile run on zeros and are not stored.
//
// dp_scen_wg_kernel (n or m past those tiles, up to 512): one workgroup per (problem, 4 scenarios),
// one wave per scenario, x and u in LDS, matrices from global memory, every element one sequential
// FMA chain.
//
// The cost is a template flag: without J no cost product is issued.  J is summed per lane in double
// for both element types and reduced once after the knot loop in a fixed order.  No atomics, no
// scratch: results are the same bits from run to run and the launch can be captured.
#include "lqrx_internal.h"
#include "lqrx_scen_ops.h"
#include "lqrx_tile.h"

#include <limits>

namespace lqrx {
namespace {

constexpr int SW_COLS = 4;    // scenarios per workgroup of the wg kernel (one wave each)
constexpr int SW_THREADS = 64 * SW_COLS;

__device__ __forceinline__ double fmad(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fmad(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }
__device__ __forceinline__ float clampd(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// D = Mat·Y with the operands loaded where they are used (the cost products: nothing to keep)
template <typename T, int IT, int KT>
__device__ __forceinline__ void mat_mma(typename Tile<T>::acc (&D)[IT], const T *__restrict__ src, int rows, int cols,
                                        const typename Tile<T>::acc (&Y)[KT], int lane)
{
    T op[IT][KT][4];
    op_load<T, IT, KT>(op, src, rows, cols, lane);
#pragma unroll
    for (int it = 0; it < IT; ++it) D[it] = typename Tile<T>::acc{0, 0, 0, 0};
    op_mma<T, IT, KT>(D, op, Y);
}

// jl += Σ over this lane's elements of v · (½·h + g + lin): v the tile of x or u, h its product with
// the symmetric weight (Q·X, R·U), g a cross product (M·X, or null), lin the linear term
template <typename T, int IT>
__device__ __forceinline__ double cost_add(double jl, const typename Tile<T>::acc (&v)[IT],
                                           const typename Tile<T>::acc (&h)[IT],
                                           const typename Tile<T>::acc (*g)[IT],
                                           const typename Tile<T>::acc (&lin)[IT])
{
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double s = fmad(0.5, (double)h[it][r], (double)lin[it][r]);
            if (g) s += (double)(*g)[it][r];
            jl = fmad((double)v[it][r], s, jl);
        }
    return jl;
}

// TV: A, B, c per knot.  COST: J is formed.  PF: K_k (and A_k, B_k with TV) are loaded one knot ahead
// into a second set of registers; without it they are loaded at the top of their own knot.
template <typename T, int NT, int MT, bool TV, bool COST, bool PF>
__global__ __launch_bounds__(64) void dp_scen_kernel(const DpScenArgs a)
{
    using acc = typename Tile<T>::acc;
    const int lane = threadIdx.x, n = a.n, m = a.m, N = a.N;
    const int64_t tiles = (a.S + DP_COLS - 1) / DP_COLS, total = a.batch * tiles;
    const int64_t nn = (int64_t)n * n, nm = (int64_t)n * m, mm = (int64_t)m * m;
    const int64_t kab = TV ? N - 1 : 1, kqr = a.tv_QR ? N - 1 : 1;
    const T inf = std::numeric_limits<T>::infinity();
    for (int64_t wi = blockIdx.x; wi < total; wi += gridDim.x) {
        const int64_t b = wi / tiles, j = (wi - b * tiles) * DP_COLS + tcol(lane);
        const bool live = j < a.S;
        const int64_t t = b * a.S + (live ? j : 0);   // a dead column addresses scenario 0 and selects zero
        const T *Ab = (const T *)a.A + b * nn * kab, *Bb = (const T *)a.B + b * nm * kab;
        const T *Kb = (const T *)a.K + b * nm * (N - 1);
        const T *cb = a.c ? (const T *)a.c + b * n * kab : nullptr;
        const T *db = a.d ? (const T *)a.d + b * m * (N - 1) : nullptr;
        const T *wt = a.w ? (const T *)a.w + t * (N - 1) * n : nullptr;
        T *Xt = a.X ? (T *)a.X + t * N * n : nullptr;
        T *Ut = a.U ? (T *)a.U + t * (N - 1) * m : nullptr;
        const T al = a.alpha ? ((const T *)a.alpha)[t] : T(1);

        acc lo[MT], hi[MT];
#pragma unroll
        for (int it = 0; it < MT; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = it * 16 + Tile<T>::row(lane, r);
                const bool ok = row < m;
                const T l = a.u_lo ? ((const T *)a.u_lo)[b * m + (ok ? row : 0)] : -inf;
                const T h = a.u_hi ? ((const T *)a.u_hi)[b * m + (ok ? row : 0)] : inf;
                lo[it][r] = ok ? l : -inf;
                hi[it][r] = ok ? h : inf;
            }

        acc X[NT], U[MT];
        rows_load<T, NT>(X, (const T *)a.x0 + t * n, n, lane, live);
        if (Xt) rows_store<T, NT>(X, Xt, n, lane, live);

        T Kc[MT][NT][4], Ac[NT][NT][4], Bc[NT][MT][4];
        if (PF || !TV) {
            op_load<T, NT, NT>(Ac, Ab, n, n, lane);
            op_load<T, NT, MT>(Bc, Bb, n, m, lane);
        }
        if (PF) op_load<T, MT, NT>(Kc, Kb, m, n, lane);
        double jl = 0.0;

        for (int k = 0; k < N - 1; ++k) {   // knot k + 1 of the header: u_{k+1}, x_{k+2}
            T Kn[MT][NT][4], An[NT][NT][4], Bn[NT][MT][4];
            if (PF) {   // the next knot's operands (the last knot loads itself again: unconditional loads)
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
            // U = clamp(−(K·X + d·αᵀ))
            rows_load<T, MT>(U, db ? db + (int64_t)k * m : nullptr, m, lane);
#pragma unroll
            for (int it = 0; it < MT; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) U[it][r] = al * U[it][r];
            op_mma<T, MT, NT>(U, Kc, X);
#pragma unroll
            for (int it = 0; it < MT; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) U[it][r] = clampd(-U[it][r], lo[it][r], hi[it][r]);
            if (Ut) rows_store<T, MT>(U, Ut + (int64_t)k * m, m, lane, live);

            if (COST) {
                const int64_t kq = a.tv_QR ? k : 0;
                const int64_t cq = b * kqr + kq;
                acc QX[NT], RU[MT], MX[MT], ql[NT], rl[MT];
                mat_mma<T, NT, NT>(QX, (const T *)a.Q + cq * nn, n, n, X, lane);
                mat_mma<T, MT, MT>(RU, (const T *)a.R + cq * mm, m, m, U, lane);
                rows_load<T, NT>(ql, a.q ? (const T *)a.q + cq * n : nullptr, n, lane);
                rows_load<T, MT>(rl, a.r ? (const T *)a.r + cq * m : nullptr, m, lane);
                jl = cost_add<T, NT>(jl, X, QX, nullptr, ql);
                if (a.M) {
                    mat_mma<T, MT, NT>(MX, (const T *)a.M + cq * nm, m, n, X, lane);
                    jl = cost_add<T, MT>(jl, U, RU, &MX, rl);
                } else {
                    jl = cost_add<T, MT>(jl, U, RU, nullptr, rl);
                }
            }

            // X⁺ = c + w + A·X + B·U
            acc Xn[NT], wv[NT];
            rows_load<T, NT>(Xn, cb ? cb + (TV ? (int64_t)k * n : 0) : nullptr, n, lane);
            rows_load<T, NT>(wv, wt ? wt + (int64_t)k * n : nullptr, n, lane, live);
#pragma unroll
            for (int it = 0; it < NT; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) Xn[it][r] = Xn[it][r] + wv[it][r];
            op_mma<T, NT, NT>(Xn, Ac, X);
            op_mma<T, NT, MT>(Xn, Bc, U);
#pragma unroll
            for (int it = 0; it < NT; ++it) X[it] = Xn[it];
            if (Xt) rows_store<T, NT>(X, Xt + (int64_t)(k + 1) * n, n, lane, live);

            if (PF) {
                op_copy<T, MT, NT>(Kc, Kn);
                if (TV) {
                    op_copy<T, NT, NT>(Ac, An);
                    op_copy<T, NT, MT>(Bc, Bn);
                }
            }
        }

        if (COST) {
            acc QX[NT], ql[NT];
            mat_mma<T, NT, NT>(QX, (const T *)a.Qf + b * nn, n, n, X, lane);
            rows_load<T, NT>(ql, a.qf ? (const T *)a.qf + b * n : nullptr, n, lane);
            jl = cost_add<T, NT>(jl, X, QX, nullptr, ql);
            // the four lane groups that share a column, in a fixed order
            jl += __shfl_xor(jl, 16);
            jl += __shfl_xor(jl, 32);
            if (live && lane < DP_COLS) ((T *)a.J)[t] = (T)jl;
        }
    }
}

// ---- past the register tiles: a workgroup per (problem, SW_COLS scenarios), a wave per scenario ----
// Lane i of the wave owns rows i, i + 64, … of u, x⁺ and the cost products: consecutive lanes read
// consecutive addresses of a column of the column-major matrices, and every element is one FMA chain
// over the contraction index in ascending order.  x_k, x_{k+1} and u_k of the wave's scenario sit in LDS.
template <typename T, bool COST>
__global__ __launch_bounds__(SW_THREADS) void dp_scen_wg_kernel(const DpScenArgs a)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, m = a.m, N = a.N;
    T *xs = reinterpret_cast<T *>(smem_raw) + (size_t)wave * (2 * n + m);
    T *xn = xs + n;
    T *us = xs + 2 * n;
    const int64_t tiles = (a.S + SW_COLS - 1) / SW_COLS, total = a.batch * tiles;
    const int64_t nn = (int64_t)n * n, nm = (int64_t)n * m, mm = (int64_t)m * m;
    const int64_t kab = a.tv_AB ? N - 1 : 1, kqr = a.tv_QR ? N - 1 : 1;
    const T inf = std::numeric_limits<T>::infinity();
    for (int64_t wi = blockIdx.x; wi < total; wi += gridDim.x) {
        const int64_t b = wi / tiles, j = (wi - b * tiles) * SW_COLS + wave;
        const bool live = j < a.S;   // a dead wave runs scenario 0 on zeros (the barriers stay uniform)
        const int64_t t = b * a.S + (live ? j : 0);
        const T *Ab = (const T *)a.A + b * nn * kab, *Bb = (const T *)a.B + b * nm * kab;
        const T *Kb = (const T *)a.K + b * nm * (N - 1);
        const T *cb = a.c ? (const T *)a.c + b * n * kab : nullptr;
        const T *db = a.d ? (const T *)a.d + b * m * (N - 1) : nullptr;
        const T *wt = (a.w && live) ? (const T *)a.w + t * (N - 1) * n : nullptr;
        const T *ulo = a.u_lo ? (const T *)a.u_lo + b * m : nullptr;
        const T *uhi = a.u_hi ? (const T *)a.u_hi + b * m : nullptr;
        T *Xt = (a.X && live) ? (T *)a.X + t * N * n : nullptr;
        T *Ut = (a.U && live) ? (T *)a.U + t * (N - 1) * m : nullptr;
        const T al = a.alpha ? ((const T *)a.alpha)[t] : T(1);
        T *xc = xs, *xx = xn;
        for (int i = lane; i < n; i += 64) {
            const T v = live ? ((const T *)a.x0)[t * n + i] : T(0);
            xc[i] = v;
            if (Xt) Xt[i] = v;
        }
        __syncthreads();
        double jl = 0.0;
        for (int k = 0; k < N - 1; ++k) {
            const T *Ak = Ab + (a.tv_AB ? k * nn : 0), *Bk = Bb + (a.tv_AB ? k * nm : 0), *Kk = Kb + k * nm;
            const T *ck = cb ? cb + (a.tv_AB ? (int64_t)k * n : 0) : nullptr;
            const T *dk = db ? db + (int64_t)k * m : nullptr;
            for (int i = lane; i < m; i += 64) {
                T s = al * (dk ? dk[i] : T(0));
                for (int l = 0; l < n; ++l) s = fmad(Kk[i + (int64_t)l * m], xc[l], s);
                const T u = clampd(-s, ulo ? ulo[i] : -inf, uhi ? uhi[i] : inf);
                us[i] = u;
                if (Ut) Ut[(int64_t)k * m + i] = u;
            }
            __syncthreads();
            if (COST) {
                const int64_t cq = b * kqr + (a.tv_QR ? k : 0);
                const T *Qk = (const T *)a.Q + cq * nn, *Rk = (const T *)a.R + cq * mm;
                const T *Mk = a.M ? (const T *)a.M + cq * nm : nullptr;
                const T *qk = a.q ? (const T *)a.q + cq * n : nullptr, *rk = a.r ? (const T *)a.r + cq * m : nullptr;
                for (int i = lane; i < n; i += 64) {
                    T h = T(0);
                    for (int l = 0; l < n; ++l) h = fmad(Qk[i + (int64_t)l * n], xc[l], h);
                    jl = fmad((double)xc[i], fmad(0.5, (double)h, qk ? (double)qk[i] : 0.0), jl);
                }
                for (int i = lane; i < m; i += 64) {
                    T h = T(0), g = T(0);
                    for (int l = 0; l < m; ++l) h = fmad(Rk[i + (int64_t)l * m], us[l], h);
                    if (Mk)
                        for (int l = 0; l < n; ++l) g = fmad(Mk[i + (int64_t)l * m], xc[l], g);
                    jl = fmad((double)us[i], fmad(0.5, (double)h, rk ? (double)rk[i] : 0.0) + (double)g, jl);
                }
            }
            for (int i = lane; i < n; i += 64) {
                T s = (ck ? ck[i] : T(0)) + (wt ? wt[(int64_t)k * n + i] : T(0));
                for (int l = 0; l < n; ++l) s = fmad(Ak[i + (int64_t)l * n], xc[l], s);
                for (int l = 0; l < m; ++l) s = fmad(Bk[i + (int64_t)l * n], us[l], s);
                xx[i] = s;
                if (Xt) Xt[(int64_t)(k + 1) * n + i] = s;
            }
            __syncthreads();
            T *sw = xc;
            xc = xx;
            xx = sw;
        }
        if (COST) {
            const T *Qk = (const T *)a.Qf + b * nn;
            const T *qk = a.qf ? (const T *)a.qf + b * n : nullptr;
            for (int i = lane; i < n; i += 64) {
                T h = T(0);
                for (int l = 0; l < n; ++l) h = fmad(Qk[i + (int64_t)l * n], xc[l], h);
                jl = fmad((double)xc[i], fmad(0.5, (double)h, qk ? (double)qk[i] : 0.0), jl);
            }
            for (int o = 32; o >= 1; o >>= 1) jl += __shfl_xor(jl, o);
            if (live && lane == 0) ((T *)a.J)[t] = (T)jl;
        }
        __syncthreads();
    }
}

template <typename T>
hipError_t scen_launch_t(const DpScenArgs &a, hipStream_t s)
{
    const int n = a.n, m = a.m;
    if (n <= 64 && m <= 32) {
        const unsigned grid = dp_grid(a.batch * ((a.S + DP_COLS - 1) / DP_COLS));
        return with_tiles(n, m, [&](auto nt, auto mt) {
            return with_bools(a.tv_AB != 0, a.J != nullptr, [&](auto tv, auto cost) {
                constexpr int NT = decltype(nt)::value, MT = decltype(mt)::value;
                constexpr bool TV = decltype(tv)::value, COST = decltype(cost)::value;
                // n = 64 in fp64: A and B alone are 192 VGPRs; a second set of per-knot operands does not fit
                constexpr bool PF = !(sizeof(T) == 8 && NT == 4);
                dp_scen_kernel<T, NT, MT, TV, COST, PF><<<grid, 64, 0, s>>>(a);
                return hipGetLastError();
            });
        });
    }
    const unsigned grid = dp_grid(a.batch * ((a.S + SW_COLS - 1) / SW_COLS));
    const size_t lds = (size_t)SW_COLS * (2 * (size_t)n + m) * sizeof(T);   // ≤ 49 152 B (n = m = 512, fp64)
    if (a.J)
        dp_scen_wg_kernel<T, true><<<grid, SW_THREADS, lds, s>>>(a);
    else
        dp_scen_wg_kernel<T, false><<<grid, SW_THREADS, lds, s>>>(a);
    return hipGetLastError();
}

} // namespace

hipError_t dp_scen_launch(const DpScenArgs &a, hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (a.n < 1 || a.m < 1 || a.n > 512 || a.m > 512 || a.N < 2 || a.S < 1) return hipErrorNotSupported;
    return a.dtype == 0 ? scen_launch_t<double>(a, s) : scen_launch_t<float>(a, s);
}

} // namespace lqrx
