// lqrx_dp_adjoint.hip — costates of a DP solve and the rank-2 assembly of the adjoint pass
// (lqrx_dp_costates, lqrx_dp_solve_adjoint; include/lqrx.h).  Layout 0 only.
//
// The textbook sweep λ_k = Q_k x_k + M_kᵀu_k + q_k + A_kᵀλ_{k+1} propagates rounding errors with the
// open-loop Aᵀ: with ρ(A) = 1.14 and N = 256 it loses eleven digits.  Adding K_kᵀ times the
// stationarity condition s_k = R_k u_k + M_k x_k + r_k + B_kᵀλ_{k+1} = 0 gives the same λ through the
// closed loop, which the solve made stable:
//
//   λ_N = Qf x_N + qf
//   λ_k = g̃_k + A_kᵀλ_{k+1} − K_kᵀ(B_kᵀλ_{k+1})
//   g̃_k = Q_k x_k + M_kᵀu_k + q_k − K_kᵀ(R_k u_k + M_k x_k + r_k)
//
// g̃_k does not depend on the chain, so the sweep is two kernels: dp_costate_g_kernel writes every
// g̃_k (and λ_N) into lam, one workgroup per (trajectory, knot); dp_costate_kernel then runs the
// serial part in place, one workgroup per trajectory (one wave for n ≤ 64).
// dp_grad_kernel (per-knot outputs) and dp_grad_sum_kernel (outputs summed over the knots) form the
// outer products.  Plain HIP: no atomics, every sum in a fixed order, so results are the same bits
// from run to run.
#include "lqrx_internal.h"

namespace lqrx {
namespace {

constexpr int CS_WAVE = 64;   // threads of the one-wave costate kernels (n ≤ 64)
constexpr int CS_WG = 256;    // threads of the workgroup kernels

__device__ inline int pow2_width(int rows)
{
    // smallest power of two ≥ rows, capped at the wave width: the lanes that stride a column
    int w = 1;
    while (w < rows && w < 64) w <<= 1;
    return w;
}

// ---- g̃_k (k < N) and λ_N = Qf x_N + qf, one workgroup per (b, k) ----
// s0 = R_k u_k + M_k x_k + r_k first (thread i owns row i of R and M: consecutive threads read
// consecutive addresses), then thread j owns row j of Q (read along its rows) and dots column j of M
// with u and column j of K with s0: a column is contiguous per thread and, over the wave, one
// contiguous block.  x, u and s0 sit in LDS.
template <typename T>
__global__ void dp_costate_g_kernel(const T *__restrict__ Q, const T *__restrict__ R, const T *__restrict__ M,
                                    const T *__restrict__ Qf, const T *__restrict__ q, const T *__restrict__ r,
                                    const T *__restrict__ qf, const T *__restrict__ K, const T *__restrict__ X,
                                    const T *__restrict__ U, T *__restrict__ lam, int n, int m, int N, int tv_QR,
                                    int64_t batch)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T *xs = reinterpret_cast<T *>(smem_raw);
    T *us = xs + n;
    T *ss = us + m;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t total = batch * (int64_t)N;
    const int64_t kq = tv_QR ? N - 1 : 1;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const int64_t b = w / N;
        const int kk = (int)(w - b * N);   // 0-based knot
        const bool last = kk == N - 1;
        const T *xk = X + (b * N + kk) * n;
        for (int i = tid; i < n; i += nt) xs[i] = xk[i];
        if (!last) {
            const T *uk = U + (b * (N - 1) + kk) * m;
            for (int i = tid; i < m; i += nt) us[i] = uk[i];
        }
        __syncthreads();
        const int64_t kidx = b * kq + (tv_QR ? kk : 0);
        const T *Mk = (!last && M) ? M + kidx * m * n : nullptr;
        if (!last) {
            const T *Rk = R + kidx * m * m;
            const T *rk = r ? r + kidx * m : nullptr;
            for (int i = tid; i < m; i += nt) {
                T acc = rk ? rk[i] : T(0);
                for (int l = 0; l < m; ++l) acc += Rk[i + (int64_t)l * m] * us[l];
                if (Mk)
                    for (int l = 0; l < n; ++l) acc += Mk[i + (int64_t)l * m] * xs[l];
                ss[i] = acc;
            }
            __syncthreads();
        }
        const T *Qk = last ? Qf + b * n * n : Q + kidx * n * n;
        const T *qk = last ? (qf ? qf + b * n : nullptr) : (q ? q + kidx * n : nullptr);
        const T *Kk = last ? nullptr : K + (b * (N - 1) + kk) * m * n;
        for (int j = tid; j < n; j += nt) {
            T acc = qk ? qk[j] : T(0);
            for (int i = 0; i < n; ++i) acc += Qk[j + (int64_t)i * n] * xs[i];
            if (Mk) {
                const T *col = Mk + (int64_t)j * m;
                for (int i = 0; i < m; ++i) acc += col[i] * us[i];
            }
            if (Kk) {
                const T *col = Kk + (int64_t)j * m;
                T kt = T(0);
                for (int i = 0; i < m; ++i) kt += col[i] * ss[i];
                acc -= kt;
            }
            lam[(b * N + kk) * n + j] = acc;
        }
        __syncthreads();
    }
}

// ---- the chain, n ≤ 64: one wave per trajectory, A in LDS ----
// lam holds g̃_k (k < N) and λ_N.  A_k is staged into LDS with coalesced loads at an odd column
// stride S (thread j reads column j: its ds_read_b64 addresses then fall on distinct banks), a
// time-invariant A once, a time-varying one per knot through PF registers per thread: knot k−1's
// loads are issued before knot k's dot products and land in LDS after them, so their HBM latency
// hides under the chain step.  PF·64 ≥ n².  The columns of B_k and K_k (n·m each, at most half of
// A) are read from global, contiguous per thread; w = B_kᵀλ_{k+1} goes through LDS.
template <typename T, int PF>
__global__ __launch_bounds__(CS_WAVE) void dp_costate_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                              const T *__restrict__ K, T *__restrict__ lam, int n,
                                                              int m, int N, int tv_AB, int64_t batch)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int S = n | 1;
    T *As = reinterpret_cast<T *>(smem_raw);   // n columns of stride S
    T *ls = As + (size_t)n * S;                 // λ, two buffers of n
    T *ws = ls + 2 * n;                         // w = Bᵀλ, m
    const int tid = threadIdx.x;
    const int nn = n * n;
    // (row, column) of this thread's e-th staged element, idx = tid + 64·e, advanced without a division
    const int r0 = tid % n, c0 = tid / n, dr = CS_WAVE % n, dc = CS_WAVE / n;
    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        T *L = lam + b * (int64_t)N * n;
        const T *Ab = A + b * (int64_t)nn * (tv_AB ? N - 1 : 1);
        const T *Bb = B + b * (int64_t)n * m * (tv_AB ? N - 1 : 1);
        const T *Kb = K + b * (int64_t)m * n * (N - 1);
        T pf[PF];
        auto fetch = [&](const T *Ak) {
#pragma unroll
            for (int e = 0; e < PF; ++e) {
                const int idx = tid + e * CS_WAVE;
                if (idx < nn) pf[e] = Ak[idx];
            }
        };
        auto stage = [&]() {
            int r = r0, c = c0;
#pragma unroll
            for (int e = 0; e < PF; ++e) {
                const int idx = tid + e * CS_WAVE;
                if (idx < nn) As[r + c * S] = pf[e];
                r += dr;
                c += dc;
                if (r >= n) {
                    r -= n;
                    ++c;
                }
            }
        };
        fetch(Ab + (tv_AB ? (int64_t)(N - 2) * nn : 0));
        stage();
        int cur = 0;
        if (tid < n) ls[tid] = L[(int64_t)(N - 1) * n + tid];
        __syncthreads();
        for (int k = N - 1; k >= 1; --k) {   // λ_k, at index k−1, from A_k, B_k, K_k (index k−1) and λ_{k+1}
            const bool more = tv_AB && k > 1;
            if (more) fetch(Ab + (int64_t)(k - 2) * nn);
            const T *lc = ls + cur * n;
            if (tid < m) {
                const T *col = Bb + (tv_AB ? (int64_t)(k - 1) * n * m : 0) + (int64_t)tid * n;
                T acc = T(0);
                for (int i = 0; i < n; ++i) acc += col[i] * lc[i];
                ws[tid] = acc;
            }
            __syncthreads();
            if (tid < n) {
                T acc = L[(int64_t)(k - 1) * n + tid];
                const T *col = As + tid * S;
                for (int i = 0; i < n; ++i) acc += col[i] * lc[i];
                const T *kc = Kb + (int64_t)(k - 1) * m * n + (int64_t)tid * m;
                T kt = T(0);
                for (int i = 0; i < m; ++i) kt += kc[i] * ws[i];
                acc -= kt;
                ls[(cur ^ 1) * n + tid] = acc;
                L[(int64_t)(k - 1) * n + tid] = acc;
            }
            __syncthreads();
            if (more) {
                stage();
                __syncthreads();
            }
            cur ^= 1;
        }
        __syncthreads();
    }
}

// ---- the chain, past one wave (n > 64 or m > 64): a workgroup per trajectory, matrices from global ----
// Wave w takes the columns j = w, w + 4, …; its lanes stride the rows of the column (coalesced) and
// reduce with a butterfly, so every lane holds the same sum: first the m columns of B_k (w = B_kᵀλ),
// then the n columns of A_k and K_k together.  λ (two buffers) and w sit in LDS.
template <typename T>
__global__ __launch_bounds__(CS_WG) void dp_costate_wg_kernel(const T *__restrict__ A, const T *__restrict__ B,
                                                              const T *__restrict__ K, T *__restrict__ lam, int n,
                                                              int m, int N, int tv_AB, int64_t batch)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T *ls = reinterpret_cast<T *>(smem_raw);
    T *ws = ls + 2 * n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = CS_WG / 64;
    const int64_t nn = (int64_t)n * n, nm = (int64_t)n * m;
    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        T *L = lam + b * (int64_t)N * n;
        const T *Ab = A + b * nn * (tv_AB ? N - 1 : 1);
        const T *Bb = B + b * nm * (tv_AB ? N - 1 : 1);
        const T *Kb = K + b * nm * (N - 1);
        int cur = 0;
        for (int i = tid; i < n; i += CS_WG) ls[i] = L[(int64_t)(N - 1) * n + i];
        __syncthreads();
        for (int k = N - 1; k >= 1; --k) {
            const T *Ak = Ab + (tv_AB ? (int64_t)(k - 1) * nn : 0);
            const T *Bk = Bb + (tv_AB ? (int64_t)(k - 1) * nm : 0);
            const T *Kk = Kb + (int64_t)(k - 1) * nm;
            const T *lc = ls + cur * n;
            T *ln = ls + (cur ^ 1) * n;
            for (int j = wave; j < m; j += nw) {
                const T *col = Bk + (int64_t)j * n;
                T acc = T(0);
                for (int i = lane; i < n; i += 64) acc += col[i] * lc[i];
                for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
                if (lane == 0) ws[j] = acc;
            }
            __syncthreads();
            for (int j = wave; j < n; j += nw) {
                const T *col = Ak + (int64_t)j * n;
                const T *kc = Kk + (int64_t)j * m;
                T acc = T(0);
                for (int i = lane; i < n; i += 64) acc += col[i] * lc[i];
                for (int i = lane; i < m; i += 64) acc -= kc[i] * ws[i];
                for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
                if (lane == 0) {
                    const T v = L[(int64_t)(k - 1) * n + j] + acc;
                    ln[j] = v;
                    L[(int64_t)(k - 1) * n + j] = v;
                }
            }
            __syncthreads();
            cur ^= 1;
        }
        __syncthreads();
    }
}

// gX (n·N per trajectory) → q' (n·(N−1) per trajectory) and qf' (n per trajectory)
template <typename T>
__global__ void dp_adjoint_pack_kernel(const T *__restrict__ gX, T *__restrict__ q, T *__restrict__ qf, int n, int N,
                                       int64_t batch)
{
    const int64_t per = (int64_t)n * N, head = (int64_t)n * (N - 1), total = per * batch;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = e / per, r = e - b * per;
        if (r < head)
            q[b * head + r] = gX[e];
        else
            qf[b * n + (r - head)] = gX[e];
    }
}

// out (rows × cols, column-major) = scale · (a bᵀ + c dᵀ); W lanes stride a column, ny columns at a time
template <typename T>
__device__ inline void outer2(T *__restrict__ out, int rows, int cols, const T *a, const T *b, const T *c, const T *d,
                              T scale, int tid, int nt)
{
    const int W = pow2_width(rows), tx = tid & (W - 1), ty = tid / W, ny = nt / W;
    for (int j = ty; j < cols; j += ny) {
        const T bj = b[j], dj = d[j];
        for (int i = tx; i < rows; i += W) out[i + (int64_t)j * rows] = scale * (a[i] * bj + c[i] * dj);
    }
}

template <typename T>
__device__ inline void copyv(T *__restrict__ out, const T *in, int len, int tid, int nt)
{
    for (int i = tid; i < len; i += nt) out[i] = in[i];
}

struct GradPtrs {
    void *gA, *gB, *gc, *gQ, *gR, *gM, *gQf, *gx0, *gq, *gr, *gqf;
};

// ---- per-knot outputs: one workgroup per (trajectory, knot); knot index N−1 carries the terminal
// outputs gQf, gqf and gx0.  Every store is along a column of its column-major output. ----
template <typename T>
__global__ __launch_bounds__(CS_WG) void dp_grad_kernel(const T *__restrict__ X, const T *__restrict__ U,
                                                        const T *__restrict__ lam, const T *__restrict__ Xa,
                                                        const T *__restrict__ Ua, const T *__restrict__ lama,
                                                        GradPtrs g, int n, int m, int N, int tv_AB, int64_t batch)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t total = batch * (int64_t)N;
    T *gA = (T *)g.gA, *gB = (T *)g.gB, *gc = (T *)g.gc, *gQ = (T *)g.gQ, *gR = (T *)g.gR, *gM = (T *)g.gM;
    T *gQf = (T *)g.gQf, *gx0 = (T *)g.gx0, *gq = (T *)g.gq, *gr = (T *)g.gr, *gqf = (T *)g.gqf;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const int64_t b = w / N;
        const int kk = (int)(w - b * N);
        const T *x = X + (b * N + kk) * n, *xa = Xa + (b * N + kk) * n;
        if (kk == N - 1) {
            if (gQf) outer2(gQf + b * n * n, n, n, xa, x, x, xa, T(0.5), tid, nt);
            if (gqf) copyv(gqf + b * n, xa, n, tid, nt);
            if (gx0) copyv(gx0 + b * n, lama + b * N * n, n, tid, nt);
            continue;
        }
        const int64_t kn = b * (N - 1) + kk;   // per-knot block index
        const T *u = U + kn * m, *ua = Ua + kn * m;
        const T *l = lam + (b * N + kk + 1) * n, *la = lama + (b * N + kk + 1) * n;   // λ_{k+1}, λ'_{k+1}
        if (tv_AB) {
            if (gA) outer2(gA + kn * n * n, n, n, la, x, l, xa, T(1), tid, nt);
            if (gB) outer2(gB + kn * n * m, n, m, la, u, l, ua, T(1), tid, nt);
            if (gc) copyv(gc + kn * n, la, n, tid, nt);
        }
        if (gQ) outer2(gQ + kn * n * n, n, n, xa, x, x, xa, T(0.5), tid, nt);
        if (gR) outer2(gR + kn * m * m, m, m, ua, u, u, ua, T(0.5), tid, nt);
        if (gM) outer2(gM + kn * m * n, m, n, ua, x, u, xa, T(1), tid, nt);
        if (gq) copyv(gq + kn * n, xa, n, tid, nt);
        if (gr) copyv(gr + kn * m, ua, m, tid, nt);
    }
}

// ---- time-invariant A, B, c: gA, gB, gc summed over the knots, one workgroup per trajectory.
// A thread owns elements of the output and adds the knots k = 1 … N−1 in ascending order in a
// register.  Virtual column j: j < n a column of gA, n ≤ j < n + m a column of gB, j = n + m is gc. ----
template <typename T>
__global__ __launch_bounds__(CS_WG) void dp_grad_sum_kernel(const T *__restrict__ X, const T *__restrict__ U,
                                                            const T *__restrict__ lam, const T *__restrict__ Xa,
                                                            const T *__restrict__ Ua, const T *__restrict__ lama,
                                                            T *__restrict__ gA, T *__restrict__ gB, T *__restrict__ gc,
                                                            int n, int m, int N, int64_t batch)
{
    const int tid = threadIdx.x;
    const int W = pow2_width(n), tx = tid & (W - 1), ty = tid / W, ny = CS_WG / W;
    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const T *Xb = X + b * N * n, *Xab = Xa + b * N * n;
        const T *Ub = U + b * (N - 1) * m, *Uab = Ua + b * (N - 1) * m;
        const T *Lb = lam + b * N * n, *Lab = lama + b * N * n;
        for (int j = ty; j < n + m + 1; j += ny) {
            const bool isA = j < n, isB = !isA && j < n + m;
            if ((isA && !gA) || (isB && !gB) || (!isA && !isB && !gc)) continue;
            const T *v = isA ? Xb + j : Ub + (j - n), *va = isA ? Xab + j : Uab + (j - n);
            const int vs = isA ? n : m;   // knot stride of v, va
            for (int i = tx; i < n; i += W) {
                T acc = T(0);
                if (isA || isB) {
                    for (int k = 0; k < N - 1; ++k)
                        acc += Lab[(int64_t)(k + 1) * n + i] * v[(int64_t)k * vs] +
                               Lb[(int64_t)(k + 1) * n + i] * va[(int64_t)k * vs];
                } else {
                    for (int k = 0; k < N - 1; ++k) acc += Lab[(int64_t)(k + 1) * n + i];
                }
                if (isA)
                    gA[b * n * n + (int64_t)j * n + i] = acc;
                else if (isB)
                    gB[b * n * m + (int64_t)(j - n) * n + i] = acc;
                else
                    gc[b * n + i] = acc;
            }
        }
    }
}

inline unsigned grid_for(int64_t items)
{
    const int64_t cap = 1 << 20;   // the kernels loop over their work items with a grid stride
    return (unsigned)(items < cap ? (items < 1 ? 1 : items) : cap);
}

template <typename T>
hipError_t costate_launch_t(const DpCostateArgs &a, hipStream_t s)
{
    const int n = a.n, m = a.m, N = a.N;
    const bool wave = n <= 64 && m <= 64;
    const int nt = wave ? CS_WAVE : CS_WG;
    dp_costate_g_kernel<T><<<grid_for(a.batch * N), nt, (size_t)(n + 2 * m) * sizeof(T), s>>>(
        (const T *)a.Q, (const T *)a.R, (const T *)a.M, (const T *)a.Qf, (const T *)a.q, (const T *)a.r,
        (const T *)a.qf, (const T *)a.K, (const T *)a.X, (const T *)a.U, (T *)a.lam, n, m, N, a.tv_QR, a.batch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const T *A = (const T *)a.A, *B = (const T *)a.B, *K = (const T *)a.K;
    if (wave) {
        // ≤ 34 816 B (n = m = 64, fp64)
        const size_t lds = ((size_t)n * (n | 1) + 2 * (size_t)n + (size_t)m) * sizeof(T);
        if (n <= 32)
            dp_costate_kernel<T, 16><<<grid_for(a.batch), CS_WAVE, lds, s>>>(A, B, K, (T *)a.lam, n, m, N, a.tv_AB,
                                                                             a.batch);
        else
            dp_costate_kernel<T, 64><<<grid_for(a.batch), CS_WAVE, lds, s>>>(A, B, K, (T *)a.lam, n, m, N, a.tv_AB,
                                                                             a.batch);
    } else {
        dp_costate_wg_kernel<T><<<grid_for(a.batch), CS_WG, (2 * (size_t)n + m) * sizeof(T), s>>>(
            A, B, K, (T *)a.lam, n, m, N, a.tv_AB, a.batch);
    }
    return hipGetLastError();
}

template <typename T>
hipError_t grad_launch_t(const DpGradArgs &a, hipStream_t s)
{
    const GradPtrs g{a.gA, a.gB, a.gc, a.gQ, a.gR, a.gM, a.gQf, a.gx0, a.gq, a.gr, a.gqf};
    const bool perknot = a.gQ || a.gR || a.gM || a.gQf || a.gx0 || a.gq || a.gr || a.gqf ||
                         (a.tv_AB && (a.gA || a.gB || a.gc));
    if (perknot) {
        dp_grad_kernel<T><<<grid_for(a.batch * a.N), CS_WG, 0, s>>>((const T *)a.X, (const T *)a.U, (const T *)a.lam,
                                                                    (const T *)a.Xa, (const T *)a.Ua,
                                                                    (const T *)a.lama, g, a.n, a.m, a.N, a.tv_AB,
                                                                    a.batch);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (!a.tv_AB && (a.gA || a.gB || a.gc)) {
        dp_grad_sum_kernel<T><<<grid_for(a.batch), CS_WG, 0, s>>>((const T *)a.X, (const T *)a.U, (const T *)a.lam,
                                                                  (const T *)a.Xa, (const T *)a.Ua, (const T *)a.lama,
                                                                  (T *)a.gA, (T *)a.gB, (T *)a.gc, a.n, a.m, a.N,
                                                                  a.batch);
        return hipGetLastError();
    }
    return hipSuccess;
}

} // namespace

hipError_t dp_costate_launch(const DpCostateArgs &a, hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (a.n < 1 || a.m < 1 || a.n > 512 || a.m > 512 || a.N < 2) return hipErrorNotSupported;
    return a.dtype == 0 ? costate_launch_t<double>(a, s) : costate_launch_t<float>(a, s);
}

hipError_t dp_adjoint_pack_launch(const void *gX, void *q, void *qf, int n, int N, int64_t batch, int dtype,
                                  hipStream_t s)
{
    if (batch <= 0) return hipSuccess;
    const int64_t total = (int64_t)n * N * batch;
    const unsigned grid = grid_for((total + 255) / 256);
    if (dtype == 0)
        dp_adjoint_pack_kernel<double><<<grid, 256, 0, s>>>((const double *)gX, (double *)q, (double *)qf, n, N, batch);
    else
        dp_adjoint_pack_kernel<float><<<grid, 256, 0, s>>>((const float *)gX, (float *)q, (float *)qf, n, N, batch);
    return hipGetLastError();
}

hipError_t dp_grad_launch(const DpGradArgs &a, hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    return a.dtype == 0 ? grad_launch_t<double>(a, s) : grad_launch_t<float>(a, s);
}

} // namespace lqrx
