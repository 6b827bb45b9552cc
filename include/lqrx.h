/*
 * lqrx.h — C ABI of the MI355X-native batched LQR / block-tridiagonal-KKT solver.
 *
 * Drop-in boundary for the hot path of bjack205/LQR.jl.  The reference has no FFI: its
 * only native boundary is Julia stdlib `ccall`s into LAPACK/BLAS, one call per knot-op
 * (SURVEY.md §1, §2 "native arithmetic" table).  This ABI replaces those calls at batch
 * grain — one call per batch of independent problems — and is what a Julia `ccall` shim
 * binds (INTEGRATION.md shows the shim).
 *
 * Conventions (all entry points):
 *   - plain C types only; `extern "C"`; no exceptions cross the boundary;
 *   - the caller owns every buffer; the library never frees or retains caller pointers;
 *   - layout 0 = Julia column-major with the batch index slowest, i.e. exactly the memory
 *     of Array{T,3}(r,c,batch) / Array{T,4}(r,c,knots,batch) — no copy from Julia;
 *   - return 0 on success; -i if argument i (1-based) is invalid (LAPACK convention);
 *     1 if the call completed synchronously and at least one trajectory has info != 0;
 *     LQRX_ERR_* (< -99) for runtime failures; lqrx_last_error() describes the last error
 *     of the calling thread;
 *   - `stream` is a hipStream_t: NULL = synchronous (like the reference's solve!), else the
 *     work is enqueued and the call returns immediately (check info[] after syncing);
 *   - reentrant and thread-safe.  Mutable library state, all of it process-wide and
 *     mutex-guarded: the calling thread's last-error string (thread-local); one HIP
 *     memory pool per device for stream-ordered scratch (created on first use, blocks kept
 *     mapped); a cache of uploaded KKT block-structure tables (≤ 4096 distinct structures,
 *     never evicted — each is uploaded once, with a blocking copy, on its first use; calls
 *     with further structures upload a per-call table on their own stream and wait for that
 *     stream only); environment switches read once.  All of it is keyed on the device of
 *     the call's `stream`, not on the thread's current device.  No call synchronises the
 *     whole device.
 */
#ifndef LQRX_H
#define LQRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LQRX_ABI_VERSION 5   /* 2: layout 1 (DP, KKT), lqrx_sqp_* (models, stage constraints);
                                3: lqrx_dp_solve_linear[_host] (linear cost terms), and
                                   dtype LQRX_F32 on the KKT path (large-block kernels);
                                4: lqrx_scratch_trim (release the library's pooled scratch);
                                   KKT blocks past 64 rows (up to 512, w up to 1024);
                                   KKT layout 1 for every structure (staged);
                                   lqrx_dp_compute_ctg[_host] (per-knot surface);
                                5: lqrx_*_host_devices (one call sharded over GPUs);
                                   lqrx_dp_solve_affine[_host], lqrx_dp_solve_cross[_host] and
                                   lqrx_dp_solve_value[_host] are additive to ABI 5 (no existing
                                   signature or struct changed, the number stays 5): detect
                                   them by symbol (dlsym); so are lqrx_dp_costates[_host],
                                   lqrx_dp_solve_adjoint and lqrx_dp_rollout[_host] */

#define LQRX_F64 0
#define LQRX_F32 1

#define LQRX_ERR_HIP (-100)         /* HIP runtime error (see lqrx_last_error)          */
#define LQRX_ERR_UNSUPPORTED (-101) /* valid but not (yet) supported shape / option    */
#define LQRX_ERR_NODEVICE (-102)    /* no gfx950 device / HIP runtime unavailable        */

/* ------------------------------------------------------------------------------------
 * DP path: Riccati backward pass + forward rollout.
 * Replaces solve!(sol::LQRSolution, solver::DPSolver, prob::LQRProblem)
 *   /root/reference/src/dynamic_programming.jl:54-72
 * including compute_gain!/compute_ctg!/chol_solve! (:28-52) and the DPSolver scratch
 * (:2-23: owned by the library, stream-ordered).  Problem data = LQRProblem fields
 * (/root/reference/src/lqr_problem.jl:1-11): time-invariant A (n×n), B (n×m), Q (n×n),
 * R (m×m), Qf (n×n), x0 (n), horizon N knots.
 *
 * Buffers (layout 0, element type per dtype):
 *   A  n·n·batch     B  n·m·batch    Q  n·n·batch    R  m·m·batch    Qf n·n·batch
 *      (×(N-1) per trajectory for time-varying fields, see knot_stride_*; the
 *       time-varying path is SURVEY §8(f) rank 1; every supported n, m)
 *   x0 n·batch
 *   K  m·n·(N-1)·batch     sol.K[k], k = 1..N-1  (LQRSolution.K)
 *   P  n·n·batch  (p_mode 0: P_1 = solver.P on return, :63)
 *      n·n·N·batch (p_mode 1: P_k for k = 1..N, P_N = Qf)
 *   X  n·N·batch           sol.X
 *   U  m·(N-1)·batch       sol.U
 *   info int32·batch : 0, or the knot k (1-based) of the first E = R + BᵀPB found not
 *        positive definite in the backward sweep (the reference discards potrf's info,
 *        dynamic_programming.jl:29; the solve still runs to completion, as there).
 * ------------------------------------------------------------------------------------ */
typedef struct lqrx_dp_desc {
    int32_t n, m, N;        /* state dim, control dim, knots (N >= 2); 1 <= n, m <= 512
                               (n <= 4: lane kernels; n <= 64, m <= 32: register-tiled
                               MFMA kernel; beyond: workgroup-per-trajectory kernel)      */
    int32_t dtype;          /* LQRX_F64 (reference precision) or LQRX_F32            */
    int64_t batch;          /* number of independent problems                          */
    int32_t layout;         /* 0 = column-major blocks, batch slowest (Julia Array{T,3});
                               1 = batch fastest (SoA): element e of trajectory b at
                               [e·batch + b], e = its layout-0 offset within the
                               trajectory (Julia permutedims(X, (3,1,2)), Python [S][batch]);
                               every array of the call (inputs and outputs) uses it.  Native
                               in the n ≤ 4 kernels (coalesced per element); n ≥ 5 converts
                               to layout 0 in stream-ordered scratch and back (2× traffic) */
    int32_t p_mode;         /* 0 = P_1 only (reference-observable), 1 = all P_k        */
    int64_t knot_stride_AB; /* 0 = time-invariant A, B (reference LQRProblem);
                               1 = per knot: A n·n·(N-1)·batch, B n·m·(N-1)·batch, knot k
                               at index k-1 (LCRProblem.A/.B, constrained_problem.jl:3-4) */
    int64_t knot_stride_QR; /* 0 = time-invariant Q, R; 1 = per knot: Q n·n·(N-1)·batch,
                               R m·m·(N-1)·batch (Qf stays the terminal cost)            */
} lqrx_dp_desc;

/* device pointers (hipMalloc'd or torch CUDA/HIP tensors) */
int lqrx_dp_solve(const lqrx_dp_desc *desc, const void *A, const void *B, const void *Q,
                  const void *R, const void *Qf, const void *x0, void *K, void *P, void *X,
                  void *U, int32_t *info, void *stream);

/* host pointers: H2D, solve, D2H, synchronous (what the Julia shim calls by default) */
int lqrx_dp_solve_host(const lqrx_dp_desc *desc, const void *A, const void *B, const void *Q,
                       const void *R, const void *Qf, const void *x0, void *K, void *P,
                       void *X, void *U, int32_t *info);

/* Per-knot DP surface — compute_ctg!(K, solver, prob) (dynamic_programming.jl:45-52, which
 * runs compute_gain! :34-43 first) for a batch of problems, from P = solver.P (P_{k+1}):
 *   K  = E⁻¹BᵀPA  with E = R + BᵀPB   (m·n·batch, sol.K[k])
 *   P_ = Q + AᵀPA − APB·K               (n·n·batch, solver.P_; NULL = compute_gain! only)
 * A, B, Q, R, P as lqrx_dp_solve's A, B, Q, R, Qf (time-invariant; desc.N, p_mode and the
 * knot strides are ignored); info as lqrx_dp_solve (1 = E not positive definite).  The same
 * kernels as lqrx_dp_solve (a 2-knot solve with Qf = P).
 * Precondition: P and Q symmetric, as every cost-to-go and cost Hessian of the recursion is.
 * The n ≥ 5 and n ≤ 4 kernel families use the symmetric fast form (P_ = Q + AᵀPA − GᵀK on the
 * lower triangle, mirrored), the n > 64 workgroup kernel the reference's operation order, so
 * for a non-symmetric P or Q the result depends on the family.  The host wrappers (Python
 * lqrx.compute_ctg*, Julia compute_ctg!) reject P or Q whose asymmetry exceeds
 * max(1e-10, 100 ulp of the dtype) of the matrix's largest entry (Q only when P_ is asked). */
int lqrx_dp_compute_ctg(const lqrx_dp_desc *desc, const void *A, const void *B, const void *Q,
                        const void *R, const void *P, void *K, void *P_, int32_t *info, void *stream);
int lqrx_dp_compute_ctg_host(const lqrx_dp_desc *desc, const void *A, const void *B, const void *Q,
                             const void *R, const void *P, void *K, void *P_, int32_t *info);

/* ------------------------------------------------------------------------------------
 * DP path with linear cost terms — SURVEY §8(f) rank 1 ("time-varying LQR … and cost
 * linear terms"), an extension of the reference LQRProblem (lqr_problem.jl:1-11 has no
 * linear terms).  Stage cost ½xᵀQx + qᵀx + ½uᵀRu + rᵀu, terminal ½xᵀQf x + qfᵀx; the
 * value function gains a linear part V_k(x) = ½xᵀP_k x + p_kᵀx and the policy a
 * feedforward: u_k = −K_k x_k − d_k.  In the reference's op order (oracle/lqr_oracle.c
 * oracle_dp_solve_one_lin): d_k = E⁻¹(r_k + Bᵀp_{k+1}) is one more right-hand side of
 * chol_solve! (dynamic_programming.jl:42), p_k = q_k + Aᵀp_{k+1} − APB·d_k follows :51.
 * Same descriptor, inputs and outputs as lqrx_dp_solve plus:
 *   q   n·batch, or n·(N−1)·batch when knot_stride_QR = 1 (knot k at k−1, like Q)
 *   r   m·batch, or m·(N−1)·batch when knot_stride_QR = 1
 *   qf  n·batch
 *   d   out: m·(N−1)·batch   feedforward d_k, k = 1..N−1
 *   p   out: n·batch (p_mode 0: p_1) or n·N·batch (p_mode 1: p_k, p_N = qf)
 * layout 1 applies to these arrays as well.  All zero q, r, qf give the lqrx_dp_solve
 * results (with d = 0, p = 0).
 * ------------------------------------------------------------------------------------ */
typedef struct lqrx_dp_linear {
    const void *q, *r, *qf; /* linear cost terms (inputs)        */
    void *d, *p;            /* feedforward, linear cost-to-go (outputs) */
} lqrx_dp_linear;

int lqrx_dp_solve_linear(const lqrx_dp_desc *desc, const void *A, const void *B,
                         const void *Q, const void *R, const void *Qf, const void *x0,
                         const lqrx_dp_linear *lin, void *K, void *P, void *X, void *U,
                         int32_t *info, void *stream);

/* host pointers in lin and everywhere else: H2D, solve, D2H, synchronous */
int lqrx_dp_solve_linear_host(const lqrx_dp_desc *desc, const void *A, const void *B,
                              const void *Q, const void *R, const void *Qf, const void *x0,
                              const lqrx_dp_linear *lin, void *K, void *P, void *X, void *U,
                              int32_t *info);

/* ------------------------------------------------------------------------------------
 * DP path with affine dynamics  x_{k+1} = A_k x_k + B_k u_k + c_k  — what a linearisation
 * about a non-equilibrium trajectory yields (reference tracking, the defect of a
 * multiple-shooting / SQP iterate, a gravity or disturbance feed-through); together with
 * the linear cost terms above and the cost cross term of lqrx_dp_solve_cross below this is
 * the LQ subproblem of an iLQR / SQP / MPC caller.  With V_{k+1}(x) = ½xᵀP x + pᵀx, E = R_k + BᵀPB, G = BᵀPA:
 *   p̃   = p_{k+1} + P_{k+1} c_k
 *   K_k = E⁻¹G                     (K, P and info do not depend on c, q, r)
 *   d_k = E⁻¹(r_k + Bᵀp̃)          p_k = q_k + Aᵀp̃ − Gᵀd_k          P_k = Q_k + AᵀPA − GᵀK_k
 *   rollout: u_k = −K_k x_k − d_k,  x_{k+1} = A_k x_k + B_k u_k + c_k
 * i.e. lqrx_dp_solve_linear's recursion with p̃ in place of p.  (The constant of the value
 * function is not formed.)  Same descriptor, inputs and outputs as lqrx_dp_solve_linear plus
 *   c   n·batch, or n·(N−1)·batch when knot_stride_AB = 1 (knot k at k−1: c follows A and B
 *       as q and r follow Q and R); desc.layout applies to it as to every array.
 * lin is required with all five pointers non-NULL (a caller without cost terms passes zero
 * q, r, qf); d and p are outputs as above.  All-zero c gives the lqrx_dp_solve_linear results.
 * Error codes follow the argument position: desc −1, A −2, B −3, c −4, Q −5, R −6, Qf −7,
 * x0 −8, lin or one of its members −9, K −10, P −11, X −12, U −13; batch = 0 returns 0.
 * Every (n, m, dtype, layout, knot stride, p_mode) lqrx_dp_solve_linear accepts is accepted.
 * Kernel routing differs from lqrx_dp_solve_linear in two places: n ≤ 4 always takes the
 * lane-per-trajectory kernel (never the four-lane kernel of small time-invariant batches),
 * and fp64 n = 64, m ∈ {16, 32} takes the one-wave register-tiled kernel (the LQRX_DP_WG4=0
 * path), not the four-wave kernel.  There is no _host_devices twin and no affine
 * lqrx_dp_compute_ctg.  Additive to ABI 5: detect by symbol.
 * ------------------------------------------------------------------------------------ */
int lqrx_dp_solve_affine(const lqrx_dp_desc *desc, const void *A, const void *B, const void *c,
                         const void *Q, const void *R, const void *Qf, const void *x0,
                         const lqrx_dp_linear *lin, void *K, void *P, void *X, void *U,
                         int32_t *info, void *stream);

/* host pointers in lin and everywhere else: H2D, solve, D2H, synchronous */
int lqrx_dp_solve_affine_host(const lqrx_dp_desc *desc, const void *A, const void *B,
                              const void *c, const void *Q, const void *R, const void *Qf,
                              const void *x0, const lqrx_dp_linear *lin, void *K, void *P,
                              void *X, void *U, int32_t *info);

/* ------------------------------------------------------------------------------------
 * DP path with a cost cross term: stage cost ½xᵀQ_k x + uᵀM_k x + ½uᵀR_k u + q_kᵀx + r_kᵀu —
 * the Q_ux of an iLQR / DDP backward pass, a cost on an output y = Cx + Du, a cost
 * discretised with the dynamics, a problem after the feedback pre-transformation u = ũ − Fx.
 * The affine recursion above changes in one place, G:
 *   E   = R_k + BᵀPB                    (unchanged: info does not depend on M)
 *   G   = BᵀPA + M_k
 *   K_k = E⁻¹G        d_k = E⁻¹(r_k + Bᵀp̃)        p̃ = p_{k+1} + P_{k+1} c_k
 *   P_k = Q_k + AᵀPA − GᵀK_k            p_k = q_k + Aᵀp̃ − Gᵀd_k
 *   rollout unchanged: u_k = −K_k x_k − d_k,  x_{k+1} = A_k x_k + B_k u_k + c_k
 * The problem is convex when the joint block [Q_k M_kᵀ; M_k R_k] is positive semidefinite;
 * info is, as everywhere, the first knot whose E is not positive definite.  Same descriptor,
 * inputs and outputs as lqrx_dp_solve_affine plus
 *   M   m·n·batch, column-major m×n per trajectory (the shape of K_k), or m·n·(N−1)·batch when
 *       knot_stride_QR = 1 (knot k at k−1: M is a cost term and follows Q and R, as q and r
 *       do); desc.layout applies to it as to every array.
 * c and lin are required with all pointers non-NULL, as in lqrx_dp_solve_affine: a caller
 * without an offset or without linear cost terms passes zeros.  One kernel family serves the
 * entry, so a caller with only a cross term pays for the linear and affine work as well; a
 * leaner variant without them is a possible follow-up.  All-zero M gives the
 * lqrx_dp_solve_affine results.
 * Error codes follow the argument position: desc −1, A −2, B −3, c −4, Q −5, R −6, M −7,
 * Qf −8, x0 −9, lin or one of its members −10, K −11, P −12, X −13, U −14, decided before the
 * device is touched; batch = 0 returns 0.
 * Every (n, m, dtype, layout, knot stride, p_mode) lqrx_dp_solve_affine accepts is accepted,
 * with its kernel routing: n ≤ 4 the lane-per-trajectory kernel, fp64 n = 64 the one-wave
 * register-tiled kernel, past the register tiles the workgroup-per-trajectory kernel.
 * Out of scope: there is no _host_devices twin, no lqrx_dp_compute_ctg with a cross term, and
 * the constant of the value function is not formed (lqrx_dp_solve_value below forms it).
 * Additive to ABI 5: detect by symbol.
 * ------------------------------------------------------------------------------------ */
int lqrx_dp_solve_cross(const lqrx_dp_desc *desc, const void *A, const void *B, const void *c,
                        const void *Q, const void *R, const void *M, const void *Qf,
                        const void *x0, const lqrx_dp_linear *lin, void *K, void *P, void *X,
                        void *U, int32_t *info, void *stream);

/* host pointers in lin and everywhere else: H2D, solve, D2H, synchronous */
int lqrx_dp_solve_cross_host(const lqrx_dp_desc *desc, const void *A, const void *B,
                             const void *c, const void *Q, const void *R, const void *M,
                             const void *Qf, const void *x0, const lqrx_dp_linear *lin, void *K,
                             void *P, void *X, void *U, int32_t *info);

/* ------------------------------------------------------------------------------------
 * DP path with the value function's constant: the solve of lqrx_dp_solve_cross, which also
 * returns the third part of V_k(x) = ½xᵀP_k x + p_kᵀx + s_k and the two numbers a caller wants
 * right after a backward pass — the optimal cost (ranking a sampling / multi-start MPC batch,
 * logging) and the expected reduction of an iLQR / DDP line search.  With the names of the
 * cross recursion above (E = R_k + BᵀPB, p̃ = p_{k+1} + P_{k+1}c_k, h = r_k + Bᵀp̃, d_k = E⁻¹h):
 *   s_N = 0
 *   s_k = s_{k+1} + c_kᵀ(p_{k+1} + ½P_{k+1}c_k) − ½h_kᵀd_k
 *   dV  = Σ_{k=1}^{N−1} h_kᵀd_k               (≥ 0 when every E is positive definite;
 *                                              ΔV(α) = −α(1 − α/2)·dV is the Armijo reference)
 *   J   = ½x0ᵀP_1x0 + p_1ᵀx0 + s_1            (= the cost of the X, U the solve returns)
 * With c = 0, s_1 = −½dV.  K, P, d, p, X, U and info are exactly those of lqrx_dp_solve_cross
 * on the same data.  Arguments, layouts, knot strides and kernel routing are those of
 * lqrx_dp_solve_cross, plus val behind lin:
 *   val->s   required.  p_mode 0: batch elements, s_1 per trajectory.  p_mode 1: N·batch, s_k of
 *            trajectory b at [b·N + (k−1)] (layout 0) or [(k−1)·batch + b] (layout 1), s_N = 0.
 *   val->dV  optional (NULL: not written): batch elements.
 *   val->J   optional (NULL: not formed): batch elements, accumulated in double from P_1, p_1,
 *            s_1 and x0 by one small kernel behind the solve, on the same stream.
 * dV, J and the p_mode-0 s are batch vectors in both layouts.  The element type is desc.dtype.
 * For a trajectory with info ≠ 0 the three values are unspecified; every other trajectory is
 * unaffected.  s_1 is the same bits in both p_modes.
 * Error codes follow the argument position: desc −1, A −2, B −3, c −4, Q −5, R −6, M −7,
 * Qf −8, x0 −9, lin or one of its members −10, val or its member s −11, K −12, P −13, X −14,
 * U −15, decided before the device is touched; batch = 0 returns 0.
 * Out of scope: there is no _host_devices twin, no per-knot lqrx_dp_compute_ctg form, and no
 * variant without the linear, affine and cross work (a caller without c, M, q, r passes zeros
 * and pays for them).  Additive to ABI 5: detect by symbol.
 * ------------------------------------------------------------------------------------ */
typedef struct lqrx_dp_value {
    void *s;    /* out, required: batch (p_mode 0: s_1) or N·batch (p_mode 1: s_k, s_N = 0) */
    void *dV;   /* out, optional (NULL): batch, Σ_k h_kᵀd_k                               */
    void *J;    /* out, optional (NULL): batch, V_1(x0)                                   */
} lqrx_dp_value;

int lqrx_dp_solve_value(const lqrx_dp_desc *desc, const void *A, const void *B, const void *c,
                        const void *Q, const void *R, const void *M, const void *Qf,
                        const void *x0, const lqrx_dp_linear *lin, const lqrx_dp_value *val,
                        void *K, void *P, void *X, void *U, int32_t *info, void *stream);

/* host pointers in lin, val and everywhere else: H2D, solve, D2H, synchronous */
int lqrx_dp_solve_value_host(const lqrx_dp_desc *desc, const void *A, const void *B,
                             const void *c, const void *Q, const void *R, const void *M,
                             const void *Qf, const void *x0, const lqrx_dp_linear *lin,
                             const lqrx_dp_value *val, void *K, void *P, void *X, void *U,
                             int32_t *info);

/* ------------------------------------------------------------------------------------
 * Costates of a DP solve — the multipliers of the dynamics constraints, with the sign
 * λ_k = ∂V_k/∂x = P_k x_k + p_k (the negative of the KKT path's lam for the same problem): what an
 * SQP caller needs for its dual residual and merit function and an iLQR caller for the
 * Hamiltonian.  They come from one backward sweep over the solve's own K, X, U, without P_k:
 *   λ_N = Qf x_N + qf
 *   λ_k = Q_k x_k + M_kᵀu_k + q_k + A_kᵀλ_{k+1} − K_kᵀ s_k          k = N−1 … 1
 *   s_k = R_k u_k + M_k x_k + r_k + B_kᵀλ_{k+1}                      (= 0 at the solution)
 * s_k is the stationarity condition, so the last term is zero in exact arithmetic and the sweep is
 * the textbook λ_k = Q_k x_k + M_kᵀu_k + q_k + A_kᵀλ_{k+1}; with it the recursion runs through the
 * closed loop (A_k − B_kK_k)ᵀ, which the solve made stable.  The textbook form propagates rounding
 * errors with the open-loop A_kᵀ: at n = 32, m = 16, N = 256 with ρ(A) = 1.14 it is wrong in the
 * fifth digit in fp64, the form above exact to 3e-15.  The price: a caller needs the solve's K and
 * the problem's B, R, r to get multipliers, and the sweep reads 2n² + m² + 3nm elements per knot
 * where the textbook form reads 2n² + nm (1.5 times the bytes at m = n/2).  λ_1 = ∂J/∂x0.
 *   A, B, Q, R, Qf, K, X, U   the problem and the outputs of the solve (knot strides of desc)
 *   M, q, r, qf               may be NULL, meaning zero (so the outputs of a plain lqrx_dp_solve
 *                             have multipliers too); M, q, r follow knot_stride_QR
 *   lam                       out: n·N·batch, laid out like X (λ_k of trajectory b at [(b·N + k−1)·n])
 * desc.p_mode is ignored.  Every (n, m ≤ 512, dtype, knot stride) the solve accepts is accepted;
 * desc.layout = 1 returns LQRX_ERR_UNSUPPORTED (a follow-up).  Error codes follow the argument
 * position: desc −1, A −2, B −3, Q −4, R −5, Qf −7, K −11, X −12, U −13, lam −14, decided before
 * the device is touched; batch = 0 returns 0.  Results are the same bits from run to run (no atomics).
 * Additive to ABI 5: detect by symbol.
 * ------------------------------------------------------------------------------------ */
int lqrx_dp_costates(const lqrx_dp_desc *desc, const void *A, const void *B, const void *Q,
                     const void *R, const void *M, const void *Qf, const void *q, const void *r,
                     const void *qf, const void *K, const void *X, const void *U, void *lam,
                     void *stream);

/* host pointers everywhere: H2D, sweep, D2H, synchronous */
int lqrx_dp_costates_host(const lqrx_dp_desc *desc, const void *A, const void *B, const void *Q,
                          const void *R, const void *M, const void *Qf, const void *q,
                          const void *r, const void *qf, const void *K, const void *X,
                          const void *U, void *lam);

/* ------------------------------------------------------------------------------------
 * Gradients through the solve (adjoint pass): for a loss ℓ(X, U) of the solution of
 * lqrx_dp_solve_cross, ∂ℓ/∂(A, B, c, Q, R, M, Qf, x0, q, r, qf) by the implicit-function theorem on
 * the KKT system.  With gX_k = ∂ℓ/∂x_k (k = 1…N) and gU_k = ∂ℓ/∂u_k (k = 1…N−1), solve the same
 * problem with q'_k = gX_k (k < N), qf' = gX_N, r'_k = gU_k, c' = 0, x0' = 0; call its solution
 * X', U' and its costates λ' (the sweep of lqrx_dp_costates on it).  Then
 *   ∂ℓ/∂A_k = λ'_{k+1} x_kᵀ + λ_{k+1} x'_kᵀ     ∂ℓ/∂B_k = λ'_{k+1} u_kᵀ + λ_{k+1} u'_kᵀ     ∂ℓ/∂c_k = λ'_{k+1}
 *   ∂ℓ/∂Q_k = ½(x'_k x_kᵀ + x_k x'_kᵀ)          ∂ℓ/∂R_k = ½(u'_k u_kᵀ + u_k u'_kᵀ)          ∂ℓ/∂M_k = u'_k x_kᵀ + u_k x'_kᵀ
 *   ∂ℓ/∂Qf  = ½(x'_N x_Nᵀ + x_N x'_Nᵀ)          ∂ℓ/∂q_k = x'_k    ∂ℓ/∂r_k = u'_k    ∂ℓ/∂qf = x'_N    ∂ℓ/∂x0 = λ'_1
 * gQ, gR, gQf are gradients with respect to the symmetric matrix (the solve reads Q, R, Qf as
 * symmetric).  x'_1 = 0, so gq_1 = 0 and gQ_1 = 0 exactly.
 *   A, B, Q, R, M, Qf   the forward problem (M required, as in lqrx_dp_solve_cross: a caller
 *                       without a cross term passes zeros and gM = NULL)
 *   X, U, lam           the forward solve's outputs and its costates (lqrx_dp_costates)
 *   grad->gX, gU        in: n·N·batch, m·(N−1)·batch
 *   grad->g*            out, each optional (NULL: not formed, and costs nothing), shaped like the
 *                       field: gQ, gR, gM, gq, gr per knot; gA, gB, gc per knot with
 *                       knot_stride_AB = 1 and summed over the knots, in ascending k, with 0
 *   info                optional: the adjoint solve's info, equal to the forward one (E does not
 *                       depend on the linear terms); gradients of a trajectory with info ≠ 0
 *                       are unspecified
 * desc.knot_stride_QR must be 1, because gX, gU sit where per-knot q, r go: a stride of 0 returns
 * LQRX_ERR_UNSUPPORTED (broadcast Q, R, M over the knots and sum gQ, gR, gM over them).
 * desc.layout = 1 returns LQRX_ERR_UNSUPPORTED (a follow-up).  desc.p_mode is ignored.
 * The call runs, all on `stream`: a repack of gX into q', qf'; the cross solve (the kernels of
 * lqrx_dp_solve_cross); the costate sweep on it; the assembly kernels.  Scratch comes from the
 * library pool and is freed in stream order: per trajectory
 *   m·n·(N−1) [K'] + 2·n·N [X', λ'] + (n + 2m)(N−1) [q', U', d'] + n·(N−1 or 1) [c'] + n² + 3n
 * elements (K' dominates: 1.05 MB per fp64 trajectory at n = 32, m = 16, N = 256).  The batch is
 * not chunked to cap it — split the batch to bound the scratch.
 * Error codes follow the argument position: desc −1, A −2, B −3, Q −4, R −5, M −6, Qf −7, X −8,
 * U −9, lam −10, grad or its members gX, gU −11, decided before the device is touched;
 * batch = 0 returns 0.  Results are the same bits from run to run (no atomics), and an output
 * has the same bits whichever other outputs are asked for.
 * There is no _host twin and no _host_devices twin of this entry.  Additive to ABI 5: detect by symbol.
 * ------------------------------------------------------------------------------------ */
typedef struct lqrx_dp_grad {
    const void *gX, *gU;                 /* in: ∂ℓ/∂X (n·N·batch), ∂ℓ/∂U (m·(N−1)·batch)   */
    void *gA, *gB, *gc;                  /* out, each optional (NULL: not formed)           */
    void *gQ, *gR, *gM, *gQf, *gx0, *gq, *gr, *gqf;
} lqrx_dp_grad;

int lqrx_dp_solve_adjoint(const lqrx_dp_desc *desc, const void *A, const void *B, const void *Q,
                          const void *R, const void *M, const void *Qf, const void *X,
                          const void *U, const void *lam, const lqrx_dp_grad *grad,
                          int32_t *info, void *stream);

/* ------------------------------------------------------------------------------------
 * Closed-loop rollout of a solved policy over many scenarios: the policy (K_k, d_k) of one solve,
 * which does not depend on x0, run from S initial states per problem, with a step length α per
 * scenario (the line-search direction u = −Kx − αd), a process disturbance w and actuator limits.
 * Per problem b and scenario j (trajectory t = b·S + j):
 *   x_1 = x0_t
 *   u_k = min(max(−K_k x_k − α_t d_k, u_lo_b), u_hi_b)
 *   x_{k+1} = A_k x_k + B_k u_k + c_k + w_{t,k}                                  k = 1 … N−1
 *   J_t = Σ_k (½x_kᵀQ_k x_k + u_kᵀM_k x_k + ½u_kᵀR_k u_k + q_kᵀx_k + r_kᵀu_k) + ½x_NᵀQf x_N + qfᵀx_N
 *   A, B        the dynamics (knot_stride_AB)
 *   c           n·batch, or n·(N−1)·batch with knot_stride_AB = 1; may be NULL (zero)
 *   K           the solve's gains, m·n·(N−1)·batch
 *   d           the solve's feedforward, m·(N−1)·batch; may be NULL (zero)
 *   cost        Q, R, M, q, r follow knot_stride_QR; Qf, qf per problem.  Needed only for J: cost may
 *               be NULL when sc->J is NULL; with J, Q, R and Qf are required, M, q, r, qf may be NULL
 *   sc          the scenarios, laid out scenario-major so that every scenario is a solve-shaped
 *               trajectory and S = 1 is exactly the solve's X / U layout:
 *                 x0_t at [t·n]            α_t at [t]          w_{t,k} at [(t·(N−1) + k−1)·n]
 *                 x_k  at [(t·N + k−1)·n]  u_k at [(t·(N−1) + k−1)·m]            J_t at [t]
 *               alpha NULL means α = 1, w NULL means no disturbance, u_lo / u_hi NULL mean no bound
 *               on that side (±inf entries are allowed in either); u_lo ≤ u_hi is a precondition and
 *               is not checked.  X, U, J are each optional, at least one is required.
 * The element type is desc.dtype; desc.p_mode is ignored.  Every (n, m ≤ 512, dtype, knot stride)
 * that lqrx_dp_solve_cross accepts is accepted, for any S ≥ 1; desc.layout = 1 returns
 * LQRX_ERR_UNSUPPORTED.  Error codes follow the argument position and are decided before the device
 * is touched: desc −1, A −2, B −3, K −5, cost −7 (J asked for and cost, or its Q, R or Qf, NULL),
 * sc −8 (sc NULL, S < 1, x0 NULL, or X, U and J all NULL; lqrx_last_error names the member);
 * batch = 0 returns 0.
 * Guaranteed:
 *   - a scenario's X, U and J are the same bits whatever S is, whatever its position j is, and
 *     whichever of X, U, J are asked for (without J no cost arithmetic is done at all);
 *   - alpha = NULL gives the bits of an all-ones alpha, u_lo = u_hi = NULL those of −inf / +inf;
 *   - results are the same bits from run to run (no atomics);
 *   - the device entry takes no scratch from the library pool: it is one kernel launch on `stream`,
 *     and can be enqueued or captured like lqrx_kkt_solve_ws.
 * Additive to ABI 5: detect by symbol.
 * ------------------------------------------------------------------------------------ */
typedef struct lqrx_dp_cost {          /* the stage / terminal cost, to form J */
    const void *Q, *R, *Qf;            /* required when J is asked for          */
    const void *M, *q, *r, *qf;        /* each may be NULL (zero)               */
} lqrx_dp_cost;

typedef struct lqrx_dp_scenarios {
    int64_t S;                         /* scenarios per problem, >= 1           */
    const void *x0;                    /* n·S·batch, required                   */
    const void *alpha;                 /* S·batch, or NULL (= 1)                */
    const void *w;                     /* n·(N−1)·S·batch, or NULL (= 0)        */
    const void *u_lo, *u_hi;           /* m·batch each, or NULL (no bound); ±inf allowed */
    void *X, *U, *J;                   /* out, each optional, at least one      */
} lqrx_dp_scenarios;

int lqrx_dp_rollout(const lqrx_dp_desc *desc, const void *A, const void *B, const void *c,
                    const void *K, const void *d, const lqrx_dp_cost *cost,
                    const lqrx_dp_scenarios *sc, void *stream);

/* host pointers everywhere (in cost and sc too): H2D, rollout, D2H of the outputs asked for, synchronous */
int lqrx_dp_rollout_host(const lqrx_dp_desc *desc, const void *A, const void *B, const void *c,
                         const void *K, const void *d, const lqrx_dp_cost *cost,
                         const lqrx_dp_scenarios *sc);

/* ------------------------------------------------------------------------------------
 * Factor once, re-solve many right-hand sides.  P_k, K_k and E_k = R_k + B_kᵀP_{k+1}B_k of a solve
 * do not depend on q, r, qf, x0: lqrx_dp_factor keeps E_k⁻¹ and g_k = P_{k+1}c_k of one solve, and
 * lqrx_dp_resolve then solves S right-hand sides (q, r, qf, x0) per problem by vector recursions
 * alone (no cost matrix is read: the cross term lives in K).  Per problem b and right-hand side j
 * (trajectory t = b·S + j):
 *   p_N = qf_t
 *   p̃   = p_{k+1} + g_k       h_k = r_{t,k} + B_kᵀp̃       d_k = E_k⁻¹h_k
 *   p_k = q_{t,k} + A_kᵀp̃ − K_kᵀh_k                                              k = N−1 … 1
 *   x_1 = x0_t,  u_k = −K_k x_k − d_k,  x_{k+1} = A_k x_k + B_k u_k + c_k          k = 1 … N−1
 * which is what lqrx_dp_solve_cross returns for that right-hand side (d, p, X, U).
 *
 * lqrx_dp_factor
 *   desc        p_mode must be 1 (0: LQRX_ERR_UNSUPPORTED)
 *   B, R        knot_stride_AB / knot_stride_QR
 *   c           as in the solve; may be NULL, then Pc must be NULL and is not formed
 *   P           the p_mode = 1 output of any solve entry: n·n·N·batch, P_N = Qf
 *   Einv        out, E_k⁻¹: m·m·(N−1)·batch, column-major, exactly symmetric
 *   Pc          out, P_{k+1}c_k: n·(N−1)·batch (NULL exactly when c is)
 *   info        optional, batch: 0, or the largest k (1-based) whose E_k is not positive definite —
 *               the knot the solve's backward sweep would report first.  Einv and Pc of such a
 *               problem are unspecified (every element is written)
 * lqrx_dp_resolve
 *   A, B, c     the dynamics (knot_stride_AB); c may be NULL exactly when fac->Pc is
 *   fac         K the solve's gains, Einv and Pc from lqrx_dp_factor
 *   rhs         laid out scenario-major exactly as in lqrx_dp_scenarios (S = 1 is the solve's layout):
 *                 q_{t,k} at [(t·(N−1) + k−1)·n] with knot_stride_QR = 1, at [t·n] with 0; r likewise with m
 *                 qf_t, x0_t at [t·n]       d_{t,k} at [(t·(N−1) + k−1)·m]
 *                 p: p_1 at [t·n] with p_mode 0, p_k at [(t·N + k−1)·n] with p_mode 1 (p_N = qf)
 *                 x_k at [(t·N + k−1)·n]    u_k at [(t·(N−1) + k−1)·m]
 *               knot_stride_QR governs only the layout of q and r here.  q, r, qf, x0 may each be
 *               NULL (zero).  d, p, X, U are each optional, at least one is required; d carries the
 *               backward pass to the forward one (the entry takes no library scratch), so X or U
 *               without d is an error on rhs.
 * Layout 0 only (desc.layout = 1: LQRX_ERR_UNSUPPORTED); 1 ≤ n ≤ 64, 1 ≤ m ≤ 32, both dtypes, both knot
 * strides; past that LQRX_ERR_UNSUPPORTED (a workgroup kernel up to 512 is a follow-up, as are
 * layout 1, a c or disturbance per right-hand side, s / dV / J per right-hand side, _host_devices
 * forms, and the use of the re-solve inside lqrx_dp_solve_adjoint; input bounds are served by
 * lqrx_dp_resolve_box below).  Error codes follow
 * the argument position and are decided before the device is touched (lqrx_last_error names the
 * member, e.g. rhs->S, fac->Einv); batch = 0 returns 0.
 *   factor:  desc −1, B −2, R −3, P −5, Einv −6, Pc −7 (Pc set without c, or NULL with c)
 *   resolve: desc −1, A −2, B −3, fac −5 (NULL, K or Einv NULL, Pc / c mismatch), rhs −6 (NULL, S < 1,
 *            no output, X or U without d)
 * Guaranteed:
 *   - a right-hand side's d, p, X, U are the same bits whatever S is, whatever its position j is,
 *     and whichever outputs are asked for;
 *   - a NULL q, r, qf or x0 gives the bits of an all-zero array;
 *   - results of both entries are the same bits from run to run (no atomics);
 *   - the device entries are one kernel launch each on `stream` and take nothing from the library's
 *     scratch pool: they can be enqueued or captured like lqrx_dp_rollout.
 * Additive to ABI 5: detect by symbol.
 * ------------------------------------------------------------------------------------ */
typedef struct lqrx_dp_factors {       /* what a re-solve needs beside A, B, c              */
    const void *K;                     /* the solve's gains, m·n·(N−1)·batch                */
    const void *Einv;                  /* E_k⁻¹, m·m·(N−1)·batch, column-major, symmetric   */
    const void *Pc;                    /* P_{k+1}c_k, n·(N−1)·batch; NULL exactly when c is */
} lqrx_dp_factors;

typedef struct lqrx_dp_rhs {
    int64_t S;                         /* right-hand sides per problem, >= 1                */
    const void *q, *r, *qf, *x0;       /* each may be NULL (zero)                           */
    void *d, *p, *X, *U;               /* out, each optional, at least one                  */
} lqrx_dp_rhs;

int lqrx_dp_factor(const lqrx_dp_desc *desc, const void *B, const void *R, const void *c,
                   const void *P, void *Einv, void *Pc, int32_t *info, void *stream);

/* host pointers: H2D, factor, D2H, synchronous */
int lqrx_dp_factor_host(const lqrx_dp_desc *desc, const void *B, const void *R, const void *c,
                        const void *P, void *Einv, void *Pc, int32_t *info);

int lqrx_dp_resolve(const lqrx_dp_desc *desc, const void *A, const void *B, const void *c,
                    const lqrx_dp_factors *fac, const lqrx_dp_rhs *rhs, void *stream);

/* host pointers everywhere (inside fac and rhs too): H2D, re-solve, D2H of the outputs asked for, synchronous */
int lqrx_dp_resolve_host(const lqrx_dp_desc *desc, const void *A, const void *B, const void *c,
                         const lqrx_dp_factors *fac, const lqrx_dp_rhs *rhs);

/* ------------------------------------------------------------------------------------
 * Input bounds u_lo ≤ u_k ≤ u_hi by ADMM on the re-solve factors.  For S instances per problem,
 *   min Σ_k (½xᵀQx + uᵀMx + ½uᵀRu + qᵀx + rᵀu) + ½x_NᵀQf x_N + qfᵀx_N
 *   subject to x⁺ = Ax + Bu + c and u_lo_b ≤ u_k ≤ u_hi_b,
 * on the factors (K, E⁻¹, Pc) of ONE solve made with R + ρI in the place of R (lqrx_dp_solve_cross,
 * p_mode = 1, then lqrx_dp_factor, both on R + ρI).  Per problem b and instance j (trajectory
 * t = b·S + j, scenario-major as in lqrx_dp_rhs), with z_{t,k}, w_{t,k} ∈ ℝᵐ for k = 1 … N−1, the
 * iteration i = 1 … max_iter is
 *   r̂_k  = r_{t,k} − ρ(z_k − w_k)
 *   (d, X, U) = the recursion of lqrx_dp_resolve on (q_t, r̂, qf_t, x0_t)
 *   û_k  = αu_k + (1 − α)z_k                                  α = relax
 *   z⁺_k = min(max(û_k + w_k, u_lo_b), u_hi_b)
 *   w⁺_k = w_k + û_k − z⁺_k
 *   r_prim = max_k ‖u_k − z⁺_k‖∞      r_dual = ρ·max_k ‖z⁺_k − z_k‖∞
 * and the instance stops after the first iteration with r_prim ≤ eps_prim and r_dual ≤ eps_dual.
 * At the fixed point z = u is the constrained optimum and y = ρ·w the multiplier of the bounds
 * (positive at an active upper bound, negative at a lower one).  Z and W are in/out: zeros are a
 * cold start, the values of the previous MPC step a warm start.  d, X, U are those of the
 * instance's last iteration (U is u, which meets the bounds to r_prim; Z meets them exactly).
 *
 *   rhs         as in lqrx_dp_resolve; d is required (it carries the backward pass to the forward
 *               one), X and U are optional, p must be NULL
 *   box->rho    > 0 and finite: the ρ the factors were made with
 *   box->relax  in [1, 2); 1 is plain ADMM
 *   box->eps_*  >= 0, absolute.  An eps of 0 never stops early: the instance runs max_iter
 *               iterations (early stopping needs both eps > 0).  A NaN residual never stops.
 *   box->max_iter  1 … 10000
 *   box->u_lo, u_hi  m·batch each, one bound per problem and input, or NULL (no bound on that
 *               side); ±inf allowed
 *   box->Z, W   in/out, m·(N−1)·S·batch each, laid out as rhs->U; required
 *   box->iters  out, optional, S·batch: the iterations the instance ran
 *   box->res    out, optional, 2·S·batch: r_prim, r_dual of its last iteration at [2t], [2t + 1]
 * The support is that of lqrx_dp_resolve: layout 0, 1 ≤ n ≤ 64, 1 ≤ m ≤ 32, both dtypes, both knot
 * strides, any S ≥ 1; anything else LQRX_ERR_UNSUPPORTED.  Error codes follow the argument position
 * and are decided before the device is touched (lqrx_last_error names the member); batch = 0
 * returns 0:
 *   desc −1, A −2, B −3, fac −5 (as in the re-solve), rhs −6 (NULL, S < 1, d NULL, p given),
 *   box −7 (NULL, rho, relax, eps_prim, eps_dual, max_iter out of range, Z or W NULL)
 * Guaranteed:
 *   - an instance's Z, W, d, X, U, iters and res are the same bits whatever S is, whatever its
 *     position j is, whichever optional outputs are asked for, and whatever the other instances do
 *     (an instance that has stopped stores nothing more);
 *   - NULL u_lo / u_hi give the bits of −inf / +inf arrays, NULL q, r, qf, x0 those of zeros;
 *   - the same bits from run to run (no atomics);
 *   - continuation is exact: with eps = 0, a run of a iterations followed by a run of b iterations
 *     on the returned Z, W gives the bits of one run of a + b;
 *   - the iteration loop is counted and bounded by max_iter;
 *   - the device entry is one kernel launch on `stream` and takes nothing from the library's
 *     scratch pool: it can be enqueued or captured like lqrx_dp_resolve.
 * Follow-ups: state or mixed constraints, a ρ per problem or an adaptive ρ (a re-factor), shapes
 * past n = 64 or m = 32, layout 1, a _host_devices form, a gradient through the constrained solve.
 * Additive to ABI 5: detect by symbol.
 * ------------------------------------------------------------------------------------ */
typedef struct lqrx_dp_box {
    double rho;                  /* > 0; the factors must come from a solve with R + rho·I           */
    double relax;                /* in [1, 2); 1 = plain ADMM                                        */
    double eps_prim, eps_dual;   /* >= 0, absolute; 0 never stops early                              */
    int32_t max_iter;            /* 1 … 10000                                                        */
    const void *u_lo, *u_hi;     /* m·batch each, or NULL (no bound on that side); ±inf allowed      */
    void *Z, *W;                 /* in/out, m·(N−1)·S·batch each, laid out as rhs->U; required       */
    int32_t *iters;              /* out, optional, S·batch: iterations this instance ran             */
    void *res;                   /* out, optional, 2·S·batch: r_prim, r_dual of its last iteration   */
} lqrx_dp_box;

int lqrx_dp_resolve_box(const lqrx_dp_desc *desc, const void *A, const void *B, const void *c,
                        const lqrx_dp_factors *fac, const lqrx_dp_rhs *rhs, const lqrx_dp_box *box,
                        void *stream);

/* host pointers everywhere (inside fac, rhs and box too): H2D (Z and W included), the iteration, D2H of Z, W
   and the outputs asked for, synchronous */
int lqrx_dp_resolve_box_host(const lqrx_dp_desc *desc, const void *A, const void *B, const void *c,
                             const lqrx_dp_factors *fac, const lqrx_dp_rhs *rhs, const lqrx_dp_box *box);

/* ------------------------------------------------------------------------------------
 * KKT path: one inner solve of CholeskySolver._solve!(solver)
 *   /root/reference/src/cholesky_solver.jl:166-182
 * = calculate_shur_factors! (jacobian_blocks.jl:220-286) → cholesky!(chol, shur)
 *   (cholesky_solve.jl:47-67) → forward_/backward_substitution! (:93-143) →
 *   calculate_primals! (cholesky_solver.jl:185-236); ginv = 0 gives the
 *   second_order_correction! variant (cholesky_solver.jl:254-273): δẑ = −Dᵀ(DDᵀ)⁻¹d.
 *
 * Block structure (shared by the whole batch) = ConstraintBlocks (conblocks.jl:403-425):
 * knot k (0-based here) has n1[k] previous-dynamics rows D2, p[k] stage rows C, n2[k]
 * dynamics rows D1 and width w[k] (= n̄ + m for k < N-1, n̄ at the last knot).
 * The four arrays are free per knot — only n1[0] = 0, n1[k] = n2[k-1] and n2[N-1] = 0 are
 * required — and Y is data.
 * Packed per-trajectory inputs, each block column-major, concatenated over k:
 *   Y  (n1+p+n2)×w   Y = [D2; C; D1]   (ConstraintBlock.Y)
 *   y  p+n2          y = [c; d]        (ConstraintBlock.y)
 *   H  h_mode 0/1: w×w cost Hessian (dense / block-diagonal Q,R; BlockCholesky modes,
 *      block_cholesky.jl:55-77);  h_mode 2: the w diagonal entries (:82-91)
 *   g  w             gradient [q; r]  (InvertedQuadratic gradient, block_cholesky.jl:126)
 * Outputs:
 *   dz  w per knot  (δZ, get_step ordering [x1;u1;…;xN])
 *   lam p+n2 per knot  [μ_k; λ_k]  (get_multipliers ordering)
 *   info int32·batch: 0 ok; k+1 if a Schur diagonal block at knot k was not SPD;
 *        −(k+1) if H_k was not SPD.
 * ------------------------------------------------------------------------------------ */
typedef struct lqrx_kkt_desc {
    int32_t N;          /* knots                                                  */
    int32_t dtype;      /* LQRX_F64 (every KKT kernel: the compile-time shapes, the
                           padded bins for trajectory structures up to n̄ <= 8, m <= 4
                           — dense / block-diagonal H on both through an H = UᵀU
                           pre/post pass — then the large-block and workgroup kernels)
                           or LQRX_F32 (layout 0: the
                           large-block MFMA kernels for n1, p, n2 <= 64, padded rows
                           <= 128, w <= 128, and the workgroup-per-trajectory kernel
                           past them; every h_mode and ginv; else
                           LQRX_ERR_UNSUPPORTED).  Every knot: n1, p, n2 <= 512 and
                           w <= 1024 (LQRX_ERR_UNSUPPORTED past that)               */
    int64_t batch;
    const int32_t *n1;  /* [N] host arrays describing the block structure           */
    const int32_t *p;   /* [N]                                                      */
    const int32_t *n2;  /* [N]                                                      */
    const int32_t *w;   /* [N]                                                      */
    int32_t h_mode;     /* 0 dense, 1 block-diagonal, 2 diagonal                    */
    int32_t ginv;       /* 1 = _solve!;  0 = second-order-correction variant        */
    int32_t layout;     /* 0 = per-trajectory packed, batch slowest: element e of
                           trajectory t's packed array (Y, y, H, g, dz, lam) at
                           [t·len + e];  1 = batch fastest (SoA) at [e·batch + t] —
                           a wave's 64 trajectories read each element as one 512-B
                           row.  Layout 1 is read natively by the compile-time shapes,
                           (n̄, m, p_first, p_interior, p_last) = Dubins (3,2,3,0,3) every
                           h_mode; cartpole (4,1,4,0,4), DoubleIntegrator(2)/(3)
                           (4,2,4,1,4)/(6,3,6,1,6), trajectory_structure(5,2,N) /
                           (7,3,N) (5,2,5,0,5)/(7,3,7,0,7) with diagonal H or ginv = 0;
                           fp64; N >= 4.  Every other layout-1 call is staged: the
                           arrays are transposed to layout 0 in library scratch, solved
                           by the layout-0 kernels and dz / lam transposed back (2x
                           the bytes).  Layout 1 arrays < 2 GiB.                      */
    int32_t reserved;
} lqrx_kkt_desc;

int lqrx_kkt_solve(const lqrx_kkt_desc *desc, const void *Y, const void *y, const void *H,
                   const void *g, void *dz, void *lam, int32_t *info, void *stream);
int lqrx_kkt_solve_host(const lqrx_kkt_desc *desc, const void *Y, const void *y,
                        const void *H, const void *g, void *dz, void *lam, int32_t *info);
/* Caller-provided workspace (the factor slab): no allocation inside the call — the form a
 * serving loop or a captured hipGraph wants.  lqrx_kkt_workspace_size gives the bytes this
 * structure and batch need (0 for batch 0); lqrx_kkt_solve_ws returns -10 if
 * workspace_bytes is smaller.  One workspace must not be shared by calls in flight on
 * different streams (lqrx_kkt_solve draws stream-ordered scratch from a library pool).
 * Large blocks: the slab (+ Schur images) is sized for the batch but capped at
 * LQRX_KKT_BIG_SLAB_MB (default 40 GiB); a larger batch runs in chunks through it.  Without
 * a caller workspace that scratch comes from the library pool, whose freed blocks stay
 * reserved for the next call (up to the cap) until lqrx_scratch_trim; an out-of-memory pool
 * allocation retries with halved chunks.  A layout-1 call whose structure has no native SoA
 * kernel is staged through layout 0: its six transposed arrays (Y y H g, δz λ) are part of
 * the workspace too (counted by lqrx_kkt_workspace_size, carved from its front), so a _ws call
 * draws no pool scratch in any layout. */
int lqrx_kkt_workspace_size(const lqrx_kkt_desc *desc, size_t *bytes);
int lqrx_kkt_solve_ws(const lqrx_kkt_desc *desc, const void *Y, const void *y, const void *H,
                      const void *g, void *dz, void *lam, int32_t *info, void *workspace,
                      size_t workspace_bytes, void *stream);
/* sizes (elements per trajectory) of the packed KKT buffers, for allocation */
int lqrx_kkt_sizes(const lqrx_kkt_desc *desc, int64_t *nY, int64_t *ny, int64_t *nH,
                   int64_t *ng, int64_t *nlam);

/* ------------------------------------------------------------------------------------
 * Multi-device host entries — SURVEY.md §8(e): "the batch of independent problems shards
 * embarrassingly across the 8 GPUs of one node".  Same arguments and results as the *_host
 * call they extend (lqrx_dp_solve_host, lqrx_dp_solve_linear_host, lqrx_kkt_solve_host; the
 * reference's solve! per shard, dynamic_programming.jl:54-72 / cholesky_solver.jl:166-182),
 * plus devices[ndev]: HIP device ordinals, repeats allowed (two shards on one GPU).  The batch
 * is split into ndev contiguous shards (trajectories [b0, b0 + nb), the first batch mod ndev
 * shards one longer); each runs concurrently on its own thread and non-blocking stream on its
 * device: its slice of every input is copied in (layout 1: the strided slice of every element
 * row), solved by the single-device path, and K/P/X/U (δz/λ) and info land in the caller's
 * host arrays at the shard's offset.  No collective and no peer traffic: the gather IS the
 * D2H into the caller's arrays.  Every trajectory is solved exactly as by the single-device
 * call, so results are bit-identical (n ≤ 4 DP: when the shard batches pick the same quad /
 * lane kernel as the whole batch, ≤ 16384 trajectories per shard or > 16384 in both).
 * Returns -13 / -14 (dp), -14 / -15 (dp linear), -9 / -10 (kkt) for a NULL devices / an
 * entry that is not a device, and ndev < 1; a failing shard's status, with its device and
 * trajectory range in lqrx_last_error; 1 if any trajectory has info != 0. */
int lqrx_dp_solve_host_devices(const lqrx_dp_desc *desc, const void *A, const void *B, const void *Q,
                               const void *R, const void *Qf, const void *x0, void *K, void *P,
                               void *X, void *U, int32_t *info, const int32_t *devices, int32_t ndev);
int lqrx_dp_solve_linear_host_devices(const lqrx_dp_desc *desc, const void *A, const void *B,
                                      const void *Q, const void *R, const void *Qf, const void *x0,
                                      const lqrx_dp_linear *lin, void *K, void *P, void *X, void *U,
                                      int32_t *info, const int32_t *devices, int32_t ndev);
int lqrx_kkt_solve_host_devices(const lqrx_kkt_desc *desc, const void *Y, const void *y,
                                const void *H, const void *g, void *dz, void *lam, int32_t *info,
                                const int32_t *devices, int32_t ndev);

/* ------------------------------------------------------------------------------------
 * Batched trajectory-optimisation SQP around the KKT path: per
 * trajectory, the outer loop of CholeskySolver.solve!/step! (/root/reference/src/
 * cholesky_solver.jl:109-153) with the KKT inputs assembled on the device (update!, :155-164:
 * RK3 dynamics Jacobians, diagonal LQRObjective expansion), _solve! (:166-182), and the
 * L1-merit backtracking line search with second-order correction of test/dubins_sqp.jl:58-97
 * (SOC = second_order_correction!, cholesky_solver.jl:254-273).
 *
 * Models (continuous dynamics, integrated with RobotDynamics' RK3 at step dt; Jacobians by
 * forward-mode dual numbers on the device, as ForwardDiff does in the reference):
 *   LQRX_MODEL_DUBINS   nx 3, nu 2: RobotZoo.DubinsCar ẋ = [v cosθ, v sinθ, ω]
 *                       (test/dubins_sqp.jl); params unused
 *   LQRX_MODEL_CARTPOLE nx 4, nu 1: RobotZoo.Cartpole, x = [x, θ, ẋ, θ̇],
 *                       params = {mc, mp, l, g} (RobotZoo defaults 1, 0.2, 0.5, 9.81;
 *                       test/problems.jl:58-88 Cartpole())
 *   LQRX_MODEL_DOUBLE_INTEGRATOR{1,2,3}  nx 2D, nu D: RobotZoo.DoubleIntegrator(D),
 *                       ẋ = [q̇; u] (test/problems.jl:14-56 DoubleIntegrator(D)); params unused
 * Problem: min Σ_{k<N} ½(x_k−xf)ᵀQ(x_k−xf) + ½u_kᵀRu_k + ½(x_N−xf)ᵀQf(x_N−xf)
 *          s.t. x_1 = x0, x_{k+1} = rk3(x_k, u_k), x_N = xf      (Q, R, Qf diagonal)
 *          and, when stage_rows > 0, A_s x_k = b_s on the interior knots k = 2..N−1 (the
 *          LinearConstraint DoubleIntegrator() adds on 2:N−1; A_s shared by the batch)
 * Buffers (device; layout 0, batch slowest), nx / nu of the model:
 *   Z      (N·nx + (N−1)·nu)·batch in/out: z = [x_1; u_1; …; x_{N−1}; u_{N−1}; x_N]
 *          (the KKT δz order)
 *   x0, xf nx·batch
 *   lam    (nx(N+1) + stage_rows(N−2))·batch out: multipliers of the last accepted Newton
 *          step (KKT λ order); unspecified for a trajectory with iters = 0 (no step accepted)
 *   iters  int32·batch out: accepted steps
 *   status int32·batch out: 0 converged (‖c‖∞ < tol_p and ‖∇f+∇cᵀλ‖₂ < tol_d before a
 *          step), 1 max_iters reached, 2 line search failed (iterate left unchanged)
 * Validation (-1): beside the ranges noted at the fields, a problem with more constraint rows
 * than variables, N·nx + (N−1)·nu < nx·(N+1) + stage_rows·(N−2), is rejected — its Newton
 * KKT matrix is singular at every point (the reference raises PosDefException).  That rules
 * out a stage row on the cartpole or DoubleIntegrator(1), Dubins with N = 2, cartpole with N < 5.
 * ------------------------------------------------------------------------------------ */
enum {
    LQRX_MODEL_DUBINS = 0,
    LQRX_MODEL_CARTPOLE = 1,
    LQRX_MODEL_DOUBLE_INTEGRATOR1 = 2,
    LQRX_MODEL_DOUBLE_INTEGRATOR2 = 3,
    LQRX_MODEL_DOUBLE_INTEGRATOR3 = 4
};

typedef struct lqrx_sqp_desc {
    int32_t model;          /* LQRX_MODEL_*                                            */
    int32_t N;              /* knots (>= 2)                                            */
    int32_t max_iters;      /* CholeskySolver.solve!: 10                               */
    int32_t stage_rows;     /* rows of the interior linear constraint, 0..2 (nx·rows ≤ 32) */
    int64_t batch;
    double dt;              /* tf / (N−1)                                              */
    double Q[8], R[8], Qf[8]; /* diagonal cost weights (> 0), first nx / nu used         */
    double params[4];       /* model parameters (see above)                            */
    double mu;              /* L1 merit weight (dubins_sqp.jl:59 uses 1)               */
    double tol_p, tol_d;    /* 1e-5, 1e-5 (cholesky_solver.jl:131-132)                 */
    double stage_A[32];     /* A_s, stage_rows × nx column-major                        */
    double stage_b[4];      /* b_s                                                      */
} lqrx_sqp_desc;

/* state / control dimension of a model; -1 for an unknown model */
int lqrx_sqp_model_dims(int32_t model, int32_t *nx, int32_t *nu);
int lqrx_sqp_solve(const lqrx_sqp_desc *desc, double *Z, const double *x0, const double *xf,
                   double *lam, int32_t *iters, int32_t *status, void *stream);
int lqrx_sqp_solve_host(const lqrx_sqp_desc *desc, double *Z, const double *x0, const double *xf,
                        double *lam, int32_t *iters, int32_t *status);

/* The round-1 Dubins-only entry points (model fixed to LQRX_MODEL_DUBINS); they forward to
 * lqrx_sqp_solve[_host]. */
typedef struct lqrx_dubins_sqp_desc {
    int32_t N;
    int32_t max_iters;
    int64_t batch;
    double dt;
    double Q[3], R[2], Qf[3];
    double mu;
    double tol_p, tol_d;
} lqrx_dubins_sqp_desc;

int lqrx_dubins_sqp_solve(const lqrx_dubins_sqp_desc *desc, double *Z, const double *x0,
                          const double *xf, double *lam, int32_t *iters, int32_t *status,
                          void *stream);
int lqrx_dubins_sqp_solve_host(const lqrx_dubins_sqp_desc *desc, double *Z, const double *x0,
                               const double *xf, double *lam, int32_t *iters, int32_t *status);

/* ------------------------------------------------------------------------------------
 * Condensed least-squares LQR: replaces
 * solve!(sol, ::LeastSquaresSolver, prob) (/root/reference/src/least_squares.jl:158-192)
 * with opts :solve_type => :cholesky — Ā/b̄ as buildAb! builds them (:58-103),
 * H = ĀᵀĀ + Hu, y = −Āᵀb̄ (:171-173), potrf/potrs 'U' (:181-182), rollout! (:197-202).
 * One workgroup per trajectory.  (N−1)·m ≤ 192 and lqrx_ls_lds_bytes(n, m, N) <= 163840
 * (e.g. n=4, m=1: N ≤ 189; n=3, m=2: N ≤ 97): the whole problem in LDS.  Larger problems up to
 * (N−1)·m ≤ 1024 keep H in stream-ordered global scratch (Nm(Nm+1)/2 doubles per trajectory)
 * with a blocked factor — e.g. the reference's own LS test problem, DoubleIntegrator()
 * n=6, m=3, N=101 (Nm = 300); lqrx_ls_lds_bytes reports the LDS of the path taken.
 *   hu_mode 0: Hu = 0 — a fresh LeastSquaresSolver (:44), the reference default; the
 *              solve then carries no control cost
 *           1: Hu = blkdiag(chol(R).U) — what build_least_squares! leaves (:121)
 *           2: Hu = blkdiag(R) — the LQR cost; U then equals the DP rollout (extension)
 * Inputs (device, layout 0, batch slowest, time-invariant): A n×n, B n×m, Q n×n, R m×m,
 * Qf n×n, x0 n.  Outputs: U (N−1)·m per trajectory (sol.U_), X N·n (sol.X);
 * Abar (N·n)×((N−1)·m) col-major and bbar N·n per trajectory when non-NULL (buildAb!'s Ā,
 * b̄, for checks).  info[b]: 0 ok, j > 0 = potrf pivot j of H not positive, −1 = Q, Qf
 * (or R for hu_mode 1) not positive definite (cholesky() throws there, :50-52).
 * Return: 0 ok, 1 some info ≠ 0 (synchronous calls only), < 0 as above.
 * ------------------------------------------------------------------------------------ */
typedef struct lqrx_ls_desc {
    int32_t n, m, N;
    int32_t hu_mode;
    int64_t batch;
} lqrx_ls_desc;

size_t lqrx_ls_lds_bytes(int32_t n, int32_t m, int32_t N);
int lqrx_ls_solve(const lqrx_ls_desc *desc, const double *A, const double *B, const double *Q,
                  const double *R, const double *Qf, const double *x0, double *U, double *X,
                  int32_t *info, double *Abar, double *bbar, void *stream);
int lqrx_ls_solve_host(const lqrx_ls_desc *desc, const double *A, const double *B,
                       const double *Q, const double *R, const double *Qf, const double *x0,
                       double *U, double *X, int32_t *info);

/* ------------------------------------------------------------------------------------
 * Utilities
 * ------------------------------------------------------------------------------------ */
int lqrx_abi_version(void);
/* "src_sha256=<SHA-256 of the library's sources> abi=<n> arch=gfx950 built=<date time>": the
 * hash covers lqr.jl_amd/csrc/{*.hip,*.h,*.cpp} (sorted by name) then include/lqrx.h, so a
 * caller can check that the loaded binary was built from the sources beside it */
const char *lqrx_build_info(void);
const char *lqrx_last_error(void);
/* copy the calling thread's last error message into buf (NUL-terminated, truncated to
 * len-1 bytes); returns the full message length.  For bindings that cannot hold a
 * pointer into library memory (SURVEY.md §8(b) lqrx_get_last_error). */
int lqrx_get_last_error(char *buf, size_t len);
/* 1 if the HIP runtime sees a gfx950 device, else 0 (no compute; safe without a GPU) */
int lqrx_device_available(void);
/* Return the library pool's unused stream-ordered scratch of `device` (-1: every device
 * the library has used) to the driver, keeping at most keep_bytes reserved.  Blocks still in
 * use by enqueued work are not affected.  Returns 0, or LQRX_ERR_HIP. */
int lqrx_scratch_trim(int32_t device, size_t keep_bytes);

/* Deterministic synthetic random-dense LQR batch: counter-based
 * splitmix64 + Box–Muller keyed by (seed, trajectory, field, element); host memory,
 * multi-threaded.  A = I + (0.1/√n)G, B = G/√n, Q = I + GᵀG/n, R = I + GᵀG/m, Qf = 10Q,
 * x0 ~ N(0,1).  traj0 offsets the trajectory index (to generate one shard of a batch). */
int lqrx_make_random_dp(int32_t n, int32_t m, int64_t batch, int64_t traj0, uint64_t seed,
                        int32_t dtype, void *A, void *B, void *Q, void *R, void *Qf,
                        void *x0);

#ifdef __cplusplus
}
#endif
#endif /* LQRX_H */
