// lqrx_internal.h — kernel argument blocks shared by the launchers and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <vector>
#include <stdint.h>

namespace lqrx {

struct DpArgs {
    const void *A, *B, *Q, *R, *Qf, *x0; // device inputs, layout 0
    void *K, *P, *X, *U;                 // device outputs
    int32_t *info;                       // device [batch] or null
    int n, m, N;
    int dtype; // 0 f64, 1 f32
    int p_all;
    int64_t batch;
    int tv_AB, tv_QR; // 1 = per-knot A_k,B_k / Q_k,R_k (N−1 knots per trajectory), 0 = time-invariant
    int layout;       // 0 = per-trajectory blocks, batch slowest; 1 = batch fastest (SoA):
                      // element e of trajectory b at [e·batch + b] (e = the layout-0 offset
                      // within the trajectory) — native in the n ≤ 4 kernels
    // linear cost terms (lqrx_dp_solve_linear; lin = 0: the plain reference problem):
    // q, r per knot with tv_QR (knot stride n / m), qf; outputs d (m per knot), p (n, or
    // n per knot with p_all)
    int lin;
    const void *q, *r, *qf;
    void *d, *p;
    // tests only (LQRX_DP_NS_OFF=1, read by dp_launch): no Newton–Schulz step, every knot takes the
    // exact LDLᵀ sweep — exercises the sweep / verdict paths of the MFMA kernels at every knot
    int ns_off;
    // affine dynamics x⁺ = A x + B u + c (lqrx_dp_solve_affine; needs lin = 1): c per knot with
    // tv_AB (knot stride n, knot k at k−1, like A and B), n per trajectory otherwise.  (Last, so
    // that every earlier field keeps its kernel-argument offset.)
    int aff;
    const void *c;
    // cost cross term uᵀMx (lqrx_dp_solve_cross; needs lin = 1 and aff = 1): M is m×n column-major,
    // per knot with tv_QR (knot stride m·n, knot k at k−1, like Q and R), m·n per trajectory
    // otherwise.  G = BᵀPA + M_k.  (Appended: every earlier field keeps its offset.)
    int cross;
    const void *M;
    // value-function constant (lqrx_dp_solve_value; needs lin = aff = cross = 1): vs receives s_1
    // (batch) or, with p_all, every s_k (N per trajectory, knot k at k−1, s_N = 0; layout as p);
    // vdV, if not null, Σ_k h_kᵀd_k (batch).  Batch vectors are the same in both layouts.
    // (Appended: every earlier field keeps its offset.)
    int value;
    void *vs, *vdV;
};

// The DP solve kinds nest: each adds arguments to the one before it (lin; c; M; val).
enum DpKind { DP_PLAIN, DP_LINEAR, DP_AFFINE, DP_CROSS, DP_VALUE };
// the kind that a.lin / a.aff / a.cross / a.value spell, or −1 when the flags do not nest (dp_launch,
// alone among the launchers, checks that and hands the kind down)
inline int dp_kind(const DpArgs &a)
{
    const int f[4] = {a.lin != 0, a.aff != 0, a.cross != 0, a.value != 0};
    return f[0] >= f[1] && f[1] >= f[2] && f[2] >= f[3] ? f[0] + f[1] + f[2] + f[3] : -1;
}
// Run-time value → compile-time constant, for the launchers: f is a generic lambda that returns
// hipError_t; it reads its argument as decltype(x)::value (a bool, a kind) or decltype(x) (the type).
template <typename F> hipError_t with_bool(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <typename F> hipError_t with_bools(bool b, bool c, F &&f)
{
    return with_bool(b, [&](auto x) { return with_bool(c, [&](auto y) { return f(x, y); }); });
}
template <typename F> hipError_t with_dtype(int dtype, F &&f) { return dtype == 0 ? f(double{}) : f(float{}); }
template <int K> using IntC = std::integral_constant<int, K>;
template <typename F> hipError_t with_kind(int kind, F &&f)
{
    return kind == DP_PLAIN ? f(IntC<DP_PLAIN>{}) : kind == DP_LINEAR ? f(IntC<DP_LINEAR>{})
         : kind == DP_AFFINE ? f(IntC<DP_AFFINE>{}) : kind == DP_CROSS ? f(IntC<DP_CROSS>{})
         : kind == DP_VALUE ? f(IntC<DP_VALUE>{}) : hipErrorInvalidValue;
}
// the register tiles of n ≤ 64 states and m ≤ 32 inputs: f(IntC<NT>, IntC<MT>), NT of 1, 2, 4 and MT of 1, 2
template <typename F> hipError_t with_tiles(int n, int m, F &&f)
{
    const auto mt = [&](auto nt) { return m <= 16 ? f(nt, IntC<1>{}) : f(nt, IntC<2>{}); };
    return n <= 16 ? mt(IntC<1>{}) : n <= 32 ? mt(IntC<2>{}) : mt(IntC<4>{});
}
hipError_t dp_launch(const DpArgs &a, hipStream_t s);
// J = V_1(x0) = ½x0ᵀP_1x0 + p_1ᵀx0 + s_1 behind a value solve (lqrx_dp.hip): one thread per
// trajectory on a's P, p, vs and x0 in a's layout, accumulated in double, written to J (batch)
hipError_t dp_value_cost_launch(const DpArgs &a, void *J, hipStream_t s);
// out = inᵀ for a rows × cols row-major matrix of 4- or 8-byte elements (lqrx_layout.hip):
// layout 1 (SoA, [S][batch]) ↔ layout 0 ([batch][S]) for the kernels that need layout 0
hipError_t batch_transpose(const void *in, void *out, int64_t rows, int64_t cols, int elem_bytes, hipStream_t s);
bool dp_supported(int dtype, int n, int m, bool tv);
// Workspace of a canonical-form solve (lqrx_dp_canon.hip writes it, dp_riccati_kernel's VAR_CANON /
// VAR_MASK / VAR_PREFB / VAR_DIAG variants read it): one int32 flag per trajectory (3: canonical with the
// pre-feedback in the basis where A₂₁ is diagonal, 2: canonical with the pre-feedback, 1: canonical,
// 0: generic), then per trajectory Ã, Q̃, Q̃f, Tᵀ (n² each), R̃, Sᵀ (m² each), column-major.  A flag-2 or
// flag-3 trajectory has Q′ in Q̃'s place and behind Sᵀ M′ (m×n, column-major) and C (m×n, as the lanes
// hold its tiles: tile, lane, register).  Behind the last trajectory's block, m doubles per trajectory:
// σ, A₂₁'s diagonal, of a flag-3 trajectory (a region of its own, so that the blocks keep their stride
// and the kernels that read them their code).  It reaches those kernels in
// DpArgs::M — a plain solve has no cross term, so M is otherwise unread there — and DpArgs, with it
// every other kernel's argument block, stays as it is.
template <typename T, int NT, int MT> struct DpCanonWs {
    static constexpr size_t nn = (size_t)256 * NT * NT, mm = (size_t)256 * MT * MT, nm = (size_t)256 * NT * MT;
    static constexpr size_t oA = 0, oQ = nn, oQf = 2 * nn, oTt = 3 * nn, oR = 4 * nn, oSt = 4 * nn + mm;
    static constexpr size_t oMp = 4 * nn + 2 * mm, oC = oMp + nm;
    static constexpr size_t per = 4 * nn + 2 * mm + 2 * nm;            // elements per trajectory
    static __host__ __device__ size_t flag_bytes(int64_t batch) { return ((size_t)batch * 4 + 255) / 256 * 256; }
    static __host__ __device__ size_t sigma_off(int64_t batch) { return flag_bytes(batch) + (size_t)batch * per * sizeof(T); }
    static __host__ __device__ size_t bytes(int64_t batch) { return sigma_off(batch) + (size_t)batch * 16 * MT * sizeof(T); }
    static __host__ __device__ int32_t *flags(void *ws) { return (int32_t *)ws; }
    static __host__ __device__ const int32_t *flags(const void *ws) { return (const int32_t *)ws; }
    static __host__ __device__ T *block(void *ws, int64_t batch, int64_t b)
    {
        return (T *)((char *)ws + flag_bytes(batch)) + (size_t)b * per;
    }
    static __host__ __device__ const T *block(const void *ws, int64_t batch, int64_t b)
    {
        return (const T *)((const char *)ws + flag_bytes(batch)) + (size_t)b * per;
    }
    static __host__ __device__ T *sigma(void *ws, int64_t batch, int64_t b)
    {
        return (T *)((char *)ws + sigma_off(batch)) + (size_t)b * 16 * MT;
    }
    static __host__ __device__ const T *sigma(const void *ws, int64_t batch, int64_t b)
    {
        return (const T *)((const char *)ws + sigma_off(batch)) + (size_t)b * 16 * MT;
    }
};
// the canonical-form solve of a plain time-invariant fp64 n = 32, m = 16, P_1-only call (lqrx_dp_canon.hip):
// set-up, VAR_DIAG kernel, VAR_PREFB kernel, VAR_CANON kernel, VAR_MASK kernel.  *ran = false (and nothing launched,
// hipSuccess) when the pool cannot give the workspace: the caller then takes the generic launch.
hipError_t dp_canon_launch(const DpArgs &a, hipStream_t s, bool *ran);
// the VAR_CANON | VAR_PREFB instantiation's launch (lqrx_dp_prefb.hip, a module of its own), on the
// workspace in a.M, over the whole batch
hipError_t dp_prefb_launch(const DpArgs &a, hipStream_t s);
// κ∞(B₁) bound of the canonical form in fp64: a factor 4 under the end of the conditioning sweep of
// tests/dp_canon_truth.py, which reached cond(B) = 1e14 with the canonical gain still under a tenth
// of the 1e-10 tolerance
constexpr double DP_CANON_KAPPA_F64 = 2.5e13;
// κ∞(B₁) bound of the pre-feedback tier (VAR_PREFB): Q′ carries A₁ᵀR̃A₁, which −GᵀK_v cancels again, and
// R̃ = SᵀRS grows like κ(B₁)², so digits go in proportion.  A factor 4 under the point of the sweep of
// tests/dp_canon_pf_truth.py where the modelled gain error first reaches 1e-11
constexpr double DP_PREFB_KAPPA_F64 = 4.7e2;
// the VAR_CANON | VAR_PREFB | VAR_DIAG instantiation's launch (lqrx_dp_diag.hip, a module of its own), likewise
hipError_t dp_diag_launch(const DpArgs &a, hipStream_t s);
// κ∞(B₁) bound of the diagonal-A₂₁ tier (VAR_DIAG): the rotation U₁ mixes Ẽ's graded basis, and the
// Newton–Schulz acceptance on max |I − EX| then leaves more of the residual in the gain.  A factor 4 under
// the point of the sweep of tests/dp_canon_dg_truth.py where the modelled gain error first reaches 1e-11
// 
constexpr double DP_DIAG_KAPPA_F64 = 1.4e2;
// the set-up's one-sided Jacobi on A₂₁ (lqrx_dp_canon.hip): cap on sweeps, rotation threshold on
// |w_p·w_q| / (‖w_p‖‖w_q‖) in units of ε, admission bound on the recomputed block's off-diagonal in units
// of ε·σ_max (4n: two chained n-term products with orthogonal factors, ‖A‖₂ up to twice σ_max) and the
// range of σ in which the threshold's products neither underflow nor overflow
constexpr int DP_DIAG_SWEEPS = 12;
constexpr double DP_DIAG_ROT_EPS = 16.0, DP_DIAG_OFF_EPS = 128.0, DP_DIAG_SIGMA_LO = 1e-60, DP_DIAG_SIGMA_HI = 1e60;
// lane-per-trajectory kernel for n ≤ 4, m ≤ 4 (lqrx_dp_lane.hip)
hipError_t dp_lane_launch(const DpArgs &a, int kind, hipStream_t s);
bool dp_lane_supported(int n, int m);
// workgroup-per-trajectory kernel for shapes past the register tiles (lqrx_dp_big.hip):
// n > 64 or m > 32, up to 512 each
hipError_t dp_big_launch(const DpArgs &a, hipStream_t s);
bool dp_big_supported(int n, int m);

// ---- costates and the adjoint pass (lqrx_dp_adjoint.hip), layout 0 only ----
// λ_N = Qf x_N + qf,  λ_k = Q_k x_k + M_kᵀu_k + q_k + A_kᵀλ_{k+1} − K_kᵀ(R_k u_k + M_k x_k + r_k + B_kᵀλ_{k+1})
// (the bracket is the stationarity condition, zero at the solution: the closed-loop, stable form
// of the sweep): lam laid out like X.  M, q, r, qf may be null (zero).  Q, R, M, q, r follow tv_QR,
// A, B follow tv_AB; K is the solve's gain, per knot.
struct DpCostateArgs {
    const void *A, *B, *Q, *R, *M, *Qf, *q, *r, *qf, *K, *X, *U;
    void *lam;
    int n, m, N;
    int dtype; // 0 f64, 1 f32
    int tv_AB, tv_QR;
    int64_t batch;
};
hipError_t dp_costate_launch(const DpCostateArgs &a, hipStream_t s);
// gX (n·N per trajectory) → q' (n·(N−1) per trajectory), qf' (n per trajectory)
hipError_t dp_adjoint_pack_launch(const void *gX, void *q, void *qf, int n, int N, int64_t batch, int dtype,
                                  hipStream_t s);
// Rank-2 assembly of the gradients from the forward (X, U, lam) and adjoint (Xa, Ua, lama)
// trajectories; every output may be null (not formed).  gA, gB, gc are per knot with tv_AB, else
// summed over the knots in ascending k; gQ, gR, gM, gq, gr are per knot.
struct DpGradArgs {
    const void *X, *U, *lam, *Xa, *Ua, *lama;
    void *gA, *gB, *gc, *gQ, *gR, *gM, *gQf, *gx0, *gq, *gr, *gqf;
    int n, m, N;
    int dtype;
    int tv_AB;
    int64_t batch;
};
hipError_t dp_grad_launch(const DpGradArgs &a, hipStream_t s);

// ---- closed-loop rollout of a policy over S scenarios per problem (lqrx_dp_scen.hip), layout 0 only ----
// Trajectory t = b·S + j: x_1 = x0_t, u_k = clamp(−K_k x_k − α_t d_k, u_lo_b, u_hi_b),
// x_{k+1} = A_k x_k + B_k u_k + c_k + w_{t,k}; J_t the cost of the trajectory.  A, B, c follow tv_AB,
// Q, R, M, q, r follow tv_QR; K and d are the solve's, per knot.  X, U, J are laid out per trajectory
// like a solve's outputs with batch·S trajectories.  Takes no scratch.
struct DpScenArgs {
    const void *A, *B, *c, *K, *d;              // c, d may be null (zero)
    const void *Q, *R, *Qf, *M, *q, *r, *qf;    // read only when J is set; M, q, r, qf may be null (zero)
    const void *x0, *alpha, *w, *u_lo, *u_hi;   // alpha (null: 1), w (null: 0), u_lo / u_hi (null: no bound)
    void *X, *U, *J;                            // each may be null (not formed)
    int n, m, N;
    int dtype; // 0 f64, 1 f32
    int tv_AB, tv_QR;
    int64_t batch, S;
};
hipError_t dp_scen_launch(const DpScenArgs &a, hipStream_t s);

// ---- factor once, re-solve S right-hand sides per problem (lqrx_dp_resolve.hip), layout 0, n ≤ 64, m ≤ 32 ----
// Factor: E_k⁻¹ (m·m per knot, symmetric) and, with c, Pc_k = P_{k+1}c_k (n per knot) from the p_all P
// of a solve; info (may be null) the largest knot whose E is not positive definite.  B, c follow
// tv_AB, R follows tv_QR.  One kernel, no scratch.
struct DpFactorArgs {
    const void *B, *R, *c, *P;   // c null exactly when Pc is
    void *Einv, *Pc;
    int32_t *info;
    int n, m, N;
    int dtype; // 0 f64, 1 f32
    int tv_AB, tv_QR;
    int64_t batch;
};
hipError_t dp_factor_launch(const DpFactorArgs &a, hipStream_t s);
// Re-solve: trajectory t = b·S + j: p_N = qf_t, p̃ = p_{k+1} + Pc_k, h = r_{t,k} + B_kᵀp̃, d_k = E_k⁻¹h,
// p_k = q_{t,k} + A_kᵀp̃ − K_kᵀh; x_1 = x0_t, u_k = −K_k x_k − d_k, x_{k+1} = A_k x_k + B_k u_k + c_k.
// A, B, c follow tv_AB; tv_QR is the knot stride of q and r alone.  q, r, qf, x0 may be null (zero);
// d, p (n, or n·N with p_all), X, U may be null (not formed), X or U needs d.  One kernel, no scratch.
struct DpResolveArgs {
    const void *A, *B, *c, *K, *Einv, *Pc;
    const void *q, *r, *qf, *x0;
    void *d, *p, *X, *U;
    int n, m, N;
    int dtype; // 0 f64, 1 f32
    int tv_AB, tv_QR, p_all;
    int64_t batch, S;
};
hipError_t dp_resolve_launch(const DpResolveArgs &a, hipStream_t s);
bool dp_resolve_supported(int n, int m);

// ---- input bounds by ADMM on the re-solve factors (lqrx_dp_box.hip), the support of the re-solve ----
// Per instance t = b·S + j, iteration 1 … max_iter: r̂_k = r_{t,k} − ρ(z_k − w_k), the re-solve recursion on
// (q, r̂, qf, x0) with the factors of R + ρI, û = αu + (1 − α)z, z⁺ = min(max(û + w, u_lo_b), u_hi_b),
// w⁺ = w + û − z⁺; the instance stops after the first iteration with max‖u − z⁺‖∞ ≤ eps_prim and
// ρ·max‖z⁺ − z‖∞ ≤ eps_dual (an eps of 0 never stops early; a NaN never stops).  The first two rows as in
// DpResolveArgs.  u_lo, u_hi (m per problem) may be null (no bound); d, Z, W (m·(N−1) per instance,
// Z and W in/out) are required; X, U, iters (per instance), res (2 per instance) may be null.
// One kernel, no scratch.
struct DpBoxArgs {
    const void *A, *B, *c, *K, *Einv, *Pc;
    const void *q, *r, *qf, *x0;
    const void *u_lo, *u_hi;
    void *d, *X, *U, *Z, *W, *res;
    int32_t *iters;
    double rho, relax, eps_prim, eps_dual;
    int max_iter;
    int n, m, N;
    int dtype; // 0 f64, 1 f32
    int tv_AB, tv_QR;
    int64_t batch, S;
};
hipError_t dp_box_launch(const DpBoxArgs &a, hipStream_t s);

struct KktArgs {
    const double *Y, *y, *H, *g; // device, packed per trajectory
    double *dz, *lam;
    int32_t *info;
    const int32_t *meta; // device: per knot {n1, p, n2, w, oY, oy, oH, og(=oz), ol}
    int N;
    int h_mode, ginv;
    int64_t batch;
    int64_t sY, sy, sH, sg, sl; // per-trajectory strides (elements)
    int maxw, maxrows, max_p1, max_ps, max_p2;
    int force_lane; // debug: LQRX_KKT_FORCE_LANE=1 selects the register-only kernel
    int layout;     // 0 per-trajectory packed; 1 batch fastest (compile-time shapes only)
    int dtype;      // 0 f64; 1 f32 (the big-block kernels only: Y..lam then point at floats)
    // internal (SQP): solve only the trajectories sel[0 .. *nsel) (device arrays; layout-0
    // LDS-staged kernel only — the other kernels solve the whole batch, which is also correct)
    const int32_t *sel, *nsel;
    void *ws;         // caller's device workspace (lqrx_kkt_solve_ws) or NULL: library pool
    size_t ws_bytes;
    // runtime (n̄, m, P0, PK, PN) of a trajectory-form structure solved on a padded compile-time
    // shape (lqrx_kkt_fil.hip, Shape<…, PAD>); unused otherwise
    int32_t rt[5];
    // live trajectories per 64-lane wave of the direct FIL kernel (lqrx_kkt_fil.hip kkt_fild_kernel,
    // layout 0; set by its launcher): 64, or 32 on small batches so that twice the waves run
    int32_t lpw;
};

hipError_t kkt_launch(const KktArgs &a, hipStream_t s);
// which generic (runtime-shaped, fp64) kernel kkt_launch would pick: 0 none, 1 LDS-staged
// ≤ (3,3,3,5,6), 2 lane ≤ (4,4,4,8,8), 3 lane ≤ (8,8,8,12,16) (runtime-indexed arrays in scratch)
int kkt_generic_class(const KktArgs &a);

// Stream-ordered scratch from a library-owned memory pool (one per device) whose release
// threshold keeps freed blocks mapped: a per-call hipMallocAsync/hipFreeAsync pair then
// costs no page-table work after the first call (the default pool returns memory at every
// synchronisation — measured +0.26 ms per 357 MB KKT slab).  Reentrant: blocks are
// stream-ordered, never shared between calls.  (lqrx_api.cpp)
hipError_t scratch_alloc(void **p, size_t bytes, hipStream_t s);
hipError_t scratch_free(void *p, hipStream_t s);
hipError_t scratch_trim(int device, size_t keep);   // lqrx_scratch_trim
// a launch's slab: the caller's workspace when one was passed, else a pool block
struct Scratch {
    void *p = nullptr;
    bool owned = false;
    hipError_t get(const KktArgs &a, size_t bytes, hipStream_t s)
    {
        if (a.ws) {
            if (a.ws_bytes < bytes) return hipErrorInvalidValue;
            p = a.ws;
            return hipSuccess;
        }
        owned = true;
        return scratch_alloc(&p, bytes, s);
    }
    hipError_t release(hipStream_t s) { return owned ? scratch_free(p, s) : hipSuccess; }
};
// slab bytes the generic kernels need (mirrors kkt_launch's selection; 0 = unsupported)
size_t kkt_scratch_bytes(const KktArgs &a);
// compile-time-shaped kernel for first/interior/last structures (lqrx_kkt_fil.hip); returns
// false (and launches nothing) when the structure has no instantiation
bool kkt_fil_launch(const KktArgs &a, const int32_t *n1, const int32_t *p, const int32_t *n2,
                    const int32_t *w, hipStream_t s, hipError_t *err);
// slab bytes of the FIL kernel for this structure; false when no FIL shape serves it
bool kkt_fil_scratch_bytes(const KktArgs &a, const int32_t *n1, const int32_t *p, const int32_t *n2,
                           const int32_t *w, size_t *bytes);

// large-block MFMA kernels (lqrx_kkt_big.hip): any structure with n1, p, n2 ≤ 64, padded
// rows ≤ 128, w ≤ 128, diagonal H or the SOC variant, layout 0, fp64 or fp32
bool kkt_big_supported(const KktArgs &a, const int32_t *n1, const int32_t *p, const int32_t *n2, const int32_t *w);
size_t kkt_big_scratch_bytes(const KktArgs &a, const int32_t *n1, const int32_t *p, const int32_t *n2,
                             const int32_t *w);
hipError_t kkt_big_launch(const KktArgs &a, const int32_t *n1, const int32_t *p, const int32_t *n2,
                          const int32_t *w, hipStream_t s);

// workgroup-per-trajectory KKT kernel (lqrx_kkt_wg.hip): the structures past the large-block
// kernels (any block > 64 rows or w > 128), every h_mode / ginv, layout 0, fp64 or fp32
constexpr int KW_MAX_BLOCK = 512, KW_MAX_W = 1024;
bool kkt_wg_supported(const KktArgs &a, const int32_t *n1, const int32_t *p, const int32_t *n2, const int32_t *w);
size_t kkt_wg_scratch_bytes(const KktArgs &a, const int32_t *n1, const int32_t *p, const int32_t *n2,
                            const int32_t *w);
hipError_t kkt_wg_launch(const KktArgs &a, const int32_t *n1, const int32_t *p, const int32_t *n2,
                         const int32_t *w, hipStream_t s);

// ---- batched trajectory SQP (lqrx_sqp.hip) ----
enum { SQP_DUBINS = 0, SQP_CARTPOLE = 1, SQP_DI1 = 2, SQP_DI2 = 3, SQP_DI3 = 4 };   // = LQRX_MODEL_*
struct SqpArgs {
    int model, N, stage_rows;         // stage_rows: PK of the interior-knot linear constraint
    double SA[32], Sb[4];             // A_s (PK × NX, column-major), b_s
    int64_t B;
    double dt, mu, tol_p, tol_d;
    double Q[8], R[8], Qf[8];         // diagonal weights, first NX / NU used
    double par[4];                    // model parameters (cartpole: mc, mp, l, g)
    const double *x0, *xf;            // B×NX
    double *Z;                        // B×NN, in/out
    double *lam;                      // B×P: multipliers of the last accepted Newton step
    int32_t *iters, *status;          // B
    double *Y, *y, *H, *g;            // KKT inputs, ABI layout (internal)
    double *dz, *lamn, *dzs;          // Newton step + its multipliers, SOC step
    double *phi0, *dphi;              // B
    int32_t *need_soc;                // B
    int32_t *n_active;                // 1
    int32_t *sel, *nsel;              // B, 1: the trajectories the next KKT solve needs
};
// kkt(ctx, ginv, dz, sel, nsel): one KKT solve of the trajectories sel[0 .. *nsel)
hipError_t sqp_run(const SqpArgs &A, int max_iters, hipStream_t s,
                   int (*kkt)(void *ctx, int ginv, double *dz, const int32_t *sel, const int32_t *nsel), void *ctx,
                   int *kkt_rc);
void sqp_structure(int nx, int nu, int pk, int N, std::vector<int32_t> &n1, std::vector<int32_t> &p,
                   std::vector<int32_t> &n2, std::vector<int32_t> &w);
bool sqp_model_dims(int model, int *nx, int *nu);

// ---- condensed least-squares LQR (lqrx_ls.hip) ----
struct LsArgs {
    const double *A, *B, *Q, *R, *Qf, *x0;
    double *U, *X, *Ab, *bb;
    int32_t *info;
    int n, m, N, hu_mode;
    int64_t batch;
};
size_t ls_lds_bytes(int n, int m, int N);
int ls_max_nm();          // (N−1)·m cap (the big, global-H path)
hipError_t ls_launch(const LsArgs &a, hipStream_t s);

} // namespace lqrx
