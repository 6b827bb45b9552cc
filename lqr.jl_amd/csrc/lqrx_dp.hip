// lqrx_dp.hip — batched finite-horizon LQR (Riccati backward pass + forward rollout) on
// gfx950.  Replaces, for a whole batch per launch, the reference's per-knot LAPACK/BLAS
// calls in solve!(sol, ::DPSolver, ::LQRProblem)  /root/reference/src/dynamic_programming.jl:54-72.
//
// Mapping: ONE WAVEFRONT PER TRAJECTORY (64-thread workgroup).  The wave walks the
// horizon k = N-1 … 1 sequentially (the Riccati recurrence is serial in k); parallelism is
// the batch.  All n×n / n×m products of a knot are fp64 MFMA (v_mfma_f64_16x16x4_f64) on
// register-resident C-layout tiles, each written as a "Mᵀ·Y" product (lqrx_tile.h) so that
// no operand ever moves between lanes:
//
//   reference (dynamic_programming.jl)      here (all tiles C-layout, P symmetric)
//   :38  PB  = P*B                          PB   = Pᵀ·B
//   :39  E   = R + B'PB                     E    = R + Bᵀ·PB
//   :40  PA  = P*A                          PA   = Pᵀ·A
//   :41  K   = B'PA                         G    = Bᵀ·PA
//   :29-30 potrf!/potrs!(E, K)              K    = E⁻¹G   (lane-per-column Cholesky, VALU)
//   :50  APB = A'PB                         APBᵀ = PBᵀ·A   (the transpose is what is needed)
//   :51  P_  = Q + A'PA - APB*K             P_   = Q + Aᵀ·PA + (APBᵀ)ᵀ·(−K)
//
// The time-invariant A, B, Q, R (lqr_problem.jl:1-11) stay in registers for the whole
// horizon; HBM traffic is the K stream (written per knot, re-read by the rollout) plus X, U.
// The m×m Cholesky + two triangular solves run on the VALU in a lane-per-column layout of
// the augmented matrix [E | G] (wave-uniform broadcasts via v_readlane), overlapping the
// MFMA work of the other wave resident on the same SIMD (launch bounds: 2 waves/SIMD).
#include <cstdlib>
#include "lqrx_tile.h"
#include "lqrx_internal.h"

// ---- build switches of this file (diagnostics for tools/tv_ablate.sh; the library build sets
// none of them).  Runtime switches (getenv, read in dp_launch): LQRX_DP_WG4, LQRX_DP_NS_OFF,
// LQRX_DP_BIG. ----
#ifndef LQRX_DP_TVEXTRA
#define LQRX_DP_TVEXTRA 0   // extra VAR bits for the time-varying launch (VAR_NOROLL …): timing only,
                            // the results of such a build are incomplete or wrong
#endif
#ifndef LQRX_DP_TVABL
#define LQRX_DP_TVABL 0     // re-read knot-1 inputs (bit 1: Q_k, bit 2: A_k/B_k/R_k): timing only,
                            // wrong results
#endif

namespace lqrx {

constexpr int LQRX_DP_TVAD = 1;   // time-varying rollout: knots of A_k/B_k row prefetch
constexpr int LQRX_DP_KD = 4;     // rollout: knots of K_k prefetch
constexpr int LQRX_DP_TVKD = 4;   // time-varying rollout: knots of K_k prefetch

// wave-level ordering of LDS traffic between the lanes of a one-wave workgroup (the LDS is in
// order per wave; this is the compiler fence + wave barrier, no s_barrier)
__device__ __forceinline__ void wsync_w()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// v of lane (lane ^ o): one ds_bpermute per dword with the lane address precomputed (the
// generic __shfl_xor adds a width test and a select per call)
__device__ __forceinline__ double xor_shfl(double v, int addr)
{
    const long long x = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_bpermute(addr, (int)(x & 0xffffffffll));
    const int hi = __builtin_amdgcn_ds_bpermute(addr, (int)(x >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ float xor_shfl(float v, int addr)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v)));
}

// Forward LDLᵀ sweep on the augmented matrix [E | G | I] — the factor/solve of
// chol_solve! (dynamic_programming.jl:28-31: potrf 'U' + potrs 'U'), reorganised so that
// it costs the fewest VALU instructions (fp64 VALU does not overlap fp64 MFMA on gfx950).
//
// E = L D Lᵀ (unit-lower L; D_ii are exactly potrf's squared pivots U_ii², so the
// potrf failure test "pivot ≤ 0" is unchanged).  One column of [E | G | I] per lane
// (columns lane + 64q).  Step i:  piv = E'[i][i] (v_readlane of lane i), t = x[i]/piv,
// x[p] −= E'[i][p]·t for p > i, where the unscaled pivot row E'[i][p] reaches every lane
// by v_readlane.  Afterwards
//   G columns hold Y = L⁻¹G,  I columns hold W = L⁻¹,  and rinv[i] = 1/piv_i,
// so  K = E⁻¹G = Wᵀ·(D⁻¹Y)  — finished by the caller as one TN MFMA product.
// Column images written back to LDS: aug[MP..MP+NP) ← Y, aug[MP+NP..2MP+NP) ← W,
// rinv (MP values) at aug + (2MP+NP)·CS.  Returns false if a pivot was not > 0.
template <typename T, int MP, int NP, int CS>
__device__ __forceinline__ bool aug_ldl_forward(T *aug, int lane)
{
    constexpr int NC = MP + NP + MP;
    constexpr int CPL = (NC + 63) / 64;
    T *rinv = aug + NC * CS + 64;     // 1/pivot per row (after a 64-wide row that is no longer used)
    T x[CPL][MP];
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        int c = lane + 64 * q;
        if (c < MP + NP) {
#pragma unroll
            for (int i = 0; i < MP; ++i) x[q][i] = aug[c * CS + i];
        } else {
#pragma unroll
            for (int i = 0; i < MP; ++i) x[q][i] = (c - MP - NP == i) ? (T)1 : (T)0;
        }
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        T piv = readlane(x[i / 64][i], i % 64);
        ok = ok && (piv > (T)0);
        T ri = rcp_nr(piv);
        if (lane == 0) rinv[i] = ri;
        T t[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) t[q] = x[q][i] * ri;
#pragma unroll
        for (int p = i + 1; p < MP; ++p) {
            const T e = readlane(x[p / 64][i], p % 64);
#pragma unroll
            for (int q = 0; q < CPL; ++q) x[q][p] = fma(-e, t[q], x[q][p]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        int c = lane + 64 * q;
        if (c >= MP && c < NC) {
#pragma unroll
            for (int i = 0; i < MP; ++i) aug[c * CS + i] = x[q][i];
        }
    }
    return ok;
}

// Newton–Schulz refinement of X ≈ E⁻¹ (E SPD, MT×MT tiles), warm-started from the previous
// knot's inverse.  One step: R = I − EᵀX (4·MT³ MFMAs, neg-A with C = I), then the update
// X += XᵀR done IN PLACE: mma_tn(X, X, R) has its accumulator alias its M operand, so the
// MFMA of k-slice s reads, as rows 4s… of "X", a tile that the slices before it have already
// added to — a Gauss–Seidel-like sweep X ← X + Σ_s X⁽ˢ⁾[s]ᵀR[s] (X⁽ˢ⁾: X after slices < s), not
// the out-of-place X + XᵀR.  Each slice's correction differs from the out-of-place one by
// O(‖X‖‖R‖²), so the step still contracts quadratically; every slice is a true MFMA→MFMA
// dependency on the one before it (the waits that PnShadow's chunks, below, are issued into).
// Returns true once the step just taken is converged to working precision: with
// ρ = 16·MT·max|R| ≥ ‖R‖∞ the new residual is ≤ cond(E)·ρ², so ρ ≤ tol (1e-11 in fp64:
// cond·1e-22, far below the rounding floor) accepts.  Not converged after `it` steps
// (e.g. a cold or poor start) → false, and the caller runs the exact sweep.
template <typename T> struct NsTol;
template <> struct NsTol<double> {
    static constexpr double v = 1e-11, one_step = 1e-9; static constexpr int it = 6;
};
template <> struct NsTol<float> {
    static constexpr float v = 3e-4f, one_step = 1e-5f; static constexpr int it = 6;
};

// NaN-propagating magnitude key: the high word of |v| (sign cleared) — order-preserving
// for magnitudes, and every NaN key exceeds +inf's.  (fmax() would silently DROP a NaN
// element — IEEE maxNum — and let a diverged iterate pass the convergence test.)
// key_bound(k) is the largest double with that high word: an upper bound of the magnitude.
__device__ __forceinline__ int mag_key(double v) { return __double2hiint(v) & 0x7fffffff; }
__device__ __forceinline__ double key_bound(int k, double) { return __hiloint2double(k, -1); }
__device__ __forceinline__ int mag_key(float v) { return __float_as_int(v) & 0x7fffffff; }
__device__ __forceinline__ float key_bound(int k, float) { return __int_as_float(k); }

// The acceptance tests on ρ = 16·MT·key_bound(key) as integer compares on the key itself.
// 16·MT is a power of two, so the product is exact (or overflows to +inf, above every
// tolerance, as its key is above every threshold) and  ρ ≤ tol ⇔ key_bound(key) ≤ t,
// ρ < 1 ⇔ key_bound(key) < 1/(16·MT),  with t = tol/(16·MT), an exact quotient.
//   fp32: key_bound(key) is the float whose bits are key, and non-negative floats order as
//         their bits, so  key_bound(key) ≤ t ⇔ key ≤ bits(t).
//   fp64: key_bound(key) is the LARGEST double with high word key.  With (h, l) the words of
//         t: key < h ⇒ below t;  key > h ⇒ above t;  key = h ⇒ (h, 0xffffffff) ≤ (h, l) only if
//         l = 0xffffffff.  So  key_bound(key) ≤ t ⇔ key ≤ h − (l ≠ 0xffffffff).
//   ρ < 1: 1/(16·MT) has a zero low word / mantissa, so  key_bound(key) < it ⇔ key < its key
//         (fp64: (h, 0xffffffff) is above (h, 0);  fp32: equal bits are not below).
//   NaN:  every NaN key — and the fp64 +inf key, whose bound (0x7ff00000, 0xffffffff) is a
//         NaN — is above every threshold here: not accepted, not contracting, as before.
// tests/test_ns_keys.py restates both decisions on the host and compares them key by key.
template <typename T, int MT> struct NsKey;
template <int MT> struct NsKey<double, MT> {
    static constexpr int le(double t)
    {
        const unsigned long long b = __builtin_bit_cast(unsigned long long, t);
        return (int)(b >> 32) - ((b & 0xffffffffull) != 0xffffffffull ? 1 : 0);
    }
    static constexpr int v = le(NsTol<double>::v / (16 * MT));
    static constexpr int one_step = le(NsTol<double>::one_step / (16 * MT));
    static constexpr int below_one = (int)(__builtin_bit_cast(unsigned long long, 1.0 / (16 * MT)) >> 32) - 1;
};
template <int MT> struct NsKey<float, MT> {
    static constexpr int v = __builtin_bit_cast(int, NsTol<float>::v / (16 * MT));
    static constexpr int one_step = __builtin_bit_cast(int, NsTol<float>::one_step / (16 * MT));
    static constexpr int below_one = __builtin_bit_cast(int, 1.0f / (16 * MT)) - 1;
};

// Work for the iteration's shadow: MFMAs that do not depend on the solve, handed to ns_refine
// in numbered chunks.  The iteration is one serial chain — the residual's MFMAs feed the test,
// every slice of the in-place update feeds the next, the update feeds K = XᵀG — and a one-wave
// workgroup has nothing else of its own to issue while a result is in flight.  ns_refine issues
// chunk 0 behind the first residual (before its test), chunks 1 … 4·MT behind the 4·MT k-slices
// of the first update, chunk 4·MT + 1 behind the second residual; the caller issues whatever
// the path taken did not reach (rest()).  NsNoShadow: nothing to issue.
struct NsNoShadow {
    template <int C> __device__ __forceinline__ void chunk() const {}
};
// the K-independent part of P_: Pn += AᵀPA (lower tiles), mma_tn_lower's MFMAs in its order,
// cut into NCH = 4·MT + 2 chunks (per accumulator the MFMA order is mma_tn_lower's: same bits).
// KT: the product's row tiles — NT, or VAR_PREFB's NT − MT (A₂ᵀ(P̃₂₂A₂): half the MFMAs per chunk)
template <typename T, int NT, int MT, int KT = NT> struct PnShadow {
    using acc = typename Tile<T>::acc;
    static constexpr int NCH = 4 * MT + 2, TOT = mma_tn_lower_count<T, KT, NT>();
    static constexpr int CH = (TOT + NCH - 1) / NCH;
    acc (&Pn)[NT][NT];
    const acc (&At)[KT][NT];
    const acc (&PA)[KT][NT];
    template <int C> __device__ __forceinline__ void chunk() const
    {
        // pinned: the scheduler must not move the chunk off the wait it is there to cover
        __builtin_amdgcn_sched_barrier(0);
        mma_tn_lower_range<T, KT, NT, C * CH, (C + 1) * CH>(Pn, At, PA);
        __builtin_amdgcn_sched_barrier(0);
    }
    // chunks [B, E) unpinned
    template <int B, int E> __device__ __forceinline__ void range() const
    {
        mma_tn_lower_range<T, KT, NT, B * CH, E * CH>(Pn, At, PA);
    }
    // the chunks ns_refine did not issue: `done` is 0 (not called), 1, 4·MT + 1 or NCH
    __device__ __forceinline__ void rest(int done) const
    {
        if (done < 1) range<0, 1>();
        if (done < 4 * MT + 1) range<1, 4 * MT + 1>();
        if (done < NCH) range<4 * MT + 1, NCH>();
    }
};

// VAR_DIAG's shadow: A₂ = [Σ | A₂₂] with Σ diagonal, so the product's tiles (i, j), i < MT, are row
// scalings that the knot forms itself; what is left for the chain's shadow is A₂₂ᵀ·PA, the lower tiles
// of rows MT … NT − 1 (At holds A₂₂'s tiles alone), in mma_tn_lower's order, cut into the same NCH chunks
template <typename T, int NT, int MT, int KT> struct PnShadowDiag {
    using acc = typename Tile<T>::acc;
    static constexpr int NCH = 4 * MT + 2;
    static constexpr int ROW = (NT * (NT + 1) - MT * (MT + 1)) / 2, TOT = KT * 4 * ROW;   // per k-slice, in all
    static constexpr int beg(int c) { return c * TOT / NCH; }
    acc (&Pn)[NT][NT];
    const acc (&At)[KT][NT - MT];
    const acc (&PA)[KT][NT];
    template <int B, int E> __device__ __forceinline__ void range() const
    {
        int idx = 0;
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = MT; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j, ++idx)
                        if (idx >= beg(B) && idx < beg(E))
                            Pn[i][j] = Tile<T>::mma(At[k][i - MT][r], PA[k][j][r], Pn[i][j]);
    }
    template <int C> __device__ __forceinline__ void chunk() const
    {
        __builtin_amdgcn_sched_barrier(0);
        range<C, C + 1>();
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void rest(int done) const
    {
        if (done < 1) range<0, 1>();
        if (done < 4 * MT + 1) range<1, 4 * MT + 1>();
        if (done < NCH) range<4 * MT + 1, NCH>();
    }
};

// k-slice S (k-tile S / 4, register S % 4) of mma_tn(X, X, R) and the slices after it, chunk
// 1 + S behind each
template <typename T, int MT, int S, typename F>
__device__ __forceinline__ void ns_update_shadowed(typename Tile<T>::acc (&X)[MT][MT],
                                                   const typename Tile<T>::acc (&R)[MT][MT], const F &shadow)
{
    constexpr int k = S / 4, r = S % 4;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) X[i][j] = Tile<T>::mma(X[k][i][r], R[k][j][r], X[i][j]);
    shadow.template chunk<1 + S>();
    if constexpr (S + 1 < 4 * MT) ns_update_shadowed<T, MT, S + 1>(X, R, shadow);
}

// one round; ROUND 0 / 1 / 2: first, second, later.  Returns 0 to go on, 1 accepted, 2 rejected.
template <typename T, int MT, int ROUND, typename F>
__device__ __forceinline__ int ns_round(typename Tile<T>::acc (&X)[MT][MT],
                                        const typename Tile<T>::acc (&E)[MT][MT],
                                        const typename Tile<T>::acc (&Id)[MT][MT], const F &shadow, int &done)
{
    using acc = typename Tile<T>::acc;
    acc R[MT][MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) R[i][j] = Id[i][j];
    mma_tn<T, MT, MT, MT, true>(R, E, X);                       // R = I − EᵀX
    if constexpr (ROUND == 0) {
        shadow.template chunk<0>();
        done = 1;
    }
    if constexpr (ROUND == 1) {
        shadow.template chunk<4 * MT + 1>();
        done = 4 * MT + 2;
    }
    int key = 0;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) key = max(key, mag_key(R[i][j][r]));
    // uniform (SGPR) key of the residual bound ρ = 16·MT·key_bound(key) ≥ ‖R‖∞ (a NaN key
    // if any element is NaN); the tests on ρ are integer compares on the key (NsKey)
    key = wave_max_uniform_i(key);
    if (key <= NsKey<T, MT>::v) return 1;                       // ρ ≤ v: X already at working precision
    if (key > NsKey<T, MT>::below_one) return 2;                // !(ρ < 1), no contraction (or NaN): exact sweep
    if constexpr (ROUND == 0) {
        // X += XᵀR in place (see above), mma_tn's MFMAs in its order, a chunk behind each k-slice
        ns_update_shadowed<T, MT, 0>(X, R, shadow);
        done = 4 * MT + 1;
    } else {
        mma_tn<T, MT, MT, MT>(X, X, R);                         // X += XᵀR, in place (see above)
    }
    if (key <= NsKey<T, MT>::one_step) return 1;                // ρ ≤ one_step: new residual ≤ cond·ρ² ≪ eps
    return 0;
}

template <typename T, int MT, typename F>
__device__ __forceinline__ bool ns_refine(typename Tile<T>::acc (&X)[MT][MT],
                                          const typename Tile<T>::acc (&E)[MT][MT],
                                          const typename Tile<T>::acc (&Id)[MT][MT], const F &shadow, int &done)
{
    static_assert(NsTol<T>::it >= 2, "two peeled rounds");
    int s = ns_round<T, MT, 0>(X, E, Id, shadow, done);
    if (s) return s == 1;
    s = ns_round<T, MT, 1>(X, E, Id, shadow, done);
    if (s) return s == 1;
    for (int it = 2; it < NsTol<T>::it; ++it) {
        s = ns_round<T, MT, 2>(X, E, Id, shadow, done);
        if (s) return s == 1;
    }
    return false;
}
template <typename T, int MT>
__device__ __forceinline__ bool ns_refine(typename Tile<T>::acc (&X)[MT][MT],
                                          const typename Tile<T>::acc (&E)[MT][MT],
                                          const typename Tile<T>::acc (&Id)[MT][MT], int lane)
{
    (void)lane;
    int done = 0;
    for (int it = 0; it < NsTol<T>::it; ++it) {
        const int s = ns_round<T, MT, 2>(X, E, Id, NsNoShadow{}, done);
        if (s) return s == 1;
    }
    return false;
}

constexpr int imax(int a, int b) { return a > b ? a : b; }
template <typename T, int NT, int MT> struct DpCfg {
    static constexpr int NP = NT * 16, MP = MT * 16;
    static constexpr int CS = MP + 2;                       // padded LDS column stride
    static constexpr int AUG = (MP + NP + MP) * CS + 64 + MP; // [E | G | I] image + row/rinv
    static constexpr int ROLL = MP * NP + NP + MP;          // K_k + x + u (rollout)
    static constexpr int SYM = NP * (NP + 2);                // symmetrize image
    static constexpr int LDS_ELEMS = (AUG > ROLL ? AUG : ROLL) > SYM ? (AUG > ROLL ? AUG : ROLL) : SYM;
    static constexpr int QCS = NP + 2;                      // LDS-resident Q image: column stride
    static constexpr int QIMG = NP * QCS;
    static constexpr int KPL = (MP * NP + 63) / 64;         // K elements per lane (rollout)
    // VAR_CANON sizes its work area by what the kernel uses: the exact sweep's image is [E | I]
    // (aug_ldl_forward<T, MP, 0, CS>: AUGC — AUG above still counts the G columns of the [E | G | I]
    // sweep that no variant runs any more, and is left as it is so that the other variants keep their
    // LDS layout and code), K̃'s transpose image MP × NP at stride CS
    static constexpr int AUGC = 2 * MP * CS + 64 + MP, KTI = NP * CS;
    static constexpr int WORK_CANON = imax(imax(AUGC, ROLL), imax(SYM, KTI));
    static constexpr int LDS_CANON = WORK_CANON + MP * CS;   // + the Sᵀ image (read once per knot), behind the work area
    static constexpr int LDS_DIAG = LDS_CANON + MP;          // VAR_DIAG: + σ (read twice per knot), behind Sᵀ
};

// Forward rollout  dynamic_programming.jl:66-70 :  u_k = −K_k x_k ; x_{k+1} = A x_k + B u_k.
// K_k is streamed back from global (written by the backward sweep of this same wave),
// DEPTH knots ahead, 64 lanes × KPL coalesced elements per knot, staged through LDS.
// Dot products are split over the wave: u_i by SU = 64/MP lanes (i = lane % MP), x'_i by
// SX = 64/NP lanes (i = lane % NP), partial sums combined with xor-shuffles.
template <typename T, int NT, int MT, int DEPTH, bool TV = false, bool LIN = false, bool AFF = false>
__device__ __forceinline__ void dp_rollout(const DpArgs &a, int64_t b, T *lds, int lane)
{
    using C = DpCfg<T, NT, MT>;
    constexpr int NP = C::NP, MP = C::MP, KPL = C::KPL;
    constexpr int SU = 64 / MP > 0 ? 64 / MP : 1, SX = 64 / NP > 0 ? 64 / NP : 1;
    constexpr int JU = NP / SU, JX = NP / SX, PX = MP / SX; // per-lane slice lengths
    static_assert(MP <= 64 && NP <= 64, "rollout assumes n, m <= 64");
    const int n = a.n, m = a.m, N = a.N;
    const size_t mn = (size_t)m * n;
    const T *__restrict__ Kg = (const T *)a.K + (size_t)b * (size_t)(N - 1) * mn;
    // time-varying (TV): knot k's A_k, B_k at knot stride sA, sB (0 for a time-invariant field)
    const int64_t sA = (TV && a.tv_AB) ? (int64_t)n * n : 0, sB = (TV && a.tv_AB) ? (int64_t)n * m : 0;
    const T *__restrict__ Ag = (const T *)a.A + (size_t)b * n * n * (TV && a.tv_AB ? N - 1 : 1);
    const T *__restrict__ Bg = (const T *)a.B + (size_t)b * n * m * (TV && a.tv_AB ? N - 1 : 1);
    T *__restrict__ Xg = (T *)a.X + (size_t)b * (size_t)N * n;
    T *__restrict__ Ug = (T *)a.U + (size_t)b * (size_t)(N - 1) * m;
    T *Ks = lds, *xs = lds + MP * NP, *us = xs + NP;

    const int iu = lane % MP, hu = lane / MP;   // u row, column part
    const int ix = lane % NP, hx = lane / NP;   // x row, column part
    // TV: A_k, B_k rows are prefetched AD knots ahead (a ring rotated by register moves)
    constexpr int AD = TV ? LQRX_DP_TVAD : 1;
    T arow[JX], brow[PX], arow_n[AD][TV ? JX : 1], brow_n[AD][TV ? PX : 1];
    auto load_rows = [&](int kk, T *ar, T *br) {   // row ix of A_kk, B_kk (this lane's part)
        const T *Ak = Ag + (int64_t)(kk - 1) * sA, *Bk = Bg + (int64_t)(kk - 1) * sB;
        // per-knot (TV) loads: lane-derived offsets are laundered and kept 32-bit, so they
        // are recomputed per call instead of hoisted out of the knot loop as 24 live
        // 64-bit addresses (which spilled the whole time-varying kernel at 2 waves/SIMD)
        int lx = ix, lh = hx;
        if constexpr (TV) asm volatile("" : "+v"(lx), "+v"(lh));
#pragma unroll
        for (int t = 0; t < JX; ++t) {
            int j = lh * JX + t;
            ar[t] = (lx < n && j < n) ? Ak[lx + j * n] : (T)0;
        }
#pragma unroll
        for (int t = 0; t < PX; ++t) {
            int p = lh * PX + t;
            br[t] = (lx < n && p < m) ? Bk[lx + p * n] : (T)0;
        }
    };
    load_rows(1, arow, brow);
    if constexpr (TV) {
#pragma unroll
        for (int d = 0; d + 1 < AD; ++d)
            if (2 + d <= N - 1) load_rows(2 + d, arow_n[d], brow_n[d]);
    }
    const T *x0 = (const T *)a.x0 + (size_t)b * n;
    if (lane < NP) xs[lane] = (lane < n) ? x0[lane] : (T)0;
    if (lane < MP) us[lane] = (T)0;
    if (lane < n) Xg[lane] = x0[lane];

    T ring[DEPTH][KPL], dring[LIN ? DEPTH : 1];   // K_k (+ the feedforward d_k, lane < m)
    const T *Dg = LIN ? (const T *)a.d + (size_t)b * (size_t)(N - 1) * m : nullptr;
    auto issue = [&](int kk, T(&dst)[KPL]) {
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            size_t e = (size_t)lane + 64 * s;
            dst[s] = (kk <= N - 1 && e < mn) ? Kg[(size_t)(kk - 1) * mn + e] : (T)0;
        }
    };
    auto issue_d = [&](int kk, T &dst) {
        if constexpr (LIN) dst = (kk <= N - 1 && lane < m) ? Dg[(size_t)(kk - 1) * m + lane] : (T)0;
    };
    // affine offset c_k (AFF): row `lane` of it, per knot with A_k, B_k (read at the top of the
    // knot, used at its end) or once
    const size_t sc = (AFF && TV && a.tv_AB) ? (size_t)n : 0;
    const T *Cg = AFF ? (const T *)a.c + (size_t)b * n * (sc ? (size_t)(N - 1) : 1) : nullptr;
    T cx = (T)0;
    if constexpr (AFF && !TV) cx = lane < n ? Cg[lane] : (T)0;
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
        issue(1 + d, ring[d]);
        issue_d(1 + d, dring[LIN ? d : 0]);
    }
    __syncthreads();

    for (int k0 = 1; k0 <= N - 1; k0 += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int k = k0 + d;
            if (k <= N - 1) {
#pragma unroll
                for (int s = 0; s < KPL; ++s) {
                    size_t e = (size_t)lane + 64 * s;
                    if (e < mn) Ks[e] = ring[d][s];
                }
                issue(k + DEPTH, ring[d]);
                T dcur = (T)0;
                if constexpr (LIN) {
                    dcur = dring[d];
                    issue_d(k + DEPTH, dring[d]);
                }
                if constexpr (TV) {
                    if (k + AD <= N - 1) load_rows(k + AD, arow_n[AD - 1], brow_n[AD - 1]);   // AD knots ahead
                }
                if constexpr (AFF && TV) cx = lane < n ? Cg[(size_t)(k - 1) * sc + lane] : (T)0;
                __syncthreads();
                // u_i = −Σ_j K[i][j] x_j   (dynamic_programming.jl:68)
                T s0 = 0, s1 = 0;
#pragma unroll
                for (int t = 0; t < JU; t += 2) {
                    int j0 = hu * JU + t, j1 = j0 + 1;
                    if (j0 < n) s0 = fma(Ks[iu + j0 * m], xs[j0], s0);
                    if (t + 1 < JU && j1 < n) s1 = fma(Ks[iu + j1 * m], xs[j1], s1);
                }
                T su = s0 + s1;
#pragma unroll
                for (int o = MP; o < 64; o <<= 1) su += xor_shfl(su, (lane ^ o) << 2);
                if (lane < m) {
                    const T u = LIN ? -(su + dcur) : -su;   // u = −K x (− d)
                    us[lane] = u;
                    Ug[(size_t)(k - 1) * m + lane] = u;
                }
                __syncthreads();
                // x_{k+1} = A x_k + B u_k   (:69)
                T t0 = 0, t1 = 0;
#pragma unroll
                for (int t = 0; t < JX; t += 2) {
                    t0 = fma(arow[t], xs[hx * JX + t], t0);
                    if (t + 1 < JX) t1 = fma(arow[t + 1], xs[hx * JX + t + 1], t1);
                }
#pragma unroll
                for (int t = 0; t < PX; ++t) t1 = fma(brow[t], us[hx * PX + t], t1);
                T xn = t0 + t1;
#pragma unroll
                for (int o = NP; o < 64; o <<= 1) xn += __shfl_xor(xn, o);
                if constexpr (AFF) xn += cx;                             // + c_k
                __syncthreads();
                if (lane < n) {
                    xs[lane] = xn;
                    Xg[(size_t)k * n + lane] = xn;
                }
                if constexpr (TV) {
#pragma unroll
                    for (int t = 0; t < JX; ++t) arow[t] = arow_n[0][t];
#pragma unroll
                    for (int t = 0; t < PX; ++t) brow[t] = brow_n[0][t];
#pragma unroll
                    for (int d = 0; d + 1 < AD; ++d) {
#pragma unroll
                        for (int t = 0; t < JX; ++t) arow_n[d][t] = arow_n[d + 1][t];
#pragma unroll
                        for (int t = 0; t < PX; ++t) brow_n[d][t] = brow_n[d + 1][t];
                    }
                }
                __syncthreads();
            }
        }
    }
}

// one global load the compiler's wait-count pass does not track (the caller waits by hand)
template <typename T, int OFF> __device__ __forceinline__ T gload_asm(const T *p);
template <> __device__ __forceinline__ double gload_asm<double, 0>(const double *p)
{
    double v;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p));
    return v;
}
template <typename T, int OFF> __device__ __forceinline__ T gload_asm(const T *p)
{
    T v;
    if constexpr (sizeof(T) == 8)
        asm volatile("global_load_dwordx2 %0, %1, off offset:%2" : "=v"(v) : "v"(p), "n"(OFF));
    else
        asm volatile("global_load_dword %0, %1, off offset:%2" : "=v"(v) : "v"(p), "n"(OFF));
    return v;
}
template <> __device__ __forceinline__ float gload_asm<float, 0>(const float *p)
{
    float v;
    asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(p));
    return v;
}
// dst[c] = p[c·STR bytes] for c < C (compile-time immediate offsets)
template <typename T, int C, int STR>
__device__ __forceinline__ void gload_run(T *dst, const T *p)
{
    if constexpr (C > 0) {
        gload_run<T, C - 1, STR>(dst, p);
        dst[C - 1] = gload_asm<T, (C - 1) * STR>(p);
    }
}
// s_waitcnt vmcnt(N) that the values r (and d) depend on: their consumers stay after it
template <int N, typename T, int C>
__device__ __forceinline__ void vm_wait_regs(T (&r)[C], T &d)
{
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(d) : "n"(N) : "memory");
#pragma unroll
    for (int c = 0; c < C; ++c) asm volatile("" : "+v"(r[c]));
}

// The same rollout for exact tile grids (n = 16·NT ∈ {16, 32, 64}, m = 16·MT; time-invariant A,
// B), restructured so that nothing but its arithmetic is left per knot: K_k goes from HBM
// straight into registers DEPTH knots ahead (no LDS staging, no exec-mask branches), in a lane
// map where lane l owns row iu = l mod MP of K_k and a contiguous run of CU columns, so
// u_i = −Σ K[i][j] x_j is one FMA chain per lane plus xor-shuffles over the SU = 64/MP lanes of
// the row; x_{k+1} = A x + B u with A, B rows in registers (lane l: row l mod NP, a
// contiguous column run); x and u pass between lanes through LDS, read as contiguous runs;
// the wave is its own workgroup, so wave-level ordering (wsync) replaces barriers.
template <typename T, int NT, int MT, int DEPTH, bool LIN, bool AFF = false>
__device__ __forceinline__ void dp_rollout_full(const DpArgs &a, int64_t b, T *lds, int lane)
{
    constexpr int NP = 16 * NT, MP = 16 * MT;
    constexpr int SU = 64 / MP, CU = NP / SU;          // lanes per K row, K columns per lane
    constexpr int SX = 64 / NP, CX = NP / SX, CB = MP / SX;   // lanes per x row; A, B columns per lane
    static_assert(64 % NP == 0 && 64 % MP == 0, "exact tile grids with 64 % n == 0");
    const int N = a.N;
    constexpr size_t mn = (size_t)MP * NP;
    const T *__restrict__ Kg = (const T *)a.K + (size_t)b * (size_t)(N - 1) * mn;
    const T *__restrict__ Ag = (const T *)a.A + (size_t)b * NP * NP;
    const T *__restrict__ Bg = (const T *)a.B + (size_t)b * NP * MP;
    T *__restrict__ Xg = (T *)a.X + (size_t)b * (size_t)N * NP;
    T *__restrict__ Ug = (T *)a.U + (size_t)b * (size_t)(N - 1) * MP;
    const T *Dg = LIN ? (const T *)a.d + (size_t)b * (size_t)(N - 1) * MP : nullptr;
    T *xs = lds, *us = lds + NP;
    const int iu = lane % MP, hu = lane / MP, ix = lane % NP, hx = lane / NP;
    T arow[CX], brow[CB];
#pragma unroll
    for (int c = 0; c < CX; ++c) arow[c] = Ag[ix + (size_t)(hx * CX + c) * NP];
#pragma unroll
    for (int c = 0; c < CB; ++c) brow[c] = Bg[ix + (size_t)(hx * CB + c) * NP];
    const T *x0 = (const T *)a.x0 + (size_t)b * NP;
    if (lane < NP) {
        const T v = x0[lane];
        xs[lane] = v;
        Xg[lane] = v;
    }
    T cx = (T)0;                                       // affine offset c (AFF): row ix
    if constexpr (AFF) cx = ((const T *)a.c)[(size_t)b * NP + ix];
    // K_kk (knot kk = 1 … N−1; past the end: the last knot again, never used).  The loads are
    // inline asm, invisible to the compiler's wait-count pass, which would otherwise wait at
    // the loop header for the loads issued one knot earlier instead of DEPTH knots earlier;
    // the wait is placed by hand: per knot the wave issues KOPS memory ops (CU loads of K
    // (+1 of d), then the U and X stores), so knot k's slot is complete once at most
    // KOPS·(DEPTH−1) are outstanding (fewer in the first DEPTH knots: the bound below is the
    // smallest such count, i.e. a slight over-wait in the steady state)
    // (A K slot too large for the 6-bit vmcnt — n = 64, m = 32 — takes compiler-tracked loads.)
    // Not with linear terms: there the compiler copied an in-flight d register (the asm load's
    // destination, which it sees as already written) into another register before the hand
    // wait, so u_k now and then used the load's address bits (an intermittent wrong X/U in
    // tests/test_dp_linear_gpu.py::test_dp_linear_device_stream; the copy is visible in the
    // gfx950 assembly of dp_riccati_kernel<double,2,1,2,64,true>).  The LIN variants take
    // compiler-tracked loads, whose waits the compiler places itself.
    constexpr int VMW = (CU + (LIN ? 1 : 0)) * (DEPTH - 1);
    constexpr bool HAND = !LIN && VMW <= 63 && CU * MP * (int)sizeof(T) <= 4096;
    T ring[DEPTH][CU], dring[DEPTH];
    auto issue = [&](int kk, T (&dst)[CU], T &dd) __attribute__((always_inline)) {
        const T *Kk = Kg + (size_t)(min(kk, N - 1) - 1) * mn + iu + (size_t)hu * CU * MP;
        const T *Dk = LIN ? Dg + (size_t)(min(kk, N - 1) - 1) * MP + iu : nullptr;
        if constexpr (HAND) {
            gload_run<T, CU, MP * (int)sizeof(T)>(dst, Kk);
            if constexpr (LIN) dd = gload_asm<T, 0>(Dk);
        } else {
#pragma unroll
            for (int c = 0; c < CU; ++c) dst[c] = Kk[(size_t)c * MP];
            if constexpr (LIN) dd = *Dk;
        }
    };
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
        dring[d] = (T)0;
        issue(1 + d, ring[d], dring[d]);
    }
    wsync_w();
    // one knot: slot d holds K_k (issued DEPTH knots earlier); NEXT: refill the slot with knot
    // k + DEPTH (the main loop) or not (the tail)
    auto knot = [&](int k, T (&rk)[CU], T &dk, bool next) __attribute__((always_inline)) {
        // u = −K_k x_k (− d_k)   (dynamic_programming.jl:68)
        T xu[CU];
#pragma unroll
        for (int c = 0; c < CU; ++c) xu[c] = xs[hu * CU + c];
        T s0 = (T)0, s1 = (T)0;
#pragma unroll
        for (int c = 0; c < CU; c += 2) {
            s0 = fma(rk[c], xu[c], s0);
            if (c + 1 < CU) s1 = fma(rk[c + 1], xu[c + 1], s1);
        }
        T su = s0 + s1;
#pragma unroll
        for (int o = MP; o < 64; o <<= 1) su += __shfl_xor(su, o);
        const T u = LIN ? -(su + dk) : -su;
        T dn = (T)0;
        if (next) issue(k + DEPTH, rk, LIN ? dk : dn);
        if (hu == 0) {
            us[iu] = u;
            Ug[(size_t)(k - 1) * MP + iu] = u;
        }
        wsync_w();
        // x_{k+1} = A x_k + B u_k   (:69)
        T t0 = (T)0, t1 = (T)0;
#pragma unroll
        for (int c = 0; c < CX; c += 2) {
            t0 = fma(arow[c], xs[hx * CX + c], t0);
            if (c + 1 < CX) t1 = fma(arow[c + 1], xs[hx * CX + c + 1], t1);
        }
#pragma unroll
        for (int c = 0; c < CB; ++c) t1 = fma(brow[c], us[hx * CB + c], t1);
        T xn = t0 + t1;
#pragma unroll
        for (int o = NP; o < 64; o <<= 1) xn += xor_shfl(xn, (lane ^ o) << 2);
        if constexpr (AFF) xn += cx;                   // + c
        wsync_w();
        if (hx == 0) {
            xs[ix] = xn;
            Xg[(size_t)k * NP + ix] = xn;
        }
        wsync_w();
    };
    // Whole groups of DEPTH knots: every slot is waited for, consumed and refilled on every
    // path through the loop body, so the hand bound VMW holds on every path the compiled code
    // has (tests/isa_vmcnt.py checks it on the gfx950 assembly; a body that skipped knots past
    // N−1 had compiled paths with fewer loads between a slot's issue and its wait).
    int k0 = 1;
    for (; k0 + DEPTH - 1 <= N - 1; k0 += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            if constexpr (HAND) vm_wait_regs<VMW>(ring[d], dring[d]);
            knot(k0 + d, ring[d], dring[d], true);
        }
    }
    // the last < DEPTH knots: their K is in the ring already; drain every load first (also
    // the clamped refills past N−1, so no load is in flight when the rollout returns)
    if constexpr (HAND) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) vm_wait_regs<0>(ring[d], dring[d]);
    }
#pragma unroll
    for (int d = 0; d < DEPTH - 1; ++d)
        if (k0 + d <= N - 1) knot(k0 + d, ring[d], dring[d], false);
}

// Kernel variants (compile-time VAR bits):
//   (0)        : the symmetric fast form: APBᵀ = PBᵀA equals G = BᵀPA for symmetric P,
//                so P_ = Q + AᵀPA − GᵀK; P_ is symmetric, so only its lower tiles are
//                computed and the upper ones mirrored (LDS transpose); Q lives in an LDS
//                image and is read into the P_ accumulators each knot.  (The reference op
//                order — explicit APB, all n×n tiles — was a round-1 A/B variant; it was
//                never selectable through the ABI and is gone: parity is checked against
//                the oracle, which keeps the reference order.)
//   VAR_NOSOLVE / VAR_NOROLL / VAR_NOKSTORE : diagnostic ablations (tools/dp_ablate).
//   VAR_TV     : time-varying A_k, B_k, Q_k, R_k (ABI knot strides 1):
//                knot k-1's A, B, R are loaded into the same registers right after knot k's
//                last product that reads them (the load hides behind the rest of the knot);
//                Q_k is loaded from global straight into the P_ accumulators.
//   VAR_LIN    : linear cost terms (lqrx_dp_solve_linear), alone (time-invariant problem) or
//                with VAR_TV: K = XᵀG's companion d = Xᵀ(r + Bᵀp) and p ← q + Aᵀp − Gᵀd
//                (Gᵀ = APB for symmetric P) on the VALU — the vectors are exchanged through
//                a small LDS image (lin_* helpers below).
//   VAR_AFF    : affine dynamics x⁺ = Ax + Bu + c (lqrx_dp_solve_affine), only with VAR_LIN, with
//                or without VAR_TV: the recursion is VAR_LIN's with p̃ = p + P c_k in place of p in
//                its two uses (w = r + Bᵀp̃, Aᵀp̃).  P c_k = Pᵀc_k (P is exactly symmetric after
//                tiles_symmetrize_lower) is one more lin_tn-style sum over the P tiles, added
//                into the p image before lin_first() reads it (aff_ptilde() in the kernel: at the
//                head of lin_first() time-varying, behind the PA product time-invariant); the
//                rollout adds c_k to x_{k+1}.
//   VAR_CROSS  : cost cross term uᵀM_k x (lqrx_dp_solve_cross), only with VAR_LIN | VAR_AFF, with
//                or without VAR_TV: G = BᵀPA + M_k, so the G accumulators start from M_k instead
//                of zero and every later reader of G (K = XᵀG, Gᵀd, −GᵀK) follows; E, info and
//                the Newton–Schulz chain do not see M.  M_k (m×n, knot stride with Q, R) is read
//                from global memory every knot — per knot from HBM when time-varying, the
//                cache-resident m·n block of the trajectory otherwise (no LDS image: LDS decides
//                the workgroups per CU on the fp64 2×1 grid and above) — issued
//                behind the PB / PA products, beside Q, so that it lands under the E product.
//   VAR_VALUE  : the value function's constant (lqrx_dp_solve_value), only with VAR_LIN | VAR_AFF |
//                VAR_CROSS, with or without VAR_TV: s_k = s_{k+1} + c_kᵀ(p + ½Pc_k) − ½h_kᵀd_k and
//                dV = Σ h_kᵀd_k.  Two per-lane accumulators on lanes 0–15, the lanes that hold p, Pc,
//                w and d in column layout: sc += c_i(p_i + ½(Pc)_i) in aff_ptilde(), hd += w_j d_j
//                where d is formed.  They live in 2·16 LDS slots behind the c image, each touched
//                by its own lane only (no barrier): as loop-carried registers they spilled 4 VGPRs
//                (20 B/lane) on the fp64 2×1 grid at 2 waves/SIMD, which has none to spare
//                (DESIGN §3.7).  No cross-lane work in the
//                knot loop unless every s_k is asked for (a.p_all, uniform over the grid); one
//                16-lane reduction of the running sums either way, so s_1 is the same bits in
//                both modes.
//   VAR_CANON  : input-canonical coordinates (plain kind, time-invariant, exact tile grid, m ≤ n, P_1
//                only).  The tiles hold Ã = TᵀAT, R̃ = SᵀRS, Q̃, Q̃f from the set-up's
//                workspace (lqrx_dp_canon.hip; T from the QR of B, S = B₁⁻¹), where B̃ = [I; 0]: no B
//                and PB tiles, E = R̃ + P̃[0:m, 0:m] (one tile add), G = the first m rows of P̃Ã (PA's
//                own tiles).  The ABI's gain is K = S·K̃·Tᵀ: K̃ᵀ by an LDS transpose, then two TN
//                products; −GᵀK keeps K̃.  P_1 = T·P̃_1·Tᵀ after the loop.  The rollout is the generic
//                one on A, B and the stored K.  A trajectory whose workspace flag is 0 returns at once.
//                (Flag 1 is its own; 2 is VAR_PREFB's, 0 VAR_MASK's.)
//   VAR_MASK   : the generic kernel behind a VAR_CANON launch: a trajectory whose flag is not 0 returns
//                at once, the others are solved as by the kernel without the bit.
//   VAR_PREFB  : on top of VAR_CANON, for the trajectories the set-up flags 2 (κ∞(B₁) under
//                DP_PREFB_KAPPA_F64): the deadbeat pre-feedback ũ = v − A₁x̃ (A₁, A₂ the first
//                m and the other rows of Ã) leaves the dynamics [0; A₂] and the cost Q′ = Q̃ + A₁ᵀR̃A₁,
//                M′ = −R̃A₁, R̃, with the same P̃_k and Ẽ.  Only A₂'s tiles are held; the one product
//                [P̃₁₂; P̃₂₂]·A₂ gives G = M′ + P̃₁₂A₂ (M′, in the registers A₁ had, is the accumulators'
//                start) and P̃₂₂A₂; Q′ + A₂ᵀ(P̃₂₂A₂) is PnShadow's shorter product; the ABI's gain is
//                K = S·K_v·Tᵀ + C, C = S·A₁·Tᵀ of the workspace the accumulators' start, loaded every
//                knot (cache-resident) behind −GᵀK_v.  80 MFMAs per knot where VAR_CANON has 108.
//   VAR_DIAG   : on top of VAR_CANON | VAR_PREFB, n = 2m, for the trajectories the set-up flags 3: it has
//                rotated the basis by the SVD of A₂'s left block, x̃ → diag(U₁, U₂)ᵀx̃, ũ → U₁ᵀũ (B̃ stays
//                [I; 0]; T·diag(U₁, U₂), S·U₁ stand where T, S stood), so that A₂ = [Σ | A₂₂] with Σ
//                diagonal.  Only A₂₂'s tiles are held, σ lives in LDS; column tile 0 of [P̃₁₂; P̃₂₂]·A₂ is
//                a column scaling of P̃'s tiles (M′ the addend for G), tile (0, 0) of A₂ᵀ(P̃₂₂A₂) a row
//                scaling of PA's: 12 v_fma_f64 where VAR_PREFB has 12 MFMAs.  68 MFMAs per knot.
enum : int { VAR_NOSOLVE = 2, VAR_NOROLL = 4, VAR_NOKSTORE = 8, VAR_SWEEPONLY = 16, VAR_TV = 32,
             VAR_LIN = 64, VAR_AFF = 128, VAR_CROSS = 256, VAR_VALUE = 512, VAR_CANON = 1024, VAR_MASK = 2048,
             VAR_PREFB = 4096, VAR_DIAG = 8192 };

// Vector products with register tiles (VAR_LIN).  A vector v is read from its LDS image in
// "row layout" (lane l, slot [i][r] = v[16i + Tile::row(l, r)], the rows a C-layout tile's
// lane holds); Mᵀv is then a per-lane FMA chain over those rows, summed over the four row
// groups (lanes l, l^16, l^32, l^48), and lands in "column layout": lane l holds
// (Mᵀv)[16j + (l & 15)] for output tile j.
template <typename T, int RT>
__device__ __forceinline__ void lin_rows(T (&v)[RT][4], const T *img, int lane)
{
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[i][r] = img[16 * i + Tile<T>::row(lane, r)];
}
template <typename T, int RT, int CT>
__device__ __forceinline__ void lin_tn(T (&y)[CT], const typename Tile<T>::acc (&M)[RT][CT], const T (&v)[RT][4])
{
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) y[j] = fma(M[i][j][r], v[i][r], y[j]);
}
template <typename T>
__device__ __forceinline__ T lin_rowsum(T x)
{
    x += __shfl_xor(x, 16);
    return x + __shfl_xor(x, 32);
}

// sum over lanes 0–15 of a 16-lane group (VAR_VALUE: the column-layout partials)
template <typename T>
__device__ __forceinline__ T lin_colsum(T x)
{
    x += __shfl_xor(x, 8);
    x += __shfl_xor(x, 4);
    x += __shfl_xor(x, 2);
    return x + __shfl_xor(x, 1);
}

template <typename T, int NT, int MT, int WAVES, int VAR, bool FULL>
__global__ __launch_bounds__(64, WAVES) void dp_riccati_kernel(const DpArgs a)
{
    using C = DpCfg<T, NT, MT>;
    using acc = typename Tile<T>::acc;
    constexpr int MP = C::MP, CS = C::CS;
    constexpr bool TV = (VAR & VAR_TV) != 0, LIN = (VAR & VAR_LIN) != 0, AFF = (VAR & VAR_AFF) != 0;
    static_assert(!AFF || LIN, "VAR_AFF extends VAR_LIN");
    constexpr bool CROSS = (VAR & VAR_CROSS) != 0;
    constexpr bool VALUE = (VAR & VAR_VALUE) != 0;
    static_assert(!VALUE || CROSS, "VAR_VALUE extends VAR_LIN | VAR_AFF | VAR_CROSS");
    constexpr bool CANON = (VAR & VAR_CANON) != 0, MASK = (VAR & VAR_MASK) != 0;
    static_assert(!CANON || (FULL && !TV && !LIN && MT <= NT && !MASK), "VAR_CANON: plain, time-invariant, exact grid");
    static_assert(!MASK || (!TV && !LIN), "VAR_MASK: the plain time-invariant kernel");
    constexpr bool PREFB = (VAR & VAR_PREFB) != 0;
    static_assert(!PREFB || (CANON && MT < NT), "VAR_PREFB extends VAR_CANON, m < n");
    constexpr bool DIAG = (VAR & VAR_DIAG) != 0;
    static_assert(!DIAG || (PREFB && NT == 2 * MT), "VAR_DIAG extends VAR_PREFB, n = 2m");
    constexpr int AK = PREFB ? NT - MT : NT;                    // A's row tiles in registers (VAR_PREFB: A₂ alone)
    constexpr int AJ = DIAG ? NT - MT : NT;                     // and its column tiles (VAR_DIAG: A₂₂ alone)
    // Q + AᵀPA in the shadow of the Newton–Schulz chain (PnShadow): time-invariant A only
    constexpr bool SHADOW = !TV && (VAR & (VAR_NOSOLVE | VAR_SWEEPONLY)) == 0;
    constexpr int NP = C::NP;
    __shared__ T lds[DIAG ? C::LDS_DIAG : CANON ? C::LDS_CANON : C::LDS_ELEMS];
    // p (NP), then w / d (MP); time-invariant q (NP), r (MP) images after them; VAR_AFF: one more
    // NP slot, the time-invariant c image
    constexpr int CIMG = TV ? NP + MP : 2 * (NP + MP);
    // VAR_VALUE: 16 + 16 accumulator slots (sc, hd) behind it
    constexpr int VIMG = CIMG + (AFF ? NP : 0);
    __shared__ T vimg[LIN ? VIMG + (VALUE ? 32 : 0) : 1];
    // Q (time-invariant, read every knot as the P_ accumulator start) lives in LDS for the
    // horizon: an LDS read per element instead of an L2 round trip per knot
    __shared__ T qimg[TV ? 1 : C::QIMG];

    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (b >= a.batch) return;
    // VAR_CANON / VAR_MASK: the set-up's verdict on this trajectory (wave-uniform), each kernel of
    // the launch takes the trajectories of its own flag value
    if constexpr (CANON || MASK) {
        if (DpCanonWs<T, NT, MT>::flags(a.M)[b] != (DIAG ? 3 : PREFB ? 2 : CANON ? 1 : 0)) return;
    }
    const int n = a.n, m = a.m, N = a.N;
    const size_t nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
    // per-trajectory bases; time-varying fields hold N-1 knots (knot k at index k-1)
    const size_t kAB = (TV && a.tv_AB) ? (size_t)(N - 1) : 1, kQR = (TV && a.tv_QR) ? (size_t)(N - 1) : 1;
    size_t sA = kAB > 1 ? nn : 0, sB = kAB > 1 ? nm : 0, sQ = kQR > 1 ? nn : 0, sR = kQR > 1 ? mm : 0;
#if LQRX_DP_TVABL
    // ablation (tools only): bit 1 = Q_k, bit 2 = A_k/B_k/R_k re-read from knot 1 (cache-resident)
    if (LQRX_DP_TVABL & 1) sQ = 0;
    if (LQRX_DP_TVABL & 2) sA = sB = sR = 0;
#endif
    const T *Ab = (const T *)a.A + b * nn * kAB, *Bb = (const T *)a.B + b * nm * kAB;
    const T *Qb = (const T *)a.Q + b * nn * kQR, *Rb = (const T *)a.R + b * mm * kQR;
    const T *Qg = Qb;                                           // VAR_CANON: Q̃ of the workspace, below
    // cross term M_k (m×n): knot stride with Q, R
    const size_t sM = (CROSS && kQR > 1) ? nm : 0;
    const T *Mb = CROSS ? (const T *)a.M + b * nm * kQR : nullptr;

    acc At[AK][AJ], Bt[CANON ? 1 : NT][MT], Rt[MT][MT], P[NT][NT];
    acc Tt[CANON ? NT : 1][CANON ? NT : 1];                     // VAR_CANON: Tᵀ
    acc Mp[PREFB ? MT : 1][PREFB ? NT : 1];                     // VAR_PREFB: M′
    const T *Cg = nullptr;                                      // VAR_PREFB: C of the workspace
    const size_t k0 = TV ? (size_t)(N - 2) : 0;                 // first backward knot k = N-1
    if constexpr (CANON) {
        using W = DpCanonWs<T, NT, MT>;
        const T *wsb = W::block(a.M, a.batch, b);
        Qg = wsb + W::oQ;                                       // VAR_PREFB: the set-up wrote Q′ there
        if constexpr (PREFB) {
            if constexpr (DIAG) {
                // rows and columns m … of Ã alone; σ to its image (the barrier behind the Q image covers it)
                tiles_load<T, AK, AJ, true>(At, wsb + W::oA + MP + (size_t)MP * n, n - m, n - m, n, lane, false);
                if (lane < MP) lds[C::LDS_CANON + lane] = W::sigma(a.M, a.batch, b)[lane];
            } else
                tiles_load<T, AK, NT, true>(At, wsb + W::oA + MP, n - m, n, n, lane, false);   // rows m … of Ã
            tiles_load<T, MT, NT, true>(Mp, wsb + W::oMp, m, n, m, lane, false);
            Cg = wsb + W::oC;
        } else
            tiles_load<T, NT, NT, true>(At, wsb + W::oA, n, n, n, lane, false);
        tiles_load<T, MT, MT, true>(Rt, wsb + W::oR, m, m, m, lane, false);
        tiles_load<T, NT, NT, true>(P, wsb + W::oQf, n, n, n, lane, false);
        tiles_load<T, NT, NT, true>(Tt, wsb + W::oTt, n, n, n, lane, false);
        for (int e = lane; e < MP * MP; e += 64) lds[C::WORK_CANON + e % MP + (e / MP) * CS] = wsb[W::oSt + e];   // Sᵀ image
    } else {
        tiles_load<T, NT, NT, FULL>(At, Ab + k0 * sA, n, n, n, lane, false);
        tiles_load<T, NT, MT, FULL>(Bt, Bb + k0 * sB, n, m, n, lane, false);
        tiles_load<T, MT, MT, FULL>(Rt, Rb + k0 * sR, m, m, m, lane, true);
        tiles_load<T, NT, NT, FULL>(P, (const T *)a.Qf + b * nn, n, n, n, lane, false); // :58 P = Qf
    }
    if constexpr (!TV) {
        // zero-padded NP×NP image of Q (padding rows/cols 0, as tiles_load_lower)
        for (int e = lane; e < C::NP * C::NP; e += 64) {
            const int i = e % C::NP, j = e / C::NP;
            qimg[i + j * C::QCS] = (i < n && j < n) ? Qg[i + (size_t)j * n] : (T)0;
        }
        __syncthreads();
    }

    T *Pall = a.p_all ? (T *)a.P + (size_t)b * nn * N : nullptr;
    if (Pall) tiles_store<T, NT, NT>(P, Pall + (size_t)(N - 1) * nn, n, n, n, lane);
    T *Kb = (T *)a.K + (size_t)b * (size_t)(N - 1) * nm;
    int info = 0;
    // linear terms: q_k, r_k (knot stride with Q, R), outputs d_k and p (p_1 or every p_k)
    const size_t sq = (LIN && a.tv_QR) ? (size_t)n : 0, sr = (LIN && a.tv_QR) ? (size_t)m : 0;
    const T *qg = LIN ? (const T *)a.q + (size_t)b * n * kQR : nullptr;
    const T *rg = LIN ? (const T *)a.r + (size_t)b * m * kQR : nullptr;
    T *dg = LIN ? (T *)a.d + (size_t)b * (size_t)(N - 1) * m : nullptr;
    T *pallv = (LIN && a.p_all) ? (T *)a.p + (size_t)b * (size_t)N * n : nullptr;
    // affine offset c_k: knot stride with A, B
    const size_t sc = (AFF && kAB > 1) ? (size_t)n : 0;
    const T *cg = AFF ? (const T *)a.c + (size_t)b * n * kAB : nullptr;
    if constexpr (LIN) {
        const T *qf = (const T *)a.qf + (size_t)b * n;
        for (int i = lane; i < NP; i += 64) {
            const T v = i < n ? qf[i] : (T)0;        // p = qf
            vimg[i] = v;
            if (pallv && i < n) pallv[(size_t)(N - 1) * n + i] = v;
            if constexpr (!TV) vimg[NP + MP + i] = i < n ? qg[i] : (T)0;
            if constexpr (AFF && !TV) vimg[CIMG + i] = i < n ? cg[i] : (T)0;
        }
        if constexpr (!TV) {
            for (int i = lane; i < MP; i += 64) vimg[2 * NP + MP + i] = i < m ? rg[i] : (T)0;
        }
        if constexpr (VALUE) {
            if (lane < 32) vimg[VIMG + lane] = (T)0;
        }
        __syncthreads();
    }
    acc Xi[MT][MT], Xp[MT][MT], Id[MT][MT];     // E⁻¹ of the last two knots, identity tiles
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Id[i][j][r] = (i == j && Tile<T>::row(lane, r) == tcol(lane)) ? (T)1 : (T)0;
                Xi[i][j][r] = (T)0;
                Xp[i][j][r] = (T)0;
            }
    // per-trajectory values of the knot loop, formed once: the symmetrize's diagonal-tile LDS
    // indices (kept opaque so that they stay in registers and are not re-derived per knot)
    const bool ns_off = a.ns_off != 0;
    // VAR_VALUE: every s_k (p_all) at N per trajectory, s_N = 0
    if constexpr (VALUE) {
        if (a.p_all && lane == 0) ((T *)a.vs)[(size_t)b * (size_t)N + (N - 1)] = (T)0;
    }
    int didx[4];
    symmetrize_diag_index<T, NT>(didx, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(didx[r]));

    for (int k = N - 1; k >= 1; --k) { // :61
        acc PB[NT][MT], E[MT][MT], PA[AK][NT], G[MT][NT], Pn[NT][NT];   // VAR_PREFB: PA = P̃₂₂A₂, its rows m …
        // column layout; time-varying: issued ahead of the MFMAs, time-invariant: read from
        // the LDS images where they are used (no registers held across the knot)
        T qv[LIN ? NT : 1], rv[LIN ? MT : 1];
        auto lin_qr_lds = [&]() {
            if constexpr (LIN && !TV) {
#pragma unroll
                for (int j = 0; j < NT; ++j) qv[j] = vimg[NP + MP + 16 * j + tcol(lane)];
#pragma unroll
                for (int j = 0; j < MT; ++j) rv[j] = vimg[2 * NP + MP + 16 * j + tcol(lane)];
            }
        };
        if constexpr (LIN && TV) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int i = 16 * j + tcol(lane);
                qv[j] = i < n ? qg[(size_t)(k - 1) * sq + i] : (T)0;
            }
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int i = 16 * j + tcol(lane);
                rv[j] = i < m ? rg[(size_t)(k - 1) * sr + i] : (T)0;
            }
        }
        // c_k in row layout (lin_rows' slots), time-varying: from global beside q_k, r_k
        T crow[(AFF && TV) ? NT : 1][4];
        if constexpr (AFF && TV) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = 16 * i + Tile<T>::row(lane, r);
                    crow[i][r] = (FULL || e < n) ? cg[(size_t)(k - 1) * sc + e] : (T)0;
                }
        }
        // VAR_VALUE, time-varying: c_k once more in column layout (lanes 0–15), issued here with the
        // row-layout read so that it lands under the knot's products; read where aff_ptilde() uses it,
        // it was an exposed HBM round trip per knot (+5.5 ms of 43 at n = 32, m = 16, B = 16384)
        T ccol[(VALUE && TV) ? NT : 1];
        if constexpr (VALUE && TV) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int i = 16 * j + lane;
                ccol[j] = (lane < 16 && (FULL || i < n)) ? cg[(size_t)(k - 1) * sc + i] : (T)0;
            }
        }
        // VAR_AFF: p̃ = p + P c_k, in place in the p image (the image is rewritten whole at the end
        // of the knot).  Every lane's reads of p from the knot before are behind that knot's closing
        // barrier, and slot 16j + lane was last written by this lane, so one barrier — after the
        // add, before lin_first() reads the image in row layout — is all it needs.  P c = Pᵀc: one
        // row tile of c at a time (lin_tn's sum with four c values live).
        // Time-varying: at the head of lin_first(), which follows the knot's products directly.
        // Time-invariant: here, behind P's last MFMA use, not in lin_first() after the solve —
        // P is dead from here on in the VAR_LIN variant, and holding its 8·NT² registers across
        // the solve for one mat-vec spilled 36 VGPRs on the fp64 2×1 grid at 2 waves/SIMD.
        auto aff_ptilde = [&]() {
            if constexpr (AFF) {
                T pc[NT];
#pragma unroll
                for (int j = 0; j < NT; ++j) pc[j] = (T)0;
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    T cr[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if constexpr (TV) cr[r] = crow[i][r];
                        else cr[r] = vimg[CIMG + 16 * i + Tile<T>::row(lane, r)];
                    }
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) pc[j] = fma(P[i][j][r], cr[r], pc[j]);
                }
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const T s = lin_rowsum(pc[j]);
                    if constexpr (VALUE) {
                        // c_i (p_i + ½(Pc)_i) from the slot before the add; c_i in column layout:
                        // the c image, or ccol (time-varying)
                        if (lane < 16) {
                            const int i = 16 * j + lane;
                            T ci;
                            if constexpr (TV) ci = ccol[j];
                            else ci = vimg[CIMG + i];
                            const T pi = vimg[i];
                            vimg[VIMG + lane] = fma(ci, fma((T)0.5, s, pi), vimg[VIMG + lane]);
                            vimg[i] = pi + s;
                        }
                    } else {
                        if (lane < 16) vimg[16 * j + lane] += s;
                    }
                }
                __syncthreads();                       // p̃ complete before the row-layout read
            }
        };
        if constexpr (!CANON) {
            tiles_zero<T, NT, MT>(PB);
            mma_tn<T, NT, NT, MT>(PB, P, Bt);                      // :38 PB = P B
        }
        if constexpr (PREFB) {
            // [P̃₁₂; P̃₂₂]·A₂ in mma_tn's order, its first m rows onto M′: G = M′ + P̃₁₂A₂, PA = P̃₂₂A₂
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) G[i][j] = Mp[i][j];
            tiles_zero<T, AK, NT>(PA);
            if constexpr (DIAG) {
                // A₂ = [Σ | A₂₂]: column tiles 0 … are P̃'s tiles (m …, ·) with their columns scaled by σ — P̃ is
                // exactly symmetric, so (m + j, i)ᵀ is the tile (i, m + j) as it stands —, the others the
                // product with A₂₂ in the order above
                int ls = lane;                                     // laundered: the image offset is formed per knot
                asm volatile("" : "+v"(ls));
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    const T sc = lds[C::LDS_CANON + 16 * j + tcol(ls)];
#pragma unroll
                    for (int i = 0; i < NT; ++i) {
                        acc &D = i < MT ? G[i][j] : PA[i < MT ? 0 : i - MT][j];
#pragma unroll
                        for (int r = 0; r < 4; ++r) D[r] = fma(P[i][MT + j][r], sc, D[r]);
                    }
                }
#pragma unroll
                for (int kk = 0; kk < AK; ++kk)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int i = 0; i < NT; ++i)
#pragma unroll
                            for (int j = MT; j < NT; ++j) {
                                acc &D = i < MT ? G[i][j] : PA[i < MT ? 0 : i - MT][j];
                                D = Tile<T>::mma(P[MT + kk][i][r], At[kk][j - MT][r], D);
                            }
            } else {
#pragma unroll
                for (int kk = 0; kk < AK; ++kk)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int i = 0; i < NT; ++i)
#pragma unroll
                            for (int j = 0; j < NT; ++j) {
                                acc &D = i < MT ? G[i][j] : PA[i < MT ? 0 : i - MT][j];
                                D = Tile<T>::mma(P[MT + kk][i][r], At[kk][j][r], D);
                            }
            }
        } else {
            tiles_zero<T, AK, NT>(PA);
            mma_tn<T, NT, NT, NT>(PA, P, At);                      // :40 PA = P A
        }
        if constexpr (AFF && !TV) aff_ptilde();
        // VAR_CROSS: G starts from M_k (zero padded past m, n).  The loads are issued here, beside
        // Q's, and land behind the E product; issued ahead of PB / PA they held G's registers across
        // both products, which spilled 11 VGPRs on the fp64 2×1 grid at 2 waves/SIMD and cost the
        // fp32 2×1 grid a wave per SIMD.  The lane index is laundered so that the per-lane offsets
        // are re-derived every knot: a time-invariant M has loop-invariant addresses, and kept live
        // across the knot loop they cost the same two grids 2 spilled VGPRs / the wave
        if constexpr (CROSS) {
            int lm = lane;
            asm volatile("" : "+v"(lm));
            tiles_load<T, MT, NT, FULL>(G, Mb + (size_t)(k - 1) * sM, m, n, m, lm, false);
        }
        if constexpr (TV) {
            tiles_load_lower<T, NT, FULL>(Pn, Qb + (size_t)(k - 1) * sQ, n, n, lane);
        }
        else tiles_lower_from_lds<T, NT>(Pn, qimg, C::QCS, lane);       // P_ ← Q (lower tiles)
        if constexpr (CANON) {
            // B̃ = [I; 0]: E = R̃ + P̃[0:m, 0:m], G = the first m rows of P̃Ã (no instruction)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j) E[i][j] = Rt[i][j] + P[i][j];
            if constexpr (!PREFB) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) G[i][j] = PA[i][j];
            }
        } else {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j) E[i][j] = Rt[i][j];
            mma_tn<T, NT, MT, MT>(E, Bt, PB);                      // :39 E = R + B'PB
            if constexpr (!CROSS) tiles_zero<T, MT, NT>(G);
            mma_tn<T, NT, MT, NT>(G, Bt, PA);                      // :41 K = B'PA (+ M_k)
        }
        // :51 Q + A'PA (lower): independent of the solve.  Time-invariant A: issued in chunks in
        // the shadow of the Newton–Schulz chain below (PnShadow); time-varying: here, before
        // A_k leaves the tiles.
        using Shadow = std::conditional_t<DIAG, PnShadowDiag<T, NT, MT, AK>, PnShadow<T, NT, MT, AK>>;
        const Shadow pn_shadow{Pn, At, PA};                         // VAR_PREFB: Q′ + A₂ᵀ(P̃₂₂A₂)
        int pn_done = 0;
        if constexpr (!SHADOW) mma_tn_lower<T, AK, NT>(Pn, At, PA);
        // linear terms, first half (time-varying: before A_k, B_k leave the tiles; time-
        // invariant: after the solve, where fewer registers are live): w = r + Bᵀp, Aᵀp partials
        T w[LIN ? MT : 1], ap[LIN ? NT : 1];
        auto lin_first = [&]() {
            if constexpr (LIN) {
                if constexpr (AFF && TV) aff_ptilde();
                T prow[NT][4];
                lin_rows<T, NT>(prow, vimg, lane);
#pragma unroll
                for (int j = 0; j < MT; ++j) w[j] = (T)0;
#pragma unroll
                for (int j = 0; j < NT; ++j) ap[j] = (T)0;
                lin_tn<T, NT, MT>(w, Bt, prow);
                lin_tn<T, NT, NT>(ap, At, prow);
#pragma unroll
                for (int j = 0; j < MT; ++j) w[j] = rv[j] + lin_rowsum(w[j]);
            }
        };
        if constexpr (LIN && TV) lin_first();
        if constexpr (TV) {
            // knot k's A, B, R are consumed: bring in knot k-1's (lands during the solve)
            if (k > 1) {
                tiles_load<T, NT, NT, FULL>(At, Ab + (size_t)(k - 2) * sA, n, n, n, lane, false);
                tiles_load<T, NT, MT, FULL>(Bt, Bb + (size_t)(k - 2) * sB, n, m, n, lane, false);
                tiles_load<T, MT, MT, FULL>(Rt, Rb + (size_t)(k - 2) * sR, m, m, m, lane, true);
            }
        }

        // :42 chol_solve!(E, K) — potrf 'U' + potrs 'U', as K = E⁻¹G with X ≈ E⁻¹:
        //  * warm start: Newton–Schulz from the previous knot's inverse, all MFMA
        //      R = I − EᵀX (neg-A modifier, C = I),  X ← X + XᵀR   (quadratic; no symmetry
        //      needed: X⁺ − E⁻¹ = −ΔᵀEΔ), accepted at working precision (see NsTol)
        //  * the first knot, and any knot whose iteration does not converge, run the exact
        //    LDLᵀ sweep of [E | I] (potrf's pivot test → info) and X = Wᵀ D⁻¹ W.
        acc Kt[MT][NT];
        if constexpr ((VAR & VAR_NOSOLVE) != 0) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) Kt[i][j] = G[i][j] * (T)1e-3 + E[0][0] * (T)1e-9;
        } else {
            bool have = false;
            if constexpr ((VAR & VAR_SWEEPONLY) == 0) {
                if (k < N - 1) {
                    // warm start: linear extrapolation 2X_{k+1} − X_{k+2} once both exist
                    acc X0[MT][MT];
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < MT; ++j) {
                            X0[i][j] = Xi[i][j];
                            Xi[i][j] = (T)2 * Xi[i][j] - Xp[i][j];   // = X_{k+1} at k = N−2 (Xp = Xi there)
                        }
                    if constexpr (SHADOW) have = !ns_off && ns_refine<T, MT>(Xi, E, Id, pn_shadow, pn_done);
                    else have = !ns_off && ns_refine<T, MT>(Xi, E, Id, lane);
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < MT; ++j) Xp[i][j] = X0[i][j];
                }
            }
            // what the path taken left of Q + A'PA (all of it ahead of an exact sweep that ran
            // no iteration)
            if constexpr (SHADOW) pn_shadow.rest(pn_done);
            if (!have) {
                tiles_to_lds<T, MT, MT>(E, lds, CS, lane);
                __syncthreads();
                bool ok = aug_ldl_forward<T, MP, 0, CS>(lds, lane);
                if (!ok && info == 0) info = k;
                __syncthreads();
                acc Wt[MT][MT], DW[MT][MT];
                tiles_from_lds<T, MT, MT>(Wt, lds + MP * CS, CS, lane);
                const T *rinv = lds + (2 * MP) * CS + 64;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        T sc = rinv[i * 16 + Tile<T>::row(lane, r)];         // D⁻¹ row scale
#pragma unroll
                        for (int j = 0; j < MT; ++j) DW[i][j][r] = Wt[i][j][r] * sc;
                    }
                __syncthreads();
                tiles_zero<T, MT, MT>(Xi);
                mma_tn<T, MT, MT, MT>(Xi, Wt, DW);                      // X = Wᵀ D⁻¹ W = E⁻¹
                if (k == N - 1) {
                    // no extrapolation into knot N−2 (only one inverse exists): 2X − Xp = X
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < MT; ++j) Xp[i][j] = Xi[i][j];
                }
            }
            tiles_zero<T, MT, NT>(Kt);
            mma_tn<T, MT, MT, NT>(Kt, Xi, G);                          // K = XᵀG = E⁻¹G
            if constexpr (DIAG) {
                // tiles (i, j), i < m/16, of A₂ᵀ(P̃₂₂A₂): PA's tiles with their rows scaled by σ, here, behind
                // the solve (ahead of the exact sweep σ's registers were live across it: 4 VGPRs spilled); the
                // other tiles are the Newton–Schulz chain's shadow (PnShadowDiag)
                int ls = lane;                                         // laundered: the image offsets are formed per knot
                asm volatile("" : "+v"(ls));
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const T sr = lds[C::LDS_CANON + 16 * i + Tile<T>::row(ls, r)];
#pragma unroll
                        for (int j = 0; j <= i; ++j) Pn[i][j][r] = fma(sr, PA[i][j][r], Pn[i][j][r]);
                    }
            }
            // VAR_CANON: K̃ to its LDS image here; the ABI's gain is formed from it behind −GᵀK, below
            if constexpr (CANON) tiles_to_lds<T, MT, NT>(Kt, lds, CS, lane);
            else if constexpr ((VAR & VAR_NOKSTORE) == 0)
                tiles_store<T, MT, NT, FULL>(Kt, Kb + (size_t)(k - 1) * nm, m, n, m, lane);
            if constexpr (LIN) {
                if constexpr (!TV) {
                    lin_qr_lds();
                    lin_first();
                }
                // second half: d = Xᵀw (the companion of K = XᵀG) ;  p ← q + Aᵀp − Gᵀd
                T dv[MT], gd[NT];
#pragma unroll
                for (int j = 0; j < MT; ++j) dv[j] = (T)0;
#pragma unroll
                for (int j = 0; j < NT; ++j) gd[j] = (T)0;
#pragma unroll
                for (int j = 0; j < MT; ++j)
                    if (lane < 16) vimg[NP + 16 * j + lane] = w[j];
                __syncthreads();
                T wrow[MT][4];
                lin_rows<T, MT>(wrow, vimg + NP, lane);
                lin_tn<T, MT, MT>(dv, Xi, wrow);
                __syncthreads();                       // w read by every lane before d lands
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    dv[j] = lin_rowsum(dv[j]);
                    const int i = 16 * j + lane;
                    if (lane < 16) {
                        // h_kᵀd_k partial: w_i from its slot (behind the barrier above), before d
                        // lands there — not from w[j], which would stay live across Xᵀw
                        if constexpr (VALUE)
                            vimg[VIMG + 16 + lane] = fma(vimg[NP + i], dv[j], vimg[VIMG + 16 + lane]);
                        vimg[NP + i] = dv[j];
                        if (i < m) dg[(size_t)(k - 1) * m + i] = dv[j];
                    }
                }
                __syncthreads();
                T drow[MT][4];
                lin_rows<T, MT>(drow, vimg + NP, lane);
                lin_tn<T, MT, NT>(gd, G, drow);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const T pn = qv[j] + lin_rowsum(ap[j]) - lin_rowsum(gd[j]);
                    const int i = 16 * j + lane;
                    if (lane < 16) {
                        vimg[i] = pn;
                        if (pallv && i < n) pallv[(size_t)(k - 1) * n + i] = pn;
                    }
                }
                __syncthreads();
            }
        }
        // VAR_PREFB: C into the ABI gain's accumulators, issued here so that the (cache-resident) load
        // lands under −GᵀK_v and K_vTᵀ.  The workspace holds C as the lanes hold its tiles (tile, lane,
        // register), 32 B per lane and tile; the lane index is laundered so that the offset is formed
        // per knot and not held across the loop.
        acc Ko[CANON ? MT : 1][CANON ? NT : 1];
        if constexpr (PREFB) {
            int lc = lane;
            asm volatile("" : "+v"(lc));
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) Ko[i][j] = *(const acc *)(Cg + ((size_t)((i * NT + j) * 64 + lc)) * 4);
        }
        mma_tn_lower<T, MT, NT, true>(Pn, G, Kt);                  // :50-51 − GᵀK (= APB K)
        if constexpr (CANON) {
            // the ABI's gain K = S·K̃·Tᵀ, here where G and K̃ are dead: K̃ᵀ read back from the image (a TN
            // product contracts rows), K̃Tᵀ = (K̃ᵀ)ᵀTᵀ, then S·(K̃Tᵀ) = (Sᵀ)ᵀ(K̃Tᵀ) with Sᵀ from its image
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            acc KtT[NT][MT], KT[MT][NT], St[MT][MT];
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        KtT[i][j][r] = lds[(j * 16 + tcol(lane)) + (i * 16 + Tile<T>::row(lane, r)) * CS];
            tiles_zero<T, MT, NT>(KT);
            mma_tn<T, NT, MT, NT>(KT, KtT, Tt);
            tiles_from_lds<T, MT, MT>(St, lds + C::WORK_CANON, CS, lane);
            if constexpr (!PREFB) tiles_zero<T, MT, NT>(Ko);       // VAR_PREFB: K = S·(K_vTᵀ) + C
            mma_tn<T, MT, MT, NT>(Ko, St, KT);
            tiles_store<T, MT, NT, FULL>(Ko, Kb + (size_t)(k - 1) * nm, m, n, m, lane);
            __syncthreads();                                       // the image is read: the symmetrize may write
        }
        tiles_symmetrize_lower<T, NT>(Pn, lds, didx, lane);        // P_ exactly symmetric
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) P[i][j] = Pn[i][j];
        if (Pall) tiles_store<T, NT, NT>(P, Pall + (size_t)(k - 1) * nn, n, n, n, lane);
        if constexpr (VALUE) {
            // every s_k: the running sums reduced, not the increments (a.p_all is a kernel argument:
            // the branch is uniform over the grid).  Each lane reads its own two slots, so no
            // barrier; here, behind the knot's last product, G and K are dead — between d and
            // −GᵀK the branch spilled 2 VGPRs on the fp64 2×1 grid at 2 waves/SIMD
            if (a.p_all) {
                const T vsc = lane < 16 ? vimg[VIMG + lane] : (T)0;
                const T vhd = lane < 16 ? vimg[VIMG + 16 + lane] : (T)0;
                const T sk = lin_colsum(vsc) - (T)0.5 * lin_colsum(vhd);
                if (lane == 0) ((T *)a.vs)[(size_t)b * (size_t)N + (k - 1)] = sk;
            }
        }
    }
    if constexpr (CANON) {
        // VAR_CANON's own tail (the statements below are every other variant's, as they were).  Its lane
        // index is laundered, so that the lane-derived offsets of the stores and the rollout are formed
        // here and not ahead of the knot loop, where they were live across it and spilled 17 VGPRs.
        int le = lane;
        asm volatile("" : "+v"(le));
        // P_1 = T·P̃_1·Tᵀ = (Tᵀ)ᵀ(P̃_1ᵀTᵀ), exactly symmetric as every P_ of the loop is
        acc PT[NT][NT];
        tiles_zero<T, NT, NT>(PT);
        mma_tn<T, NT, NT, NT>(PT, P, Tt);
        tiles_zero<T, NT, NT>(P);
        mma_tn<T, NT, NT, NT>(P, Tt, PT);
        tiles_symmetrize_lower<T, NT>(P, lds, le);
        tiles_store<T, NT, NT>(P, (T *)a.P + (size_t)b * nn, n, n, n, le);
        if (a.info && le == 0) a.info[b] = info;
        // make this wave's K stores visible to its own (other-lane) rollout loads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        dp_rollout_full<T, NT, MT, LQRX_DP_KD, false, false>(a, b, lds, le);
        return;
    }
    if (!a.p_all) tiles_store<T, NT, NT>(P, (T *)a.P + (size_t)b * nn, n, n, n, lane);
    if (a.info && lane == 0) a.info[b] = info;
    if constexpr (LIN) {
        if (!a.p_all && lane < n) ((T *)a.p)[(size_t)b * n + lane] = vimg[lane];   // p_1
    }
    if constexpr (VALUE) {
        const T vsc = lane < 16 ? vimg[VIMG + lane] : (T)0;
        const T vhd = lane < 16 ? vimg[VIMG + 16 + lane] : (T)0;
        const T rsc = lin_colsum(vsc), rhd = lin_colsum(vhd);
        if (lane == 0) {
            if (!a.p_all) ((T *)a.vs)[b] = rsc - (T)0.5 * rhd;    // s_1
            if (a.vdV) ((T *)a.vdV)[b] = rhd;
        }
    }

    if constexpr ((VAR & VAR_NOROLL) == 0) {
        // make this wave's K stores visible to its own (other-lane) rollout loads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (FULL && !TV && (64 % (16 * NT)) == 0 && (64 % (16 * MT)) == 0)
            dp_rollout_full<T, NT, MT, LQRX_DP_KD, LIN, AFF>(a, b, lds, lane);   // exact tile grids: register-streamed
        else
            dp_rollout<T, NT, MT, TV ? LQRX_DP_TVKD : LQRX_DP_KD, TV, LIN, AFF>(a, b, lds, lane);
    }
}

// ------------------------------------------------------------------ four waves per trajectory
// dp_wg4_kernel<T, MT, VAR> — fp64 n = 64, m = 16·MT: the shape whose tile grid does not fit one
// wave (A alone is 128 fp64 registers; the one-wave kernel spills ~2–3 KB per lane there).  One
// 256-thread workgroup per trajectory, one wave per SIMD, the same fast form and the same
// Newton–Schulz / exact-sweep inverse as dp_riccati_kernel, with the knot's products split by the
// n-dimension's 16-column tiles (wave w ↔ tile column w):
//   :38  PB[w][:] = P[:, w]ᵀ·B            (P tiles from the LDS image, B from its image)
//   :40  PA[:, w] = Pᵀ·A[:, w]             (all of P from LDS, A[:, w] in registers)
//   :39  E tile (w mod MT, w / MT) = R + BᵀPB   (PB from its LDS image; one tile per wave)
//   :41  G[:, w] = Bᵀ·PA[:, w]             (registers only; also to an LDS image)
//   :42  X ≈ E⁻¹ — m = 32, time-invariant: on wave 3 alone, published with its verdict through
//        the PB image while waves 0–2 form the K-independent half Q + A[:, i]ᵀPA[:, w] of their P_
//        tiles; otherwise in every wave, the four verdicts AND-ed — then K[:, w] = XᵀG[:, w] to sol.K
//   :51  P_ tiles (i, w), i from wave w's row list — the ten tiles of the symmetric 4×4 grid
//        as 3, 3, 3, 1 (inverse on wave 3) or 3, 3, 2, 2 per wave: Q + A[:, i]ᵀPA[:, w] −
//        G[:, i]ᵀK[:, w], written to the P image at (i, w) and mirrored to (w, i) (diagonal tiles
//        from their lower triangle), so the image stays exactly symmetric as
//        tiles_symmetrize_lower keeps the one-wave P.
// Four workgroup barriers per knot (after PB/PA, after E/G, the inverse's verdict (and X), after
// P_).  A lives in an LDS image (the P_ rows' A columns are read from it), A[:, w] also in
// registers; B, Q in images; R's E tile in registers.
// VAR_TV (constrained_problem.jl:3-4: per-knot A_k, B_k, Q_k, R_k): A is double-buffered in LDS
// (the time-invariant Q image's space — Q_k's P_ tiles come straight from HBM into the P_
// accumulators); knot k−1's A, B and R are requested at the top of knot k and land in LDS after
// the last reader of their buffer (A: the other buffer, after PB/PA; B: after B2; R: registers).
// VAR_LIN (lqrx_dp_solve_linear): w = r + Bᵀp (every wave, beside PB), d = Xᵀw (every wave, its
// own X), p ← q + Aᵀp − Gᵀd for rows 16w…16w+15 (A[:, w], G[:, w] are the wave's own tiles);
// p is double-buffered in LDS, w and d pass from column to row layout through per-wave slots.
// The rollout (:66-70): dp_rollout_wg4 on all four waves.  Was tried: the time-invariant rollout
// as dp_rollout_full on wave 0 alone, 234.1 vs 224.4 ms at n=64 m=32 N=512 B=8192; the
// Newton–Schulz step split over the four waves by output tile (wg4_ns_split, m = 32), 247.5 vs
// 234.1 ms — one more barrier per step and 224 B of spills.  Both forms, and the
// m = 32 time-invariant inverse in every wave instead of on wave 3, were in the tree up to bba8ceb.
template <typename T, int MT, int VAR>
struct Wg4Cfg {
    static constexpr bool TV = (VAR & VAR_TV) != 0, LIN = (VAR & VAR_LIN) != 0;
    static constexpr int NT = 4, NP = 64, MP = 16 * MT;
    // odd column strides: the compiler pairs a tile's rows into ds_read2_b64 / ds_write_b64, whose
    // 16-lane groups bank by (a/4) mod 32 — at an even stride (NP + 2) columns c and c + 8 of a tile
    // shared banks (2-way; SQ_LDS_BANK_CONFLICT ≈ a quarter of the kernel's cycles)
    static constexpr int PL = NP + 1;                    // P, Q, A, B images
    static constexpr int CS = MP + 1;                    // PB / E / G images, aug sweep
    static constexpr int P_EL = NP * PL;
    static constexpr int AUG = 2 * MP * CS + 64 + MP;   // [E | I] sweep image + row/rinv
    static constexpr int PB_EL = (MP * PL > AUG ? MP * PL : AUG);   // PB (NP × MP, stride PL) | the sweep image
    static constexpr int E_EL = MP * CS, G_EL = NP * CS;
    static constexpr int B_EL = MP * PL;                                 // B image (NP × MP)
    static constexpr int V_EL = LIN ? 2 * NP + 8 * MP : 0;               // p (×2), per-wave w, d
    static constexpr int LDS = 3 * P_EL + B_EL + PB_EL + E_EL + G_EL + V_EL + 8;   // P, Q | A₂, A, B images
    static_assert(LDS * sizeof(T) <= 160 * 1024, "dp_wg4_kernel LDS");
};
// row tile of wave w's t-th P_ tile (column tile w), −1: none
__host__ __device__ constexpr int wg4_pn_row(int w, int t)
{
    constexpr int tab[4][3] = {{0, 1, 2}, {1, 2, 3}, {2, 3, -1}, {3, 0, -1}};
    return tab[w][t];
}
// the same ten tiles when wave 3 runs the knot's Newton–Schulz inverse alone (wg4 "NS on one
// wave", m = 32): 3, 3, 3, 1 — each pair {i, j} is formed by one of its two column waves
__host__ __device__ constexpr int wg4_pn_row1(int w, int t)
{
    constexpr int tab[4][3] = {{0, 1, 3}, {1, 2, 3}, {2, 0, 3}, {3, -1, -1}};
    return tab[w][t];
}

template <typename T>
__device__ __forceinline__ typename Tile<T>::acc wg4_tload(const T *X, int ld, int lane)
{
    typename Tile<T>::acc c;
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = X[Tile<T>::row(lane, r) + tcol(lane) * ld];
    return c;
}
template <typename T>
__device__ __forceinline__ void wg4_tstore(T *X, int ld, const typename Tile<T>::acc &c, int lane)
{
#pragma unroll
    for (int r = 0; r < 4; ++r) X[Tile<T>::row(lane, r) + tcol(lane) * ld] = c[r];
}
// D += Mᵀ·Y (one 16×16×16 tile product, 4 MFMAs)
template <typename T, bool NEG = false>
__device__ __forceinline__ void wg4_mtn(typename Tile<T>::acc &D, const typename Tile<T>::acc &M,
                                        const typename Tile<T>::acc &Y)
{
#pragma unroll
    for (int r = 0; r < 4; ++r) D = NEG ? Tile<T>::mma_nega(M[r], Y[r], D) : Tile<T>::mma(M[r], Y[r], D);
}
// y += Mᵀv for one tile M (rows 16i…, this lane's column) and v in row layout (lin_rows)
template <typename T>
__device__ __forceinline__ T wg4_vtn(T y, const typename Tile<T>::acc &M, const T (&v)[4])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) y = fma(M[r], v[r], y);
    return y;
}

// Forward rollout (dynamic_programming.jl:66-70) on the four waves of dp_wg4_kernel: wave w owns
// rows 16w…16w+15 of x_{k+1} = A_k x_k + B_k u_k (lane l: row 16w + (l & 15), column quarter l >> 4
// of A's and B's columns, summed by two xor-shuffles); every wave forms the whole
// u_k = −K_k x_k (− d_k) itself (lane l: row l mod MP of K_k, a contiguous run of its columns), so
// the only workgroup barrier per knot publishes x_{k+1} (a double-buffered LDS vector).  K_k, d_k
// and — time-varying — the wave's rows of A_k, B_k are requested one knot ahead.
template <typename T, int MT, bool TV, bool LIN>
__device__ __forceinline__ void dp_rollout_wg4(const DpArgs &a, int64_t b, T *lds, int w, int lane)
{
    constexpr int NP = 64, MP = 16 * MT;
    constexpr int SU = 64 / MP, CU = NP / SU;        // lanes per K row, K columns per lane
    constexpr int CA = NP / 4, CB = MP / 4;          // A, B columns per lane
    const int N = a.N;
    constexpr size_t mn = (size_t)MP * NP;
    const bool tvab = TV && a.tv_AB;
    const int64_t sA = tvab ? (int64_t)NP * NP : 0, sB = tvab ? (int64_t)NP * MP : 0;
    const T *__restrict__ Kg = (const T *)a.K + (size_t)b * (size_t)(N - 1) * mn;
    const T *__restrict__ Ag = (const T *)a.A + (size_t)b * NP * NP * (tvab ? (size_t)(N - 1) : 1);
    const T *__restrict__ Bg = (const T *)a.B + (size_t)b * NP * MP * (tvab ? (size_t)(N - 1) : 1);
    T *__restrict__ Xg = (T *)a.X + (size_t)b * (size_t)N * NP;
    T *__restrict__ Ug = (T *)a.U + (size_t)b * (size_t)(N - 1) * MP;
    const T *Dg = LIN ? (const T *)a.d + (size_t)b * (size_t)(N - 1) * MP : nullptr;
    T *xs = lds, *us = lds + 2 * NP + w * MP;        // x_k double-buffered; this wave's u_k
    const int iu = lane % MP, hu = lane / MP;
    const int ix = 16 * w + (lane & 15), hx = lane >> 4;
    T ar[CA], br[CB], arn[TV ? CA : 1], brn[TV ? CB : 1];
    auto load_ab = [&](int kk, T *ra, T *rb) __attribute__((always_inline)) {
        const T *Ak = Ag + (int64_t)(kk - 1) * sA + ix + (size_t)hx * CA * NP;
        const T *Bk = Bg + (int64_t)(kk - 1) * sB + ix + (size_t)hx * CB * NP;
#pragma unroll
        for (int c = 0; c < CA; ++c) ra[c] = Ak[(size_t)c * NP];
#pragma unroll
        for (int c = 0; c < CB; ++c) rb[c] = Bk[(size_t)c * NP];
    };
    T kr[CU], krn[CU], dr = (T)0, drn = (T)0;
    auto load_k = [&](int kk, T *rk, T &dd) __attribute__((always_inline)) {
        const T *Kk = Kg + (size_t)(kk - 1) * mn + iu + (size_t)hu * CU * MP;
#pragma unroll
        for (int c = 0; c < CU; ++c) rk[c] = Kk[(size_t)c * MP];
        if constexpr (LIN) dd = Dg[(size_t)(kk - 1) * MP + iu];
    };
    load_ab(1, ar, br);
    load_k(1, kr, dr);
    if (N - 1 >= 2) {
        load_k(2, krn, drn);
        if constexpr (TV) load_ab(2, arn, brn);
    }
    const T *x0 = (const T *)a.x0 + (size_t)b * NP;
    if (w == 0) {
        const T v = x0[lane];
        xs[NP + lane] = v;                           // x_1 in buffer 1 (knot k reads buffer k & 1)
        Xg[lane] = v;
    }
    __syncthreads();
    for (int k = 1; k <= N - 1; ++k) {
        const T *xc = xs + (k & 1) * NP;
        // u = −K_k x_k (− d_k)   (dynamic_programming.jl:68)
        T s0 = (T)0, s1 = (T)0;
#pragma unroll
        for (int c = 0; c < CU; c += 2) {
            s0 = fma(kr[c], xc[hu * CU + c], s0);
            s1 = fma(kr[c + 1], xc[hu * CU + c + 1], s1);
        }
        T su = s0 + s1;
#pragma unroll
        for (int o = MP; o < 64; o <<= 1) su += xor_shfl(su, (lane ^ o) << 2);
        const T u = LIN ? -(su + dr) : -su;
#pragma unroll
        for (int c = 0; c < CU; ++c) kr[c] = krn[c];
        dr = drn;
        if (k + 2 <= N - 1) load_k(k + 2, krn, drn);
        if (hu == 0) {
            us[iu] = u;
            if (w == 0) Ug[(size_t)(k - 1) * MP + iu] = u;
        }
        wsync_w();
        // x_{k+1} = A_k x_k + B_k u_k   (:69), rows 16w…16w+15
        T t0 = (T)0, t1 = (T)0;
#pragma unroll
        for (int c = 0; c < CA; c += 2) {
            t0 = fma(ar[c], xc[hx * CA + c], t0);
            t1 = fma(ar[c + 1], xc[hx * CA + c + 1], t1);
        }
#pragma unroll
        for (int c = 0; c < CB; ++c) t1 = fma(br[c], us[hx * CB + c], t1);
        T xn = t0 + t1;
        xn += xor_shfl(xn, (lane ^ 16) << 2);
        xn += xor_shfl(xn, (lane ^ 32) << 2);
        if constexpr (TV) {
#pragma unroll
            for (int c = 0; c < CA; ++c) ar[c] = arn[c];
#pragma unroll
            for (int c = 0; c < CB; ++c) br[c] = brn[c];
            if (k + 2 <= N - 1) load_ab(k + 2, arn, brn);
        }
        if (lane < 16) {
            xs[((k + 1) & 1) * NP + ix] = xn;
            Xg[(size_t)k * NP + ix] = xn;
        }
        __syncthreads();
    }
}

template <typename T, int MT, int VAR>
__global__ __launch_bounds__(256, 1) void dp_wg4_kernel(const DpArgs a)
{
    using C = Wg4Cfg<T, MT, VAR>;
    using acc = typename Tile<T>::acc;
    constexpr bool TV = C::TV, LIN = C::LIN;
    constexpr int NT = C::NT, NP = C::NP, MP = C::MP, PL = C::PL, CS = C::CS;
    constexpr int BPT = NP * MP / 256;           // B elements per thread (TV staging)
    __shared__ T lds[C::LDS];
    T *Pim = lds, *Q2 = Pim + C::P_EL, *Bim = Q2 + C::P_EL, *PBim = Bim + C::B_EL, *Eim = PBim + C::PB_EL;
    T *Gim = Eim + C::E_EL, *Aim = Gim + C::G_EL, *vec = Aim + C::P_EL;
    int *flag = (int *)(vec + C::V_EL);
    T *Qim = Q2;                         // time-invariant Q; time-varying: A's second buffer
    T *aug = PBim;                       // the exact sweep reuses the PB image (read before it)
    int *vote = flag + 4;                // per-wave Newton–Schulz verdicts (flag[0]: the sweep's)
    T *pimg = vec, *wslot = vec + 2 * NP, *dslot = wslot + 4 * MP;   // VAR_LIN vectors

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x;
    if (b >= a.batch) return;            // whole workgroup
    const int N = a.N;
    constexpr size_t nn = (size_t)NP * NP, nm = (size_t)NP * MP, mm = (size_t)MP * MP;
    // per-trajectory bases; time-varying fields hold N−1 knots (knot k at index k−1)
    const size_t kAB = (TV && a.tv_AB) ? (size_t)(N - 1) : 1, kQR = (TV && a.tv_QR) ? (size_t)(N - 1) : 1;
    const size_t sA = kAB > 1 ? nn : 0, sB = kAB > 1 ? nm : 0, sQ = kQR > 1 ? nn : 0, sR = kQR > 1 ? mm : 0;
    const T *Ab = (const T *)a.A + b * nn * kAB, *Bb = (const T *)a.B + b * nm * kAB;
    const T *Qb = (const T *)a.Q + b * nn * kQR, *Rb = (const T *)a.R + b * mm * kQR;
    auto abuf = [&](int k) { return (TV && (k & 1)) ? Q2 : Aim; };   // knot k's A image
    const size_t k0 = TV ? (size_t)(N - 2) : 0;                     // first backward knot k = N − 1
    // linear terms: q_k, r_k (knot stride with Q, R), outputs d_k and p (p_1 or every p_k)
    const size_t sq = (LIN && kQR > 1) ? (size_t)NP : 0, sr = (LIN && kQR > 1) ? (size_t)MP : 0;
    const T *qg = LIN ? (const T *)a.q + (size_t)b * NP * kQR : nullptr;
    const T *rg = LIN ? (const T *)a.r + (size_t)b * MP * kQR : nullptr;
    T *dg = LIN ? (T *)a.d + (size_t)b * (size_t)(N - 1) * MP : nullptr;
    T *pallv = (LIN && a.p_all) ? (T *)a.p + (size_t)b * (size_t)N * NP : nullptr;

    acc Ar[NT], Rw = acc{0, 0, 0, 0};
    auto Bt = [&](int kk, int j) { return wg4_tload(Bim + 16 * kk + 16 * j * PL, PL, lane); };   // B[kk][j]
    const int ei = w % MT, ej = w / MT;          // this wave's E tile (w < MT²)
    if (w < MT * MT) Rw = wg4_tload(Rb + k0 * sR + 16 * ei + (size_t)16 * ej * MP, MP, lane);
    if constexpr (!TV) {
#pragma unroll
        for (int kk = 0; kk < NT; ++kk) Ar[kk] = wg4_tload(Ab + 16 * kk + (size_t)16 * w * NP, NP, lane);  // A[kk][w]
    }
    // P = Qf (:58) into the image; Q (the P_ accumulators' start) into its own; A, B of knot N−1
    {
        T *A0 = abuf(N - 1);
        for (int e = tid; e < NP * NP; e += 256) {
            Pim[(e % NP) + (e / NP) * PL] = ((const T *)a.Qf)[b * nn + e];
            if constexpr (!TV) Qim[(e % NP) + (e / NP) * PL] = Qb[e];
            A0[(e % NP) + (e / NP) * PL] = Ab[k0 * sA + e];
        }
    }
    for (int e = tid; e < NP * MP; e += 256) Bim[(e % NP) + (e / NP) * PL] = Bb[k0 * sB + e];
    if constexpr (LIN) {
        if (tid < NP) {
            const T v = ((const T *)a.qf)[(size_t)b * NP + tid];          // p = qf
            pimg[(N & 1) * NP + tid] = v;                                // p_k in buffer k & 1
            if (pallv) pallv[(size_t)(N - 1) * NP + tid] = v;
        }
    }
    T *Pall = a.p_all ? (T *)a.P + (size_t)b * nn * N : nullptr;
    T *Kb = (T *)a.K + (size_t)b * (size_t)(N - 1) * nm;
    int info = 0;
    acc Xi[MT][MT], Xp[MT][MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) Xi[i][j] = Xp[i][j] = acc{0, 0, 0, 0};
    __syncthreads();
    if (Pall)
        for (int e = tid; e < NP * NP; e += 256) Pall[(size_t)(N - 1) * nn + e] = Pim[(e % NP) + (e / NP) * PL];

    for (int k = N - 1; k >= 1; --k) {           // :61
        T *Acur = abuf(k);
        // time-varying: knot k−1's A, B (this thread's elements) and R tile, requested now
        T An[TV ? 16 : 1], Bn[TV ? BPT : 1];
        acc Rn = Rw;
        if constexpr (TV) {
#pragma unroll
            for (int kk = 0; kk < NT; ++kk) Ar[kk] = wg4_tload(Acur + 16 * kk + 16 * w * PL, PL, lane);
            if (k > 1) {
                const T *Ak = Ab + (size_t)(k - 2) * sA, *Bk = Bb + (size_t)(k - 2) * sB;
#pragma unroll
                for (int s = 0; s < 16; ++s) An[s] = Ak[tid + 256 * s];
#pragma unroll
                for (int s = 0; s < BPT; ++s) Bn[s] = Bk[tid + 256 * s];
                if (w < MT * MT) Rn = wg4_tload(Rb + (size_t)(k - 2) * sR + 16 * ei + (size_t)16 * ej * MP, MP, lane);
            }
        }
        // linear terms: w = Bᵀp_{k+1} partials (p_{k+1} read per row tile, in row layout)
        const T *pk1 = pimg + ((k + 1) & 1) * NP;
        T wv[LIN ? MT : 1];
        if constexpr (LIN) {
#pragma unroll
            for (int j = 0; j < MT; ++j) wv[j] = (T)0;
        }
        // :38, :40 — one pass over the P image: PA[:, w] and PB[w][:]
        acc PA[NT], PB[MT];
#pragma unroll
        for (int i = 0; i < NT; ++i) PA[i] = acc{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < MT; ++j) PB[j] = acc{0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < NT; ++kk) {
            acc Pt[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) Pt[i] = wg4_tload(Pim + 16 * kk + 16 * i * PL, PL, lane);   // P[kk][i]
#pragma unroll
            for (int i = 0; i < NT; ++i) wg4_mtn<T>(PA[i], Pt[i], Ar[kk]);
            const acc Pw = wg4_tload(Pim + 16 * kk + 16 * w * PL, PL, lane);                     // P[kk][w]
            T prow[4];
            if constexpr (LIN) {
#pragma unroll
                for (int r = 0; r < 4; ++r) prow[r] = pk1[16 * kk + Tile<T>::row(lane, r)];
            }
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const acc Bkj = Bt(kk, j);
                wg4_mtn<T>(PB[j], Pw, Bkj);
                if constexpr (LIN) wv[j] = wg4_vtn<T>(wv[j], Bkj, prow);                          // Bᵀp
            }
        }
#pragma unroll
        for (int j = 0; j < MT; ++j) wg4_tstore(PBim + 16 * w + 16 * j * PL, PL, PB[j], lane);
        if constexpr (TV) {
            if (k > 1) {                                   // knot k−1's A into the other buffer
                T *An_img = abuf(k - 1);
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int e = tid + 256 * s;
                    An_img[(e % NP) + (e / NP) * PL] = An[s];
                }
            }
        }
        __syncthreads();                                   // B1: PB image complete, P image read
        // :39 E tile, :41 G[:, w]
        if (w < MT * MT) {
            acc Et = Rw;
#pragma unroll
            for (int kk = 0; kk < NT; ++kk) {
                const acc Y = wg4_tload(PBim + 16 * kk + 16 * ej * PL, PL, lane);               // PB[kk][ej]
                wg4_mtn<T>(Et, Bt(kk, ei), Y);
            }
            wg4_tstore(Eim + 16 * ei + 16 * ej * CS, CS, Et, lane);
        }
        acc G[MT];
#pragma unroll
        for (int c = 0; c < MT; ++c) {
            G[c] = acc{0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < NT; ++kk) wg4_mtn<T>(G[c], Bt(kk, c), PA[kk]);
            wg4_tstore(Gim + 16 * c + 16 * w * CS, CS, G[c], lane);
        }
        __syncthreads();                                   // B2: E and G images complete, B read
        acc Qt[TV ? 3 : 1];
        if constexpr (TV) {
            if (k > 1) {                                   // knot k−1's B (B's last reader was G)
#pragma unroll
                for (int s = 0; s < BPT; ++s) {
                    const int e = tid + 256 * s;
                    Bim[(e % NP) + (e / NP) * PL] = Bn[s];
                }
            }
#pragma unroll
            for (int t = 0; t < 3; ++t) {                  // Q_k's P_ tiles straight from HBM
                const int i = wg4_pn_row(w, t) < 0 ? w : wg4_pn_row(w, t);
                Qt[t] = wg4_tload(Qb + (size_t)(k - 1) * sQ + 16 * i + (size_t)16 * w * NP, NP, lane);
            }
        }
        // m = 32, time-invariant (NS1): wave 3 alone refines X ≈ E⁻¹ and publishes it through the free
        // PB image while waves 0–2 form the K-independent part Q + A[:, i]ᵀPA[:, w] of their three
        // P_ tiles — the knot's critical path drops from 16 + 4 + 18 tile products (inverse in every
        // wave, 3/3/2/2 P_ tiles) to 16 + 4 + 6 (3/3/3/1 tiles, wg4_pn_row1)
        // (time-varying problems keep the inverse in every wave: with Q_k's tiles from HBM added
        // after the barrier the TV / TV+LIN variants measured 73.2 vs 72.7 and 159.5 vs 121.1 ms,
        // profiles/r06/u)
        constexpr bool NS1 = MT == 2 && !TV;
        acc PnA[NS1 ? 3 : 1];
        if constexpr (NS1) {
            if (w != 3) {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int i = wg4_pn_row1(w, t);
                    PnA[t] = wg4_tload(Qim + 16 * i + 16 * w * PL, PL, lane);                     // Q[i][w]
#pragma unroll
                    for (int kk = 0; kk < NT; ++kk) {
                        const acc At = t == 0 ? Ar[kk] : wg4_tload(Acur + 16 * kk + 16 * i * PL, PL, lane);
                        wg4_mtn<T>(PnA[t], At, PA[kk]);
                    }
                }
            }
        }
        // :42 X ≈ E⁻¹ (warm-started Newton–Schulz; the exact sweep on wave 0 otherwise)
        bool have = false;
        if (NS1 && k < N - 1) {
            T *Ximg = PBim;                              // free after B2 (the sweep reuses it only when !have)
            if (w == 3) {
                acc Id[MT][MT], E[MT][MT];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < MT; ++j) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) Id[i][j][r] = (i == j && Tile<T>::row(lane, r) == tcol(lane)) ? (T)1 : (T)0;
                        E[i][j] = wg4_tload(Eim + 16 * i + 16 * j * CS, CS, lane);
                        const acc x1 = Xi[i][j];
                        Xi[i][j] = (T)2 * x1 - Xp[i][j];
                        Xp[i][j] = x1;
                    }
                have = !a.ns_off && ns_refine<T, MT>(Xi, E, Id, lane);
                if (have) {
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < MT; ++j) wg4_tstore(Ximg + 16 * i + 16 * j * CS, CS, Xi[i][j], lane);
                }
                if (lane == 0) vote[0] = have ? 1 : 0;
            }
            __syncthreads();                             // wave 3's verdict (uniform by construction) and X
            have = vote[0] != 0;
            if (have && w != 3) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < MT; ++j) Xi[i][j] = wg4_tload(Ximg + 16 * i + 16 * j * CS, CS, lane);
            }
        } else if (k < N - 1) {
            // warm start 2X_{k+1} − X_{k+2}; Xp takes X_{k+1} before the refinement
            acc Id[MT][MT];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) Id[i][j][r] = (i == j && Tile<T>::row(lane, r) == tcol(lane)) ? (T)1 : (T)0;
                    const acc x1 = Xi[i][j];
                    Xi[i][j] = (T)2 * x1 - Xp[i][j];
                    Xp[i][j] = x1;
                }
            acc E[MT][MT];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j) E[i][j] = wg4_tload(Eim + 16 * i + 16 * j * CS, CS, lane);
            have = !a.ns_off && ns_refine<T, MT>(Xi, E, Id, lane);
            // workgroup-uniform verdict by construction (the branch below holds a barrier): each
            // wave posts its own Newton–Schulz verdict, every wave takes the AND of all four — no
            // reliance on the four refinements agreeing bitwise.  (The slots are rewritten only
            // after this knot's B3, which every wave reaches after reading them.)
            if (lane == 0) vote[w] = have ? 1 : 0;
            __syncthreads();
            have = (vote[0] & vote[1] & vote[2] & vote[3]) != 0;
        }
        if (!have) {                                       // uniform (k == N − 1, or the vote above)
            if (w == 0) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < MT; ++j)
                        wg4_tstore(aug + 16 * i + 16 * j * CS, CS, wg4_tload(Eim + 16 * i + 16 * j * CS, CS, lane), lane);
                wsync_w();
                const bool ok = aug_ldl_forward<T, MP, 0, CS>(aug, lane);
                if (lane == 0) *flag = ok ? 1 : 0;
            }
            __syncthreads();
            if (!*flag && info == 0) info = k;
            acc Wt[MT][MT], DW[MT][MT];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j) Wt[i][j] = wg4_tload(aug + MP * CS + 16 * i + 16 * j * CS, CS, lane);
            const T *rinv = aug + 2 * MP * CS + 64;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const T sc = rinv[i * 16 + Tile<T>::row(lane, r)];
#pragma unroll
                    for (int j = 0; j < MT; ++j) DW[i][j][r] = Wt[i][j][r] * sc;
                }
            tiles_zero<T, MT, MT>(Xi);
            mma_tn<T, MT, MT, MT>(Xi, Wt, DW);             // X = Wᵀ D⁻¹ W = E⁻¹
            if (k == N - 1) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < MT; ++j) Xp[i][j] = Xi[i][j];
            }
        }
        // K[:, w] = XᵀG[:, w]  → sol.K[k−1] columns 16w…16w+15
        acc Kt[MT];
#pragma unroll
        for (int c = 0; c < MT; ++c) {
            Kt[c] = acc{0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < MT; ++i) wg4_mtn<T>(Kt[c], Xi[i][c], G[i]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Kb[(size_t)(k - 1) * nm + 16 * c + Tile<T>::row(lane, r) + (size_t)(16 * w + tcol(lane)) * MP] = Kt[c][r];
        }
        if constexpr (LIN) {
            // d = Xᵀw (w = r + Bᵀp, the companion of K = XᵀG); p_k rows 16w… = q + Aᵀp − Gᵀd
            T *ws_ = wslot + w * MP, *ds_ = dslot + w * MP;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const T wj = rg[(size_t)(k - 1) * sr + 16 * j + tcol(lane)] + lin_rowsum(wv[j]);   // r + Bᵀp
                if (lane < 16) ws_[16 * j + lane] = wj;
            }
            wsync_w();
            T wrow[MT][4], dv[MT];
            lin_rows<T, MT>(wrow, ws_, lane);
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                dv[j] = (T)0;
#pragma unroll
                for (int i = 0; i < MT; ++i) dv[j] = wg4_vtn<T>(dv[j], Xi[i][j], wrow[i]);
                dv[j] = lin_rowsum(dv[j]);
                if (lane < 16) {
                    ds_[16 * j + lane] = dv[j];
                    if (w == 0) dg[(size_t)(k - 1) * MP + 16 * j + lane] = dv[j];
                }
            }
            wsync_w();
            T drow[MT][4];
            lin_rows<T, MT>(drow, ds_, lane);
            T ap = (T)0, gd = (T)0, prow[NT][4];
            lin_rows<T, NT>(prow, pk1, lane);
#pragma unroll
            for (int kk = 0; kk < NT; ++kk) ap = wg4_vtn<T>(ap, Ar[kk], prow[kk]);
#pragma unroll
            for (int c = 0; c < MT; ++c) gd = wg4_vtn<T>(gd, G[c], drow[c]);
            const T pn = qg[(size_t)(k - 1) * sq + 16 * w + tcol(lane)] + lin_rowsum(ap) - lin_rowsum(gd);
            if (lane < 16) {
                pimg[(k & 1) * NP + 16 * w + lane] = pn;
                if (pallv) pallv[(size_t)(k - 1) * NP + 16 * w + lane] = pn;
            }
        }
        // :51 P_ tiles (i, w) = Q + A[:, i]ᵀPA[:, w] − G[:, i]ᵀK[:, w] → the P image, mirrored
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int i = NS1 ? wg4_pn_row1(w, t) : wg4_pn_row(w, t);
            if (i < 0) continue;
            acc Pn;
            if (NS1 && w != 3) {
                Pn = PnA[NS1 ? t : 0];                   // Q + A[:, i]ᵀPA[:, w] formed beside the inverse
            } else {
                if constexpr (TV) Pn = Qt[t];
                else Pn = wg4_tload(Qim + 16 * i + 16 * w * PL, PL, lane);                       // Q[i][w]
#pragma unroll
                for (int kk = 0; kk < NT; ++kk) {
                    const acc At = t == 0 ? Ar[kk] : wg4_tload(Acur + 16 * kk + 16 * i * PL, PL, lane);  // A[kk][i]
                    wg4_mtn<T>(Pn, At, PA[kk]);
                }
            }
#pragma unroll
            for (int c = 0; c < MT; ++c)
                wg4_mtn<T, true>(Pn, wg4_tload(Gim + 16 * c + 16 * i * CS, CS, lane), Kt[c]);
            T *at = Pim + 16 * i + 16 * w * PL, *mr = Pim + 16 * w + 16 * i * PL;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = Tile<T>::row(lane, r), cc = tcol(lane);
                if (i != w) {
                    at[rr + cc * PL] = Pn[r];
                    mr[cc + rr * PL] = Pn[r];
                } else if (rr >= cc) {                     // diagonal tile: its lower triangle
                    at[rr + cc * PL] = Pn[r];
                    at[cc + rr * PL] = Pn[r];
                }
            }
        }
        if constexpr (TV) Rw = Rn;
        __syncthreads();                                   // B3: P_ image complete
        if (Pall)
            for (int e = tid; e < NP * NP; e += 256) Pall[(size_t)(k - 1) * nn + e] = Pim[(e % NP) + (e / NP) * PL];
    }
    if (!a.p_all)
        for (int e = tid; e < NP * NP; e += 256) ((T *)a.P)[b * nn + e] = Pim[(e % NP) + (e / NP) * PL];
    if constexpr (LIN) {
        if (!a.p_all && tid < NP) ((T *)a.p)[(size_t)b * NP + tid] = pimg[NP + tid];   // p_1 (buffer 1)
    }
    if (a.info && tid == 0) a.info[b] = info;
    // rollout once every wave's K (and d) stores are visible to the waves that read them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    dp_rollout_wg4<T, MT, TV, LIN>(a, b, lds, w, lane);
}

// The launchers.  lqrx_dp_canon.hip includes this file for dp_riccati_kernel alone and leaves them
// out: its VAR_CANON / VAR_MASK instantiations are compiled in that unit, so that this unit holds
// the instantiations it always held (the compiler's code for a kernel was seen to depend on which
// other instantiations share its module).
#ifndef LQRX_DP_KERNELS_ONLY
template <int MT>
static hipError_t launch_wg4(const DpArgs &a, hipStream_t s)
{
    dim3 grid((unsigned)a.batch), block(256);
    return with_bools(a.lin, a.tv_AB || a.tv_QR, [&](auto lin, auto tv) {
        constexpr int VAR = (decltype(lin)::value ? VAR_LIN : 0) | (decltype(tv)::value ? VAR_TV : 0);
        hipLaunchKernelGGL((dp_wg4_kernel<double, MT, VAR>), grid, block, 0, s, a);
        return hipGetLastError();
    });
}

// the VAR bits of a solve kind (enum DpKind): each kind carries the bits of the kinds below it
constexpr int var_of(int kind)
{
    return (kind >= DP_LINEAR ? VAR_LIN : 0) | (kind >= DP_AFFINE ? VAR_AFF : 0) | (kind >= DP_CROSS ? VAR_CROSS : 0) |
           (kind >= DP_VALUE ? VAR_VALUE : 0);
}

// ------------------------------------------------------------------ launcher
template <typename T, int NT, int MT, int WAVES, int VAR>
static hipError_t launch_dp(const DpArgs &a, hipStream_t s);

// One tile grid's variants, each at its launch bound (waves per SIMD) — the occupancy table:
//   grid (16·NT × 16·MT)   plain / LIN / AFF / CROSS   VAR_TV   VAR_TV|VAR_LIN(|VAR_AFF(|VAR_CROSS))
//   1×1                     2                   2        2
//   2×1                     2                   2        fp64 1, fp32 2
//   2×2                     2                   1        1
//   4×2                     1                   1        1
template <typename T, int NT, int MT>
static hipError_t launch_dp_tv(const DpArgs &a, int kind, hipStream_t s)
{
    // time-invariant (plain, linear terms, affine offset): 2 waves/SIMD up to n ≤ 32, 1 at n ≤ 64.
    // 2×2 fp64 tiles do not fit 256 registers (≈ 450 live): the 2-wave launch bound compiles
    // to occupancy 1 (hipcc: "desired occupancy 2, final occupancy 1"; 44–60 B of spills).
    // Declaring one wave per SIMD instead gave an allocation with 124 B of spills whose launch
    // ended the process with SIGABRT on the box (round 6, profiles/r06/d) — kept at the launch
    // bound that passes, see DESIGN §3.1
    constexpr int WAVES = NT <= 2 ? 2 : 1;
    // 2 waves/SIMD where the time-varying kernel fits 256 registers without spills (tile
    // grids up to 2×1, i.e. n ≤ 32, m ≤ 16 — cfg4's shape), else 1
    constexpr int TVW = (NT <= 2 && MT <= 1) ? 2 : 1;
    // linear cost terms.  Time-varying: the extra vectors tip cfg4's 2×1 double grid over 256
    // VGPRs (72–91 spilled at 2 waves/SIMD), so VAR_TV|VAR_LIN runs 2 waves/SIMD only on the
    // 1×1 (double) and up to 2×1 (float) grids; time-invariant LIN keeps the plain kernel's
    // occupancy (its vector work sits after the solve, where fewer tiles are live)
    constexpr int LW = (NT * MT <= (sizeof(T) == 4 ? 2 : 1)) ? 2 : 1;
    // (the affine offset, the cross term and the value constant keep the linear-terms launch bounds)
    return with_kind(kind, [&](auto k) {
        return with_bool(a.tv_AB || a.tv_QR, [&](auto tv) {
            constexpr int KIND = decltype(k)::value, TV = decltype(tv)::value;
            constexpr int VAR = var_of(KIND) | (TV ? VAR_TV | (KIND == DP_PLAIN ? LQRX_DP_TVEXTRA : 0) : 0);
            return launch_dp<T, NT, MT, !TV ? WAVES : (KIND == DP_PLAIN ? TVW : LW), VAR>(a, s);
        });
    });
}

template <typename T, int NT, int MT, int WAVES, int VAR>
static hipError_t launch_dp(const DpArgs &a, hipStream_t s)
{
    dim3 grid((unsigned)a.batch), block(64);
    return with_bool(a.n == NT * 16 && a.m == MT * 16, [&](auto full) {
        hipLaunchKernelGGL((dp_riccati_kernel<T, NT, MT, WAVES, VAR, decltype(full)::value>), grid, block, 0, s, a);
        return hipGetLastError();
    });
}

hipError_t dp_launch(const DpArgs &a_in, hipStream_t s)
{
    static const int ns_off = [] { const char *e = std::getenv("LQRX_DP_NS_OFF"); return e && *e == '1' ? 1 : 0; }();
    DpArgs a = a_in;
    a.ns_off = ns_off;
    const int kind = dp_kind(a);   // the one check that the flags nest; the launchers take the kind
    if (kind < 0) return hipErrorInvalidValue;
    // n ≤ 4: one lane per trajectory (a 16×16 MFMA tile would be mostly padding)
    if (dp_lane_supported(a.n, a.m)) return dp_lane_launch(a, kind, s);
    // smallest instantiated tile grid that covers (n, m); padding is exact (zero rows /
    // columns, unit diagonal in R), see tiles_load
    const int nt = (a.n + 15) / 16, mt = (a.m + 15) / 16;
    // LQRX_DP_BIG=1 sends every shape past the lane kernel to dp_big_kernel (A/B checks)
    static const bool force_big = [] { const char *e = std::getenv("LQRX_DP_BIG"); return e && *e == '1'; }();
    if (force_big && dp_big_supported(a.n, a.m)) return dp_big_launch(a, s);
    // fp64, n = 64, m ∈ {16, 32}: four waves per trajectory — time-invariant or time-varying, with
    // or without linear terms (LQRX_DP_WG4=0 in the environment: the one-wave kernel, for A/B
    // runs and tests)
    static const bool wg4 = [] { const char *e = std::getenv("LQRX_DP_WG4"); return !(e && *e == '0'); }();
    // plain time-invariant fp64 n = 32, m = 16, P_1 only: canonical coordinates (LQRX_DP_CANON=0 in
    // the environment: the generic kernel, for A/B runs and tests; LQRX_DP_PREFB=0, read in
    // dp_canon_launch: canonical without the pre-feedback tier).  The other exact grids stay
    // generic.
    static const bool canon = [] { const char *e = std::getenv("LQRX_DP_CANON"); return !(e && *e == '0'); }();
    return with_dtype(a.dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (std::is_same_v<T, double>)
            if (canon && kind == DP_PLAIN && !a.tv_AB && !a.tv_QR && !a.p_all && a.layout == 0 && a.n == 32 && a.m == 16) {
                bool ran = false;                    // false: the pool had no workspace — the generic launch
                const hipError_t e = dp_canon_launch(a, s, &ran);
                if (ran || e != hipSuccess) return e;
            }
        if (nt <= 1 && mt <= 1) return launch_dp_tv<T, 1, 1>(a, kind, s);
        if (nt <= 2 && mt <= 1) return launch_dp_tv<T, 2, 1>(a, kind, s);
        if (nt <= 2 && mt <= 2) return launch_dp_tv<T, 2, 2>(a, kind, s);
        // (an affine or cross call takes the one-wave kernel below: dp_wg4_kernel has no c_k, no M_k)
        if constexpr (std::is_same_v<T, double>)
            if (wg4 && kind <= DP_LINEAR && a.n == 64 && (a.m == 16 || a.m == 32))
                return a.m == 16 ? launch_wg4<1>(a, s) : launch_wg4<2>(a, s);
        if (nt <= 4 && mt <= 2) return launch_dp_tv<T, 4, 2>(a, kind, s);    // cfg5: n=64 m=32
        return dp_big_launch(a, s);     // past the register tiles: workgroup per trajectory
    });
}

bool dp_supported(int dtype, int n, int m, bool tv)
{
    (void)dtype;
    (void)tv;
    if (dp_lane_supported(n, m)) return true;
    const int nt = (n + 15) / 16, mt = (m + 15) / 16;
    return (n >= 1 && m >= 1 && nt <= 4 && mt <= 2) || dp_big_supported(n, m);
}

// ------------------------------------------------------------------ J = V_1(x0)
// dp_value_cost_kernel<T> — behind a value solve of any family, on its outputs: one thread per
// trajectory reads P_1 (symmetric, column-major n×n), p_1, s_1 and x0, accumulates
// ½x0ᵀP_1x0 + p_1ᵀx0 + s_1 in double and rounds to T.  Element e of trajectory b sits at
// [b·S + e] (layout 0, S the array's elements per trajectory) or [e·batch + b] (layout 1); with
// p_all, P_1 / p_1 / s_1 are element block 0 of N.  n² + 2n + 1 loads per trajectory: the solve
// itself moved (N−1)·(mn + n + m) and more.
template <typename T>
__global__ __launch_bounds__(256) void dp_value_cost_kernel(const DpArgs a, T *__restrict__ J)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.batch) return;
    const int n = a.n;
    const int64_t kP = a.p_all ? a.N : 1;
    const bool soa = a.layout == 1;
    const int64_t es = soa ? a.batch : 1;                       // element stride
    const T *P = (const T *)a.P + (soa ? b : b * (int64_t)n * n * kP);
    const T *p = (const T *)a.p + (soa ? b : b * (int64_t)n * kP);
    const T *x = (const T *)a.x0 + (soa ? b : b * (int64_t)n);
    const T *sv = (const T *)a.vs;
    double acc = a.p_all ? (double)sv[soa ? b : b * kP] : (double)sv[b];   // s_1
    for (int j = 0; j < n; ++j) {
        const double xj = (double)x[j * es];
        double col = 0.0;
        for (int i = 0; i < n; ++i) col += (double)P[((int64_t)j * n + i) * es] * (double)x[i * es];
        acc += xj * (0.5 * col + (double)p[j * es]);
    }
    J[b] = (T)acc;
}

hipError_t dp_value_cost_launch(const DpArgs &a, void *J, hipStream_t s)
{
    dim3 grid((unsigned)((a.batch + 255) / 256)), block(256);
    if (a.dtype == 0) hipLaunchKernelGGL((dp_value_cost_kernel<double>), grid, block, 0, s, a, (double *)J);
    else hipLaunchKernelGGL((dp_value_cost_kernel<float>), grid, block, 0, s, a, (float *)J);
    return hipGetLastError();
}

#endif // LQRX_DP_KERNELS_ONLY

} // namespace lqrx
