// lqrx_dp_canon.hip — set-up of the input-canonical form of a time-invariant LQR problem
// ("canonical coordinates"), one wavefront per trajectory.
//
// Householder QR of B (n×m, m ≤ n, exact tile grids):  TᵀB = [B₁; 0], T orthogonal, B₁ upper
// triangular, S = B₁⁻¹.  In x̃ = Tᵀx, ũ = B₁u the problem reads
//   Ã = TᵀAT,  B̃ = [I_m; 0],  Q̃ = TᵀQT,  Q̃f = TᵀQfT,  R̃ = SᵀRS
// and P̃_k = TᵀP_kT obeys the same recursion with BᵀPB, BᵀPA reduced to sub-blocks of P̃, P̃Ã
// (dp_riccati_kernel, VAR_CANON).  The kernel writes Ã, Q̃, Q̃f, Tᵀ (n² each), R̃, Sᵀ (m² each) of
// every trajectory and one flag per trajectory into the launch's workspace (DpCanonWs):
// flag = 1, canonical applies;  0, it does not — a reflector met a zero column (rank-deficient
// B), a non-finite value, or κ∞(B₁) = ‖B₁‖∞‖S‖∞ above the bound — and the trajectory is left to
// the generic kernel (VAR_MASK), which the launcher runs behind the canonical one;  2, canonical
// with the deadbeat pre-feedback (VAR_PREFB, lqrx_dp_prefb.hip), where κ∞(B₁) is also under
// DP_PREFB_KAPPA_F64: for those the kernel writes Q′ = Q̃ + A₁ᵀR̃A₁ in Q̃'s place and, behind Sᵀ,
// M′ = −R̃A₁ and C = S·A₁·Tᵀ (A₁ the first m rows of Ã), 36 MFMAs more per trajectory.
// 3, the pre-feedback form in the basis where A₂₁, the lower-left block of Ã, is diagonal (VAR_DIAG,
// lqrx_dp_diag.hip; n = 2m, κ∞(B₁) also under DP_DIAG_KAPPA_F64): x̃ → diag(U₁, U₂)ᵀx̃, ũ → U₁ᵀũ from the
// SVD A₂₁ = U₂ΣU₁ᵀ by a one-sided Jacobi in the wave (dg_jacobi) keep B̃ = [I; 0]; T·diag(U₁, U₂) and S·U₁
// then stand where T and S stand above, and σ is written behind the last trajectory's block.
//
// The reflectors run on the augmented matrix [B | I] (n × (m + n)), one column per lane in
// registers: after the m steps the first m lanes hold B₁ and the other n hold Tᵀ.  Reflector j's
// vector is lane j's column, broadcast by v_readlane.  The congruences are TN MFMA products on
// C-layout tiles (lqrx_tile.h); Q̃, Q̃f and R̃ are made exactly symmetric from their lower triangle.
// Symmetric Q, Qf and R are assumed, as include/lqrx.h states them: the generic kernel mirrors Q's
// lower triangle too, but reads Qf and R in full, so for a non-symmetric Qf or R the two paths would
// solve different problems.
//
// This unit also holds the VAR_CANON and VAR_MASK instantiations of dp_riccati_kernel: it includes
// lqrx_dp.hip for the kernel template alone (LQRX_DP_KERNELS_ONLY leaves that file's launchers out),
// so that lqrx_dp.hip's own module keeps the instantiations, and with them the code, it always had.
#define LQRX_DP_KERNELS_ONLY
#include "lqrx_dp.hip"

namespace lqrx {

// x of lane l ^ 1 / l ^ 2 (DPP quad_perm: no LDS traffic), for the sums over a quad of lanes
template <int CTRL> __device__ __forceinline__ double quad_swap(double v)
{
    const long long x = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(x & 0xffffffffll), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(x >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double quad_sum(double v)
{
    v += quad_swap<0xB1>(v);            // quad_perm:[1,0,3,2]
    return v + quad_swap<0x4E>(v);      // quad_perm:[2,3,0,1]
}

// One-sided (Hestenes) Jacobi on the 16 columns of W (16×16, in `img` at column stride CS), VAR_DIAG's
// set-up: on return the columns of W·V are orthogonal, u2 holds W·V·diag(1/σ) and u1 holds V, as images
// at the same stride.  Lane 4j + c holds rows 4c … 4c + 3 of column j of W and of V.  A sweep is the 15
// steps of a round-robin tournament, 8 disjoint pairs each: column 15 meets column t, the others pair up
// with i + j ≡ 2t (mod 15).  Both lanes of a pair fetch the other column (ds_bpermute), form the same
// three dot products bit for bit, and rotate their own column by the tangent of their own view,
// own ← c·(own − t·other): the two views differ by the sign of t alone (equal norms: by index).  A pair rotates while
// (w_p·w_q)² > (tol·‖w_p‖‖w_q‖)².  The sweeps are a counted loop; the verdict — a sweep went by without a
// rotation, and every σ inside [DP_DIAG_SIGMA_LO, DP_DIAG_SIGMA_HI], false for a NaN — is wave-uniform.
__device__ __forceinline__ bool dg_jacobi(const double *img, double *u1, double *u2, int CS, int lane)
{
    const int j = lane >> 2, c = lane & 3;
    double w[4], v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = img[4 * c + i + j * CS];
        v[i] = (4 * c + i == j) ? 1.0 : 0.0;
    }
    constexpr double tol = DP_DIAG_ROT_EPS * 2.220446049250313e-16, tol2 = tol * tol;
    bool conv = false;
#pragma unroll 1
    for (int sw = 0; sw < DP_DIAG_SWEEPS && !conv; ++sw) {
        bool rot = false;
#pragma unroll 1
        for (int t = 0; t < 15; ++t) {
            int k = (2 * t - j + 15) % 15;
            k = j == 15 ? t : (k == j ? 15 : k);
            const int src = 4 * k + c;
            double wo[4], vo[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                wo[i] = __shfl(w[i], src);
                vo[i] = __shfl(v[i], src);
            }
            double aa = 0.0, bb = 0.0, gg = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                aa = fma(w[i], w[i], aa);
                bb = fma(wo[i], wo[i], bb);
                gg = fma(w[i], wo[i], gg);
            }
            aa = quad_sum(aa);
            bb = quad_sum(bb);
            gg = quad_sum(gg);
            const bool r = gg * gg > tol2 * (aa * bb);
            rot = rot || r;
            // the rotation, division-free: with d = ‖other‖² − ‖own‖², h = √(d² + (2γ)²), D = |d| + h the tangent is
            // t = sign(d)·2γ/D and c = D/√(D² + (2γ)²), so own ← q·(D·own − sign(d)·2γ·other), q = 1/√(D² + (2γ)²);
            // d = 0: the lower column takes +1.  None: c = 1, c·t = 0
            const double d = bb - aa, g2 = 2.0 * gg;
            const double h2 = fma(d, d, g2 * g2);
            const double D = fabs(d) + h2 * rsqrt_nr(h2);
            const double q = rsqrt_nr(fma(D, D, g2 * g2));
            const bool pos = d != 0.0 ? d > 0.0 : j < k;
            const double cs = r ? D * q : 1.0, ct = r ? (pos ? g2 * q : -(g2 * q)) : 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[i] = fma(-ct, wo[i], cs * w[i]);
                v[i] = fma(-ct, vo[i], cs * v[i]);
            }
        }
        conv = !__any(rot);
    }
    double aa = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) aa = fma(w[i], w[i], aa);
    const double sg = sqrt(quad_sum(aa));
    const bool ok = conv && __all(sg >= DP_DIAG_SIGMA_LO && sg <= DP_DIAG_SIGMA_HI);
    const double inv = 1.0 / sg;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u2[4 * c + i + j * CS] = w[i] * inv;
        u1[4 * c + i + j * CS] = v[i];
    }
    return ok;
}

template <typename T, int NT, int MT>
__global__ __launch_bounds__(64) void dp_canon_prep_kernel(const DpArgs a, void *wsv, T kappa_max, T kappa_pf,
                                                           T kappa_dg)
{
    using acc = typename Tile<T>::acc;
    using W = DpCanonWs<T, NT, MT>;
    constexpr int NP = 16 * NT, MP = 16 * MT, NC = MP + NP;
    constexpr int TS = NP + 2, SS = MP + 2;              // image column strides
    static_assert(NC <= 64 && MP <= NP, "one column of [B | I] per lane");
    __shared__ T timg[NP * TS];                          // Tᵀ, later the symmetrize image
    __shared__ T bimg[MP * SS], simg[MP * SS];           // B₁, S

    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (b >= a.batch) return;
    constexpr size_t nn = (size_t)NP * NP, nm = (size_t)NP * MP, mm = (size_t)MP * MP;
    const T *Bb = (const T *)a.B + b * nm;
    int32_t *flag = W::flags(wsv) + b;
    T *ws = W::block(wsv, a.batch, b);

    // column `lane` of [B | I]
    T x[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (lane < MP) x[i] = Bb[i + (size_t)lane * NP];
        else x[i] = (lane - MP == i) ? (T)1 : (T)0;
    }
    bool deficient = false;
#pragma unroll
    for (int j = 0; j < MP; ++j) {
        // H_j = I − τ v vᵀ on rows j …: v from column j (LAPACK's larfg: v_j = 1, H_j x = β e_j)
        T v[NP];
        T ss = (T)0;
#pragma unroll
        for (int i = j; i < NP; ++i) {
            v[i] = readlane(x[i], j);
            ss = fma(v[i], v[i], ss);
        }
        const T alpha = v[j];
        const bool zero = !(ss > (T)0);
        deficient = deficient || zero;
        const T beta = -copysign(sqrt(ss), alpha);
        const T tau = zero ? (T)0 : (beta - alpha) / beta;
        const T sc = zero ? (T)0 : (T)1 / (alpha - beta);
        T w = x[j];
#pragma unroll
        for (int i = j + 1; i < NP; ++i) {
            v[i] *= sc;
            w = fma(v[i], x[i], w);
        }
        w *= tau;
        x[j] -= w;
#pragma unroll
        for (int i = j + 1; i < NP; ++i) x[i] = fma(-w, v[i], x[i]);
    }
    // images: B₁ (upper triangle; below it zero), Tᵀ
    if (lane < MP) {
#pragma unroll
        for (int i = 0; i < MP; ++i) bimg[i + lane * SS] = i <= lane ? x[i] : (T)0;
    } else if (lane < NC) {
#pragma unroll
        for (int i = 0; i < NP; ++i) timg[i + (lane - MP) * TS] = x[i];
    }
    __syncthreads();
    // S = B₁⁻¹ by back substitution, column `lane` (rows past the column come out zero)
    T s[MP];
    const int c = lane < MP ? lane : 0;
#pragma unroll
    for (int i = MP - 1; i >= 0; --i) {
        T r = (i == c) ? (T)1 : (T)0;
#pragma unroll
        for (int k = i + 1; k < MP; ++k) r = fma(-bimg[i + k * SS], s[k], r);
        s[i] = r / bimg[i + i * SS];
    }
    if (lane < MP) {
#pragma unroll
        for (int i = 0; i < MP; ++i) simg[i + lane * SS] = s[i];
    }
    __syncthreads();
    // κ∞(B₁) = ‖B₁‖∞‖S‖∞ from the row sums (row `lane`)
    T rb = (T)0, rs = (T)0;
    if (lane < MP) {
#pragma unroll
        for (int k = 0; k < MP; ++k) {
            rb += fabs(bimg[lane + k * SS]);
            rs += fabs(simg[lane + k * SS]);
        }
    }
    const bool finite = __all((rb + rs) < (T)INFINITY);                 // false for inf and NaN
    const T kappa = wave_max(rb) * wave_max(rs);
    const bool ok = !deficient && finite && kappa <= kappa_max;
    const bool pf = ok && kappa <= kappa_pf;                            // the pre-feedback tier (VAR_PREFB)
    if (lane == 0) *flag = ok ? (pf ? 2 : 1) : 0;
    if (!ok) return;                                                    // wave-uniform

    // T (transposed read of the Tᵀ image) and S in tiles
    acc Tn[NT][NT], Sn[MT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Tn[i][j][r] = timg[(j * 16 + tcol(lane)) + (i * 16 + Tile<T>::row(lane, r)) * TS];
    tiles_from_lds<T, MT, MT>(Sn, simg, SS, lane);
    __syncthreads();                                                    // timg is free from here
    // The diagonal-A₂₁ tier (VAR_DIAG, flag 3; wave-uniform branch), for a pre-feedback trajectory with κ∞(B₁)
    // also under kappa_dg: with the SVD A₂₁ = U₂ΣU₁ᵀ of Ã's lower-left block, T′ = T·diag(U₁, U₂) and S′ = S·U₁
    // keep B̃ = [I; 0] and make that block Σ.  Admitted when the Jacobi's verdict is good and the block as the
    // congruence below will form it from T′ — the same products in the same order, so the same bits — has a
    // diagonal σ above DP_DIAG_OFF_EPS·ε·σ_max and nothing beside it above that bound (what the solve kernel then
    // drops is a backward error in A of that size).  T′ and S′ then stand where T and S stood in everything below.
    // Otherwise nothing here has touched T, S or the workspace: flag 2, the parent's bytes.
    if constexpr (NT == 2 && MT == 1) {
        if (pf && kappa <= kappa_dg) {
            acc Ttt[NT][NT], Xa[NT][NT], Yc[NT][1], Tc[NT][1], Zc[1][1];
            tiles_from_lds<T, NT, NT>(Ttt, timg, TS, lane);             // Tᵀ's tiles, as they stand in the image
            tiles_load<T, NT, NT, true>(Xa, (const T *)a.A + b * nn, NP, NP, NP, lane, false);
            // Ã₂₁ = (AᵀT₂)ᵀT₁
            auto lower_left = [&](const acc (&Tm)[NT][NT]) {
#pragma unroll
                for (int k = 0; k < NT; ++k) Tc[k][0] = Tm[k][1];
                tiles_zero<T, NT, 1>(Yc);
                mma_tn<T, NT, NT, 1>(Yc, Xa, Tc);
#pragma unroll
                for (int k = 0; k < NT; ++k) Tc[k][0] = Tm[k][0];
                tiles_zero<T, 1, 1>(Zc);
                mma_tn<T, NT, 1, 1>(Zc, Yc, Tc);
            };
            lower_left(Tn);
            __syncthreads();
            tiles_to_lds<T, 1, 1>(Zc, bimg, SS, lane);                  // B₁'s image is dead: W, then U₂
            __syncthreads();
            const bool jac = dg_jacobi(bimg, timg, bimg, SS, lane);     // U₁ to the head of the Tᵀ image
            __syncthreads();
            if (jac) {
                acc U[NT][1][1], Tp[NT][NT], Stt[1][1], Sp[1][1];
                tiles_from_lds<T, 1, 1>(U[0], timg, SS, lane);
                tiles_from_lds<T, 1, 1>(U[1], bimg, SS, lane);
                // T′ = T·diag(U₁, U₂): tile (i, j) = (Tᵀ's tile (j, i))ᵀ·U_j;  S′ = (Sᵀ)ᵀ·U₁
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        Tp[i][j] = acc{0, 0, 0, 0};
#pragma unroll
                        for (int r = 0; r < 4; ++r) Tp[i][j] = Tile<T>::mma(Ttt[j][i][r], U[j][0][0][r], Tp[i][j]);
                    }
#pragma unroll
                for (int r = 0; r < 4; ++r) Stt[0][0][r] = simg[tcol(lane) + Tile<T>::row(lane, r) * SS];
                tiles_zero<T, 1, 1>(Sp);
                mma_tn<T, 1, 1, 1>(Sp, Stt, U[0]);
                lower_left(Tp);
                // σ: the block's diagonal (lane l, register r holds (row(l, r), l & 15))
                T dmax = (T)0;
                bool good = true;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (Tile<T>::row(lane, r) == tcol(lane)) {
                        dmax = Zc[0][0][r];
                        good = good && Zc[0][0][r] > (T)0;                  // false for a NaN
                    }
                // σ_min above the bound too: under it σ is no larger than what is dropped beside it, its sign is
                // rounding's, and A₂₁ is rank-deficient to working precision
                const T bound = (T)(DP_DIAG_OFF_EPS * 2.220446049250313e-16) * wave_max(dmax);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    good = good && (Tile<T>::row(lane, r) != tcol(lane) ? fabs(Zc[0][0][r]) <= bound : Zc[0][0][r] > bound);
                if (__all(good)) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (Tile<T>::row(lane, r) == tcol(lane)) W::sigma(wsv, a.batch, b)[tcol(lane)] = Zc[0][0][r];
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j) Tn[i][j] = Tp[i][j];
                    Sn[0][0] = Sp[0][0];
                    tiles_to_lds<T, 1, 1>(Sp, simg, SS, lane);          // the pre-feedback data reads S from its image
                    if (lane == 0) *flag = 3;
                }
            }
            __syncthreads();
        }
    }
    // Tᵀ and Sᵀ: T's and S's tiles stored transposed
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                ws[W::oTt + (j * 16 + tcol(lane)) + (size_t)(i * 16 + Tile<T>::row(lane, r)) * NP] = Tn[i][j][r];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                ws[W::oSt + (j * 16 + tcol(lane)) + (size_t)(i * 16 + Tile<T>::row(lane, r)) * MP] = Sn[i][j][r];

    // R̃ = Sᵀ(RᵀS)
    acc Rm[MT][MT], RS[MT][MT], Rc[MT][MT];
    tiles_load<T, MT, MT, true>(Rm, (const T *)a.R + b * mm, MP, MP, MP, lane, false);
    tiles_zero<T, MT, MT>(RS);
    mma_tn<T, MT, MT, MT>(RS, Rm, Sn);
    tiles_zero<T, MT, MT>(Rc);
    mma_tn<T, MT, MT, MT>(Rc, Sn, RS);
    tiles_symmetrize_lower<T, MT>(Rc, timg, lane);
    tiles_store<T, MT, MT, true>(Rc, ws + W::oR, MP, MP, MP, lane);

    acc X[NT][NT], Y[NT][NT], Z[NT][NT];
    // Ã = TᵀAT = (AᵀT)ᵀT
    tiles_load<T, NT, NT, true>(X, (const T *)a.A + b * nn, NP, NP, NP, lane, false);
    tiles_zero<T, NT, NT>(Y);
    mma_tn<T, NT, NT, NT>(Y, X, Tn);
    tiles_zero<T, NT, NT>(Z);
    mma_tn<T, NT, NT, NT>(Z, Y, Tn);
    tiles_store<T, NT, NT, true>(Z, ws + W::oA, NP, NP, NP, lane);
    // the pre-feedback tier's own data (wave-uniform branch), A₁ = the first m rows of Ã:
    //   M′ = −R̃A₁ (R̃ exactly symmetric: R̃ᵀA₁),  R̃A₁ kept for Q′ below,
    //   C = S·A₁·Tᵀ = S·(T₁ᵀA), T₁ the first m columns of T (A₁Tᵀ = T₁ᵀA·TTᵀ): from A's and T's tiles
    //   as they stand, Sᵀ's tile a transposed read of the S image
    acc A1[MT][NT], RA[MT][NT];
    if (pf) {
        acc Mn[MT][NT], T1[NT][MT], W1[MT][NT], Stt[MT][MT], Cc[MT][NT];
        tiles_zero<T, MT, NT>(RA);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) A1[i][j] = Z[i][j];
        mma_tn<T, MT, MT, NT>(RA, Rc, A1);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) Mn[i][j] = -RA[i][j];
        tiles_store<T, MT, NT, true>(Mn, ws + W::oMp, MP, NP, MP, lane);
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int i = 0; i < MT; ++i) T1[k][i] = Tn[k][i];
        tiles_zero<T, MT, NT>(W1);
        mma_tn<T, NT, MT, NT>(W1, T1, X);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Stt[i][j][r] = simg[(j * 16 + tcol(lane)) + (i * 16 + Tile<T>::row(lane, r)) * SS];
        tiles_zero<T, MT, NT>(Cc);
        mma_tn<T, MT, MT, NT>(Cc, Stt, W1);
        // C as the lanes hold its tiles (tile, lane, register): the solve kernel reads 32 B per lane and tile
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) ws[W::oC + ((size_t)((i * NT + j) * 64 + lane)) * 4 + r] = Cc[i][j][r];
    }
    // Q̃ = Tᵀ(QT), Q the symmetric matrix that the generic kernel reads: the lower triangle, mirrored
    tiles_load_lower<T, NT, true>(X, (const T *)a.Q + b * nn, NP, NP, lane);
    tiles_symmetrize_lower<T, NT>(X, timg, lane);
    tiles_zero<T, NT, NT>(Y);
    mma_tn<T, NT, NT, NT>(Y, X, Tn);
    tiles_zero<T, NT, NT>(Z);
    mma_tn<T, NT, NT, NT>(Z, Tn, Y);
    if (pf) mma_tn_lower<T, MT, NT>(Z, A1, RA);                         // Q′ = Q̃ + A₁ᵀ(R̃A₁), in Q̃'s place
    tiles_symmetrize_lower<T, NT>(Z, timg, lane);
    tiles_store<T, NT, NT, true>(Z, ws + W::oQ, NP, NP, NP, lane);
    // Q̃f = Tᵀ(QfᵀT)
    tiles_load<T, NT, NT, true>(X, (const T *)a.Qf + b * nn, NP, NP, NP, lane, false);
    tiles_zero<T, NT, NT>(Y);
    mma_tn<T, NT, NT, NT>(Y, X, Tn);
    tiles_zero<T, NT, NT>(Z);
    mma_tn<T, NT, NT, NT>(Z, Tn, Y);
    tiles_symmetrize_lower<T, NT>(Z, timg, lane);
    tiles_store<T, NT, NT, true>(Z, ws + W::oQf, NP, NP, NP, lane);
}

// The canonical-form solve: the set-up fills a pool workspace and sorts the trajectories into four
// tiers; the VAR_DIAG kernel solves those flagged 3, the VAR_PREFB kernel those flagged 2, the VAR_CANON
// kernel those flagged 1, the generic kernel behind them (VAR_MASK) the ones the set-up did not admit —
// over the same grid, each an empty launch (16 µs) when it has none.  Stream-ordered throughout: no host synchronisation.  Where
// the pool cannot give the workspace (44 KB per trajectory) nothing is launched and *ran is false.
hipError_t dp_canon_launch(const DpArgs &a_in, hipStream_t s, bool *ran)
{
    using W = DpCanonWs<double, 2, 1>;
    void *ws = nullptr;
    *ran = false;
    if (scratch_alloc(&ws, W::bytes(a_in.batch), s) != hipSuccess) {
        (void)hipGetLastError();                     // the allocation's error is not the caller's
        return hipSuccess;
    }
    *ran = true;
    DpArgs a = a_in;
    a.M = ws;
    dim3 grid((unsigned)a.batch), block(64);
    // LQRX_DP_PREFB=0 in the environment (read once): no trajectory gets flag 2 — κ∞ ≥ 1 is above a
    // zero bound — so the pre-feedback candidates go to the VAR_CANON kernel.  LQRX_DP_DIAG=0 likewise: no
    // flag 3, the diagonal-A₂₁ candidates go to the pre-feedback kernel; LQRX_DP_PREFB=0 switches both off
    static const bool prefb = [] { const char *e = std::getenv("LQRX_DP_PREFB"); return !(e && *e == '0'); }();
    static const bool diag = [] { const char *e = std::getenv("LQRX_DP_DIAG"); return !(e && *e == '0'); }();
    hipLaunchKernelGGL((dp_canon_prep_kernel<double, 2, 1>), grid, block, 0, s, a, ws, DP_CANON_KAPPA_F64,
                       prefb ? DP_PREFB_KAPPA_F64 : 0.0, prefb && diag ? DP_DIAG_KAPPA_F64 : 0.0);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = dp_diag_launch(a, s);
    if (e == hipSuccess) e = dp_prefb_launch(a, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((dp_riccati_kernel<double, 2, 1, 2, VAR_CANON, true>), grid, block, 0, s, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL((dp_riccati_kernel<double, 2, 1, 2, VAR_MASK, true>), grid, block, 0, s, a);
        e = hipGetLastError();
    }
    const hipError_t f = scratch_free(ws, s);
    return e != hipSuccess ? e : f;
}

} // namespace lqrx
