// lqrx_resolve_ops.h — what the kernels built on the re-solve recursion share (lqrx_dp_resolve.hip,
// lqrx_dp_box.hip): the interleaved pair of TN chains of the backward pass, the register copies of
// the one-knot-ahead operand loads, and the one map through which a column of a C-layout tile
// (lqrx_tile.h) is stored to and loaded from a per-trajectory array.
#pragma once
#include "lqrx_tile.h"

namespace lqrx {

// D1[i] += Σ_k M1[k][i]ᵀ Y[k] and D2[i] (+|−)= Σ_k M2[k][i]ᵀ Y[k], two TN chains on one B operand, in
// mma_tn's order (k-tile, k-slice outermost) with the two products' MFMAs alternating
template <typename T, int KT, int I1, int I2, bool NEG2>
__device__ __forceinline__ void tn_pair(typename Tile<T>::acc (&D1)[I1], const typename Tile<T>::acc (&M1)[KT][I1],
                                        typename Tile<T>::acc (&D2)[I2], const typename Tile<T>::acc (&M2)[KT][I2],
                                        const typename Tile<T>::acc (&Y)[KT])
{
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int i = 0; i < I1; ++i) D1[i] = Tile<T>::mma(M1[k][i][r], Y[k][r], D1[i]);
#pragma unroll
            for (int i = 0; i < I2; ++i)
                D2[i] = NEG2 ? Tile<T>::mma_nega(M2[k][i][r], Y[k][r], D2[i]) : Tile<T>::mma(M2[k][i][r], Y[k][r], D2[i]);
        }
}

template <typename T, int I, int J>
__device__ __forceinline__ void tiles_copy(typename Tile<T>::acc (&dst)[I][J], const typename Tile<T>::acc (&src)[I][J])
{
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j) dst[i][j] = src[i][j];
}

template <typename T, int I>
__device__ __forceinline__ void vec_copy(typename Tile<T>::acc (&dst)[I], const typename Tile<T>::acc (&src)[I])
{
#pragma unroll
    for (int i = 0; i < I; ++i) dst[i] = src[i];
}

// d_{t,k}: this lane's column ↔ m elements at dk.  The store of the backward pass and the load of the
// forward pass use this one map (no __restrict__: the load reads what the store wrote).
template <typename T, int IT>
__device__ __forceinline__ void d_store(const typename Tile<T>::acc (&D)[IT], T *dk, int rows, int lane, bool live)
{
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = it * 16 + Tile<T>::row(lane, r);
            if (live && row < rows) dk[row] = D[it][r];
        }
}
template <typename T, int IT>
__device__ __forceinline__ void d_load(typename Tile<T>::acc (&D)[IT], const T *dk, int rows, int lane, bool live)
{
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = it * 16 + Tile<T>::row(lane, r);
            const bool ok = live && row < rows;
            const T x = dk[ok ? row : 0];
            D[it][r] = ok ? x : T(0);
        }
}

} // namespace lqrx
