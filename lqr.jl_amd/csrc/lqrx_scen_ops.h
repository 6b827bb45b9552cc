// lqrx_scen_ops.h — the operand helpers of the kernels whose tile columns are scenarios, right-hand
// sides or ADMM instances (lqrx_dp_scen.hip, lqrx_dp_resolve.hip, lqrx_dp_box.hip): X, U and their kin
// are C-layout tiles (lqrx_tile.h) with one trajectory per column, so register r of such a tile is the
// B operand of k-slice r and a matrix enters a product as A operands loaded straight from global memory.
#pragma once
#include "lqrx_tile.h"

namespace lqrx {

constexpr int DP_COLS = 16;   // trajectories per wave (the columns of a tile)

// one wave per work item, the kernels loop over their work items with a grid stride
inline unsigned dp_grid(int64_t items)
{
    const int64_t cap = 1 << 20;
    return (unsigned)(items < cap ? items : cap);
}

// A rows×cols column-major matrix (leading dimension rows) as the A operands of D[IT] += Mat·Y[KT]:
// op[it][kt][r] = Mat(it·16 + (lane & 15), kt·16 + Tile<T>::row(lane, r)), zero past the matrix.  Loads
// are unconditional (a lane past the matrix reads element 0 and selects zero).
template <typename T, int IT, int KT>
__device__ __forceinline__ void op_load(T (&op)[IT][KT][4], const T *__restrict__ src, int rows, int cols, int lane)
{
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int row = it * 16 + (lane & 15), col = kt * 16 + Tile<T>::row(lane, r);
                const bool ok = row < rows && col < cols;
                const T v = src[ok ? row + col * rows : 0];
                op[it][kt][r] = ok ? v : T(0);
            }
}

template <typename T, int IT, int KT>
__device__ __forceinline__ void op_copy(T (&dst)[IT][KT][4], const T (&src)[IT][KT][4])
{
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[it][kt][r] = src[it][kt][r];
}

// D[it] += op·Y: k-tile and k-slice outermost, so consecutive MFMAs go to different accumulators
// wherever IT > 1
template <typename T, int IT, int KT>
__device__ __forceinline__ void op_mma(typename Tile<T>::acc (&D)[IT], const T (&op)[IT][KT][4],
                                       const typename Tile<T>::acc (&Y)[KT])
{
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int it = 0; it < IT; ++it) D[it] = Tile<T>::mma(op[it][kt][r], Y[kt][r], D[it]);
}

// a vector of `rows` elements along the rows of C-layout tiles (every column the same), zero past
// it and for a null vector
template <typename T, int IT>
__device__ __forceinline__ void rows_load(typename Tile<T>::acc (&D)[IT], const T *__restrict__ v, int rows, int lane,
                                          bool live = true)
{
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = it * 16 + Tile<T>::row(lane, r);
            const bool ok = live && row < rows;
            const T x = v ? v[ok ? row : 0] : T(0);   // a null vector is never dereferenced
            D[it][r] = ok ? x : T(0);
        }
}

// this lane's column of C-layout tiles → rows elements at dst (a live scenario's x_k or u_k)
template <typename T, int IT>
__device__ __forceinline__ void rows_store(const typename Tile<T>::acc (&D)[IT], T *__restrict__ dst, int rows,
                                           int lane, bool live)
{
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = it * 16 + Tile<T>::row(lane, r);
            if (live && row < rows) dst[row] = D[it][r];
        }
}

} // namespace lqrx
