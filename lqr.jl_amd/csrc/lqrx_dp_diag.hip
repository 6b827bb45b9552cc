// lqrx_dp_diag.hip — the VAR_CANON | VAR_PREFB | VAR_DIAG instantiation of dp_riccati_kernel (canonical
// coordinates with the deadbeat pre-feedback, rotated so that A₂₁ is diagonal) in a module
// of its own, as lqrx_dp_prefb.hip holds the VAR_CANON | VAR_PREFB one and for the same reason: no other
// instantiation gets a new module neighbour.  The set-up that fills the workspace and the launcher that
// calls this one are lqrx_dp_canon.hip's.
#define LQRX_DP_KERNELS_ONLY
#include "lqrx_dp.hip"

namespace lqrx {

hipError_t dp_diag_launch(const DpArgs &a, hipStream_t s)
{
    dim3 grid((unsigned)a.batch), block(64);
    hipLaunchKernelGGL((dp_riccati_kernel<double, 2, 1, 2, VAR_CANON | VAR_PREFB | VAR_DIAG, true>), grid, block, 0, s, a);
    return hipGetLastError();
}

} // namespace lqrx
