// lqrx_dp_prefb.hip — the VAR_CANON | VAR_PREFB instantiation of dp_riccati_kernel (canonical
// coordinates with the deadbeat pre-feedback) in a module of its own: it includes
// lqrx_dp.hip for the kernel template alone, as lqrx_dp_canon.hip does, so that neither that unit's
// instantiations nor lqrx_dp.hip's get a new module neighbour (the compiler's code for one
// instantiation was seen to depend on them).  The set-up that fills the workspace and the launcher
// that calls this one are lqrx_dp_canon.hip's.
#define LQRX_DP_KERNELS_ONLY
#include "lqrx_dp.hip"

namespace lqrx {

hipError_t dp_prefb_launch(const DpArgs &a, hipStream_t s)
{
    dim3 grid((unsigned)a.batch), block(64);
    hipLaunchKernelGGL((dp_riccati_kernel<double, 2, 1, 2, VAR_CANON | VAR_PREFB, true>), grid, block, 0, s, a);
    return hipGetLastError();
}

} // namespace lqrx
