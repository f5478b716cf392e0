/* solve-kernel instantiations for combined options beyond the LDS-resident horizons (round 4): collocation / adaptive shooting integrators
 * together with the dynamic loss model or with integrateLosses on the streamed kernel (stage blocks in device memory), up to 1023 intervals --
 * the reference builds any option set for any N (simulations/table3.py:34 sweeps N to 5000); see msd_kernels_compose.hip, msd_kernels_stream3.hip */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_stream4(const KernelId &id)
{
    MSD_KERNEL(512, 2, 2, LOSS_TABLE, true, true, 0, 1)
    MSD_KERNEL(512, 2, 2, LOSS_TABLE, true, true, 0, 2)
    MSD_KERNEL(512, 2, 2, LOSS_INTEGRATED, true, true, 0, 1)
    MSD_KERNEL(512, 2, 2, LOSS_INTEGRATED, true, true, 0, 2)
    return nullptr;
}
}
