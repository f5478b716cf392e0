/* first-pass kernels of the time-optimal problem (OptionsCasadiSolver.energyOptimal = False, ocp.py:150) with the structure of the reference's rolling stock
 * compiled in (FULL_TIME_BOTH); see msd_kernels_static.hip, msd_kernel.hpp: FULL */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_time2(const KernelId &id)
{
    MSD_KERNEL(64, 1, 1, LOSS_STATIC, false, false, FULL_TIME_BOTH, 1)
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, false, FULL_TIME_BOTH, 1)
    MSD_KERNEL(128, 2, 1, LOSS_STATIC, false, false, FULL_TIME_BOTH, 1)
    return nullptr;
}
}
