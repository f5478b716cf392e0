/* solve-kernel instantiations with the structure of the reference's rolling stock compiled in (both brakes, power rows, energy
 * objective) for the other transcriptions: collocation / adaptive shooting integrators and integrateLosses; see msd_kernels_full.hip */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_full2(const KernelId &id)
{
    MSD_KERNEL(64, 1, 1, LOSS_STATIC, false, true, 1, 1)
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, true, 1, 1)
    MSD_KERNEL(128, 1, 1, LOSS_STATIC, false, true, 1, 1)
    MSD_KERNEL(64, 1, 1, LOSS_INTEGRATED, false, false, FULL_BOTH, 1)
    MSD_KERNEL(64, 2, 1, LOSS_INTEGRATED, false, false, FULL_BOTH, 1)
    MSD_KERNEL(128, 1, 1, LOSS_INTEGRATED, false, false, FULL_BOTH, 1)
    return nullptr;
}
}
