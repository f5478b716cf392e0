/* solve-kernel instantiations for the dynamic loss model with the structure of the reference's rolling stock compiled in (FULL_RG); see msd_kernels_dynamic.hip */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_dynamic2(const KernelId &id)
{
    MSD_KERNEL(64, 1, 1, LOSS_TABLE, false, false, FULL_RG, 1)
    MSD_KERNEL(128, 1, 1, LOSS_TABLE, false, false, FULL_RG, 1)
    MSD_KERNEL(128, 2, 1, LOSS_TABLE, false, false, FULL_RG, 1)
    MSD_KERNEL(192, 2, 1, LOSS_TABLE, false, false, FULL_RG, 1)
    return nullptr;
}
}
