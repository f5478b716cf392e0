/* solve-kernel instantiations with the collocation and adaptive shooting integrators (static loss models); see msd_geometry.hpp */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_general(const KernelId &id)
{
    MSD_KERNEL(64, 1, 1, LOSS_STATIC, false, true, 0, 1)
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, true, 0, 1)
    MSD_KERNEL(128, 2, 1, LOSS_STATIC, false, true, 0, 1)
    return nullptr;
}
}
