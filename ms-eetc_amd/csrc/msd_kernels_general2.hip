/* solve-kernel instantiations with the collocation and adaptive shooting integrators (static loss models), 257 ... 640 nodes; see
 * msd_kernels_general.hip and msd_geometry.hpp */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_general2(const KernelId &id)
{
#ifndef MSD_MINIMAL_GEOMETRIES
    MSD_KERNEL(192, 2, 1, LOSS_STATIC, false, true, 0, 1)
    MSD_KERNEL(256, 2, 1, LOSS_STATIC, false, true, 0, 1)
    MSD_KERNEL(320, 2, 2, LOSS_STATIC, false, true, 0, 1)
#endif
    return nullptr;
}
}
