/* solve-kernel instantiations for the dynamic loss model: the first-pass kernels without a structure compiled in (with one: msd_kernels_dynamic2.hip,
 * msd_kernels_dynamic3.hip); see msd_geometry.hpp, msd_select.hpp */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_dynamic(const KernelId &id)
{
    MSD_KERNEL(64, 1, 1, LOSS_TABLE, false, false, 0, 1)
    MSD_KERNEL(128, 1, 1, LOSS_TABLE, false, false, 0, 1)
    MSD_KERNEL(64, 2, 1, LOSS_TABLE, false, false, 0, 1)
    MSD_KERNEL(128, 2, 1, LOSS_TABLE, false, false, 0, 1)
#ifndef MSD_MINIMAL_GEOMETRIES      /* tuning builds (tools/build_variant.py) */
    MSD_KERNEL(192, 2, 1, LOSS_TABLE, false, false, 0, 1)
    MSD_KERNEL(256, 2, 1, LOSS_TABLE, false, false, 0, 1)
    MSD_KERNEL_UNUSED(192, 3, 1, LOSS_TABLE, false, false, 0, 1)
    MSD_KERNEL(320, 2, 2, LOSS_TABLE, false, false, 0, 1)
#endif
    return nullptr;
}
}
