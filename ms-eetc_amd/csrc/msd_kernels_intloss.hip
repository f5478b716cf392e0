/* solve-kernel instantiations for integrateLosses (loss slacks from the integrated loss power, msd_lossint.hpp); see msd_geometry.hpp */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_intloss(const KernelId &id)
{
    MSD_KERNEL(64, 1, 1, LOSS_INTEGRATED, false, false, 0, 1)
    MSD_KERNEL_UNUSED(128, 1, 1, LOSS_INTEGRATED, false, false, 0, 1)
    MSD_KERNEL(64, 2, 1, LOSS_INTEGRATED, false, false, 0, 1)
    MSD_KERNEL(128, 2, 1, LOSS_INTEGRATED, false, false, 0, 1)
#ifndef MSD_MINIMAL_GEOMETRIES      /* tuning builds (tools/build_variant.py) */
    MSD_KERNEL(192, 2, 1, LOSS_INTEGRATED, false, false, 0, 1)
    MSD_KERNEL(256, 2, 1, LOSS_INTEGRATED, false, false, 0, 1)
    MSD_KERNEL_UNUSED(192, 3, 1, LOSS_INTEGRATED, false, false, 0, 1)
    MSD_KERNEL(320, 2, 2, LOSS_INTEGRATED, false, false, 0, 1)
#endif
    return nullptr;
}
}
