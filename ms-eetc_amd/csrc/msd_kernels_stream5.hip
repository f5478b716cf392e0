/* first-pass kernels of the streamed static family with the structure of the reference's rolling stock compiled in (FULL_RG); see msd_kernels_stream.hip */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_stream5(const KernelId &id)
{
    MSD_KERNEL(512, 2, 2, LOSS_STATIC, true, false, FULL_RG, 1)
    MSD_KERNEL(512, 4, 2, LOSS_STATIC, true, false, FULL_RG, 1)
    MSD_KERNEL(512, 6, 2, LOSS_STATIC, true, false, FULL_RG, 1)
    MSD_KERNEL(512, 10, 2, LOSS_STATIC, true, false, FULL_RG, 1)
    return nullptr;
}
}
