/* solve-kernel instantiations for long horizons (stage blocks in device memory), up to 2047 intervals: first pass and follow-up kernel (with the structure
 * of the rolling stock compiled into the first pass: msd_kernels_stream5.hip, msd_kernels_stream6.hip); see msd_select.hpp */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_stream(const KernelId &id)
{
    MSD_KERNEL(512, 2, 2, LOSS_STATIC, true, false, 0, 1)
    MSD_KERNEL(512, 2, 2, LOSS_STATIC, true, false, 0, 2)
    MSD_KERNEL(512, 4, 2, LOSS_STATIC, true, false, 0, 1)
    MSD_KERNEL(512, 4, 2, LOSS_STATIC, true, false, 0, 2)
    return nullptr;
}
}
