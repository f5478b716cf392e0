/* solve-kernel instantiations for long horizons (stage blocks in device memory), 2048 ... 3071 intervals (3072 ... 5119: msd_kernels_stream7.hip -- the
 * two geometries in one unit made that unit the build's critical path); see msd_geometry.hpp */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_stream2(const KernelId &id)
{
    MSD_KERNEL(512, 6, 2, LOSS_STATIC, true, false, 0, 1)
    MSD_KERNEL(512, 6, 2, LOSS_STATIC, true, false, 0, 2)
    return nullptr;
}
}
