/* solve-kernel instantiations for long horizons (stage blocks in device memory), 3072 ... 5119 intervals; see msd_kernels_stream2.hip, msd_geometry.hpp */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_stream7(const KernelId &id)
{
    MSD_KERNEL(512, 10, 2, LOSS_STATIC, true, false, 0, 1)
    MSD_KERNEL(512, 10, 2, LOSS_STATIC, true, false, 0, 2)
    return nullptr;
}
}
