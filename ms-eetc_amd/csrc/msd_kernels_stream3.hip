/* solve-kernel instantiations of the other transcriptions for horizons beyond the LDS-resident kernels (stage blocks in device memory),
 * up to 1023 intervals; see msd_geometry.hpp */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_stream3(const KernelId &id)
{
    MSD_KERNEL(512, 2, 2, LOSS_TABLE, true, false, 0, 1)
    MSD_KERNEL(512, 2, 2, LOSS_TABLE, true, false, 0, 2)
    MSD_KERNEL(512, 2, 2, LOSS_STATIC, true, true, 0, 1)
    MSD_KERNEL(512, 2, 2, LOSS_STATIC, true, true, 0, 2)
    MSD_KERNEL(512, 2, 2, LOSS_INTEGRATED, true, false, 0, 1)
    MSD_KERNEL(512, 2, 2, LOSS_INTEGRATED, true, false, 0, 2)
    return nullptr;
}
}
