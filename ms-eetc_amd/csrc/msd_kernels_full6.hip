/* the first-pass kernels of msd_kernels_full4.hip (second-order correction inside the fused iteration) once more, with the early results inside
 * (solve_kernel: EARLY); see msd_kernels_full5.hip */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_full6(const KernelId &id)
{
    MSD_KERNEL_EARLY(64, 1, 1, LOSS_STATIC, false, false, FULL_BOTH, 1, false, true)
    MSD_KERNEL_EARLY(64, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1, true, true)
    return nullptr;
}
}
