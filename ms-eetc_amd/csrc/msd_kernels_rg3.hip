/* the first-pass kernels of msd_kernels_rg.hip (regenerative brake only) once more, with the early results inside (solve_kernel: EARLY); see
 * msd_kernels_full5.hip */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_rg3(const KernelId &id)
{
    MSD_KERNEL_EARLY(64, 1, 1, LOSS_STATIC, false, false, FULL_RG, 1)
    MSD_KERNEL_EARLY(64, 1, 1, LOSS_STATIC, false, false, FULL_RG, 3)
    MSD_KERNEL_EARLY(64, 2, 1, LOSS_STATIC, false, false, FULL_RG, 1, true)
    MSD_KERNEL_EARLY(64, 2, 1, LOSS_STATIC, false, false, FULL_RG, 3, true)
    MSD_KERNEL_EARLY(64, 2, 1, LOSS_STATIC, false, false, FULL_RG, 1)
    MSD_KERNEL_EARLY(64, 2, 1, LOSS_STATIC, false, false, FULL_RG, 3)
    MSD_KERNEL_EARLY(128, 2, 1, LOSS_STATIC, false, false, FULL_RG, 1)
    MSD_KERNEL_EARLY(128, 2, 1, LOSS_STATIC, false, false, FULL_RG, 3)
    MSD_KERNEL_EARLY(192, 2, 1, LOSS_STATIC, false, false, FULL_RG, 1)
    MSD_KERNEL_EARLY(192, 2, 1, LOSS_STATIC, false, false, FULL_RG, 3)
    MSD_KERNEL_EARLY(256, 2, 1, LOSS_STATIC, false, false, FULL_RG, 1)
    MSD_KERNEL_EARLY(256, 2, 1, LOSS_STATIC, false, false, FULL_RG, 3)
    return nullptr;
}
}
