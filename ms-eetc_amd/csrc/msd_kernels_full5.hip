/* the first-pass kernels of msd_kernels_full.hip once more, with the early results inside (solve_kernel: EARLY -- completion words, the mirror of the stats
 * records, the iteration budget): what a begun batch (msd_solve_batch_begin) or a handle with an iteration budget launches.  A unit of its own, so that the
 * default kernels' code objects carry nothing of it. */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_full5(const KernelId &id)
{
#ifndef MSD_HOT_ONLY_64X2      /* (tuning builds of the benchmark geometry alone, like msd_kernels_full.hip) */
    MSD_KERNEL_EARLY(64, 1, 1, LOSS_STATIC, false, false, FULL_BOTH, 1)
    MSD_KERNEL_EARLY(64, 1, 1, LOSS_STATIC, false, false, FULL_BOTH, 3)
#endif
    MSD_KERNEL_EARLY(64, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1, true)
    MSD_KERNEL_EARLY(64, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 3, true)
    MSD_KERNEL_EARLY(64, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1)
    MSD_KERNEL_EARLY(64, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 3)
#ifndef MSD_HOT_ONLY_64X2
    MSD_KERNEL_EARLY(128, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1)
    MSD_KERNEL_EARLY(128, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 3)
    MSD_KERNEL_EARLY(192, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1)
    MSD_KERNEL_EARLY(192, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 3)
    MSD_KERNEL_EARLY(256, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1)
    MSD_KERNEL_EARLY(256, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 3)
#endif
    return nullptr;
}
}
