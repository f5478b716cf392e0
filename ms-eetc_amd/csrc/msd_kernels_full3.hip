/* follow-up kernels of the split solves of msd_kernels_full.hip (solve_kernel's PART = 2): general iteration, restoration phase and second
 * attempt for the scenarios the first pass hands over -- or for the whole batch when none of its scenarios can start with the fused iteration */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_full3(const KernelId &id)
{
    /* (no 64 x 1 instantiation: the 64 x 2 kernel follows up the one-node-per-lane first pass, msd_select.hpp) */
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 2)
    MSD_KERNEL(128, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 2)
    MSD_KERNEL(192, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 2)
    MSD_KERNEL(256, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 2)
    return nullptr;
}
}
