/* solve-kernel instantiations with the structure of the reference's scripts compiled in (FULL_RG: regenerative brake only -- forceMinPn = 0,
 * figure5.py:88, figure6.py:108, figure10.py:17, table3.py:18 --, power rows, energy objective, constant efficiencies); see msd_kernels_full.hip.
 * These solves are split launches (solve_kernel: PART): this unit holds the first-pass kernels -- the fused iteration alone --,
 * msd_kernels_rg2.hip the follow-up kernels (general iteration, restoration phase, second attempt). */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
/* the ladder hands these kernels XCH_FAST exchange arrays (and no reduction scratch for a single wave): the layout of a kernel whose Solver::FAST holds */
static_assert(Solver<64, 2, LOSS_STATIC, false, false, FULL_RG, 1>::FAST && Solver<256, 2, LOSS_STATIC, false, false, FULL_RG, 3>::FAST, "the tuning switches of this build (MSD_PARALLEL_RICCATI) leave no fused iteration: the ladder of msd_select.hpp would size the LDS wrongly");
KernelFn kernels_rg(const KernelId &id)
{
    MSD_KERNEL(64, 1, 1, LOSS_STATIC, false, false, FULL_RG, 1)
    MSD_KERNEL(64, 1, 1, LOSS_STATIC, false, false, FULL_RG, 3)
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, false, FULL_RG, 1, true)
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, false, FULL_RG, 3, true)
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, false, FULL_RG, 1)
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, false, FULL_RG, 3)
    MSD_KERNEL(128, 2, 1, LOSS_STATIC, false, false, FULL_RG, 1)
    MSD_KERNEL(128, 2, 1, LOSS_STATIC, false, false, FULL_RG, 3)
    MSD_KERNEL(192, 2, 1, LOSS_STATIC, false, false, FULL_RG, 1)
    MSD_KERNEL(192, 2, 1, LOSS_STATIC, false, false, FULL_RG, 3)
    MSD_KERNEL(256, 2, 1, LOSS_STATIC, false, false, FULL_RG, 1)
    MSD_KERNEL(256, 2, 1, LOSS_STATIC, false, false, FULL_RG, 3)
    return nullptr;
}
}
