/* solve-kernel instantiations with the structure of the reference's rolling stock compiled in (both brakes, power rows, energy
 * objective, constant efficiencies: BASELINE configs 1-4); see msd_geometry.hpp and Solver::rowOn in msd_kernel.hpp.
 * These solves are split launches (solve_kernel: PART): this unit holds the first-pass kernels -- the fused iteration alone --,
 * msd_kernels_full3.hip the follow-up kernels (general iteration, restoration phase, second attempt). */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
/* the ladder hands these kernels XCH_FAST exchange arrays (and no reduction scratch for a single wave): the layout of a kernel whose Solver::FAST holds */
static_assert(Solver<64, 2, LOSS_STATIC, false, false, FULL_BOTH, 1>::FAST && Solver<256, 2, LOSS_STATIC, false, false, FULL_BOTH, 3>::FAST, "the tuning switches of this build (MSD_PARALLEL_RICCATI) leave no fused iteration: the ladder of msd_select.hpp would size the LDS wrongly");
KernelFn kernels_full(const KernelId &id)
{
#ifndef MSD_HOT_ONLY_64X2      /* tuning builds of the benchmark geometry alone (tools/build_hot.py: a fifth of the unit's compile time) */
    MSD_KERNEL(64, 1, 1, LOSS_STATIC, false, false, FULL_BOTH, 1)
    MSD_KERNEL(64, 1, 1, LOSS_STATIC, false, false, FULL_BOTH, 3)
#endif
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1, true)
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 3, true)
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1)
    MSD_KERNEL(64, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 3)
#ifndef MSD_HOT_ONLY_64X2
    MSD_KERNEL(128, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1)
    MSD_KERNEL(128, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 3)
    MSD_KERNEL(192, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1)
    MSD_KERNEL(192, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 3)
    MSD_KERNEL(256, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 1)
    MSD_KERNEL(256, 2, 1, LOSS_STATIC, false, false, FULL_BOTH, 3)
#endif
    return nullptr;
}
}
