/* TEST-ONLY: host emulation, kernel family "full" (see emu_common.h) */
#include "emu_common.h"

EmuFn emu_kernels_full(const msd::KernelId &id)
{
    /* split solves: first pass (fused iteration only), the same behind the least-squares multiplier estimate, follow-up kernel -- and the kernel with
     * everything in it (PART = 0: EMU_MONOLITHIC).  No 64 x 1 follow-up kernel: the 64 x 2 one follows up (emu_driver.cpp); 128 x 2 with both brakes only */
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_RG, 1)
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_RG, 3)
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_RG, 0)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_RG, 1)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_RG, 3)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_RG, 2)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_RG, 0)
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 1)
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 3)
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 0)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 1)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 3)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 2)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 0)
    EMU_KERNEL(128, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 1)
    EMU_KERNEL(128, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 3)
    EMU_KERNEL(128, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 2)
    EMU_KERNEL(128, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 0)
    /* the first-pass kernels with the second-order correction inside the fused iteration (msd_kernels_full4.hip: both brakes, 64 x 1 and the 64 x 2 kernel
     * with the node constants in LDS; EMU_SOCK) */
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 1, false, true)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_BOTH, 1, true, true)
    return nullptr;
}
