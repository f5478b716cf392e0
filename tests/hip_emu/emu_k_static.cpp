/* TEST-ONLY: host emulation, kernel family "static" (see emu_common.h) */
#include "emu_common.h"

EmuFn emu_kernels_static(const msd::KernelId &id)
{
    /* the time-optimal problem with the structure of the rolling stock compiled in (msd_kernels_time.hip / time2.hip) */
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_TIME_RG, 1)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_TIME_RG, 1)
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, false, msd::FULL_TIME_BOTH, 1)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, msd::FULL_TIME_BOTH, 1)
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, false, 0, 1)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, false, 0, 1)
    EMU_KERNEL(128, 1, 1, msd::LOSS_STATIC, false, false, 0, 1)
    EMU_KERNEL(128, 2, 1, msd::LOSS_STATIC, false, false, 0, 1)
    EMU_KERNEL(192, 2, 1, msd::LOSS_STATIC, false, false, 0, 1)
    EMU_KERNEL(256, 2, 1, msd::LOSS_STATIC, false, false, 0, 1)
    EMU_KERNEL(192, 3, 1, msd::LOSS_STATIC, false, false, 0, 1)
    EMU_KERNEL(320, 2, 1, msd::LOSS_STATIC, false, false, 0, 1)
    /* the streamed follow-up kernel of the family */
    EMU_KERNEL(128, 5, 1, msd::LOSS_STATIC, true, false, 0, 2)
    return nullptr;
}
