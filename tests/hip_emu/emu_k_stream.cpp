/* TEST-ONLY: host emulation, streamed kernels (see emu_common.h) */
#include "emu_common.h"

EmuFn emu_kernels_stream(const msd::KernelId &id)
{
    /* first pass, also with the structure of the rolling stock compiled in (msd_kernels_stream5.hip / 6.hip), and follow-up kernel */
    EMU_KERNEL(128, 5, 1, msd::LOSS_STATIC, true, false, msd::FULL_RG, 1)
    EMU_KERNEL(128, 5, 1, msd::LOSS_STATIC, true, false, msd::FULL_BOTH, 1)
    EMU_KERNEL(128, 5, 1, msd::LOSS_STATIC, true, false, 0, 1)
    EMU_KERNEL(128, 5, 1, msd::LOSS_STATIC, true, false, 0, 2)
    return nullptr;
}
