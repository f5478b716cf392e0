/* TEST-ONLY: host emulation, kernel family "general" (see emu_common.h) */
#include "emu_common.h"

EmuFn emu_kernels_general(const msd::KernelId &id)
{
    EMU_KERNEL(64, 1, 1, msd::LOSS_STATIC, false, true, 0, 1)
    EMU_KERNEL(64, 2, 1, msd::LOSS_STATIC, false, true, 0, 1)
    /* the streamed follow-up kernel of the family */
    EMU_KERNEL(128, 5, 1, msd::LOSS_STATIC, true, true, 0, 2)
    /* the same integrators with integrateLosses (loss rows from the integrated loss distance, msd_lossint.hpp) */
    EMU_KERNEL(64, 1, 1, msd::LOSS_INTEGRATED, false, true, 0, 1)
    EMU_KERNEL(128, 5, 1, msd::LOSS_INTEGRATED, true, true, 0, 2)
    return nullptr;
}
