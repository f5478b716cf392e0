/* TEST-ONLY: host emulation, kernel family "integrated losses" (see emu_common.h) */
#include "emu_common.h"

EmuFn emu_kernels_intloss(const msd::KernelId &id)
{
    EMU_KERNEL(64, 1, 1, msd::LOSS_INTEGRATED, false, false, 0, 1)
    EMU_KERNEL(64, 2, 1, msd::LOSS_INTEGRATED, false, false, 0, 1)
    /* the streamed follow-up kernel of the family */
    EMU_KERNEL(128, 5, 1, msd::LOSS_INTEGRATED, true, false, 0, 2)
    return nullptr;
}
