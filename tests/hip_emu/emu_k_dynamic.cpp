/* TEST-ONLY: host emulation, kernel family "dynamic loss table" (see emu_common.h) */
#include "emu_common.h"

EmuFn emu_kernels_dynamic(const msd::KernelId &id)
{
    /* the structure of the rolling stock compiled in (msd_kernels_dynamic2.hip / 3.hip), two geometries each */
    EMU_KERNEL(64, 1, 1, msd::LOSS_TABLE, false, false, msd::FULL_RG, 1)
    EMU_KERNEL(128, 1, 1, msd::LOSS_TABLE, false, false, msd::FULL_RG, 1)
    EMU_KERNEL(64, 1, 1, msd::LOSS_TABLE, false, false, msd::FULL_BOTH, 1)
    EMU_KERNEL(128, 1, 1, msd::LOSS_TABLE, false, false, msd::FULL_BOTH, 1)
    EMU_KERNEL(64, 1, 1, msd::LOSS_TABLE, false, false, 0, 1)
    EMU_KERNEL(64, 2, 1, msd::LOSS_TABLE, false, false, 0, 1)
    EMU_KERNEL(128, 1, 1, msd::LOSS_TABLE, false, false, 0, 1)
    EMU_KERNEL(128, 2, 1, msd::LOSS_TABLE, false, false, 0, 1)
    EMU_KERNEL(192, 2, 1, msd::LOSS_TABLE, false, false, 0, 1)
    /* the streamed follow-up kernel of the family */
    EMU_KERNEL(128, 5, 1, msd::LOSS_TABLE, true, false, 0, 2)
    return nullptr;
}
