/* integrateLosses with a loss table (msd_lossint_table.hpp), the streamed kernels: first pass and follow-up kernel (restoration phase, watchdog procedure,
 * second attempt) for horizons of up to 1023 intervals; the follow-up kernel also serves the LDS-resident first-pass kernels of msd_kernels_intloss_table.hip */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_intloss_table2(const KernelId &id)
{
    MSD_KERNEL(512, 2, 2, LOSS_INTEGRATED_TABLE, true, false, 0, 1)
    MSD_KERNEL(512, 2, 2, LOSS_INTEGRATED_TABLE, true, false, 0, 2)
    return nullptr;
}
}
