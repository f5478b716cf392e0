/* solve-kernel instantiations for combined options: collocation / adaptive shooting integrators together with the dynamic loss model
 * (ocp.py:92 with efficiency.py) or with integrateLosses (ocp.py:92 with ocp.py:231-241: the loss integrals have their own time-domain
 * integrator, train.py:367-413, whatever integrates the shooting intervals); see msd_geometry.hpp */
#include <hip/hip_runtime.h>

#include "msd_geometry.hpp"

namespace msd {
KernelFn kernels_compose(const KernelId &id)
{
    MSD_KERNEL(64, 1, 1, LOSS_TABLE, false, true, 0, 1)
    MSD_KERNEL(128, 1, 1, LOSS_TABLE, false, true, 0, 1)
    MSD_KERNEL(128, 2, 1, LOSS_TABLE, false, true, 0, 1)
    MSD_KERNEL(64, 1, 1, LOSS_INTEGRATED, false, true, 0, 1)
    MSD_KERNEL(128, 1, 1, LOSS_INTEGRATED, false, true, 0, 1)
    MSD_KERNEL(256, 1, 1, LOSS_INTEGRATED, false, true, 0, 1)
    return nullptr;
}
}
