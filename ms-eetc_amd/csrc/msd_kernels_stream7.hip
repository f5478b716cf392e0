/* solve-kernel instantiations for long horizons (stage blocks in device memory), 3072 ... 5119 intervals; see msd_kernels_stream2.hip, msd_geometry.hpp */
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "msd_geometry.hpp"

namespace msd {
Geometry stream_geometry_static_spt10() { return stream_geometry_t<LOSS_STATIC, false, 10>(); }
}
