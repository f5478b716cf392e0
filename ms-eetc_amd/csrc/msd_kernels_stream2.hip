/* solve-kernel instantiations for long horizons (stage blocks in device memory), 2048 ... 3071 intervals (3072 ... 5119: msd_kernels_stream7.hip -- the
 * two geometries in one unit made that unit the build's critical path); see msd_geometry.hpp */
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "msd_geometry.hpp"

namespace msd {
Geometry stream_geometry_static_spt10();      /* msd_kernels_stream7.hip */
Geometry pick_stream_geometry_static_long(int N)       /* N <= 5119: pick_stream_geometry_long_t<LOSS_STATIC>, one geometry per unit */
{
    if (N + 1 <= 3072) return stream_geometry_t<LOSS_STATIC, false, 6>();
    if (N + 1 <= 5120) return stream_geometry_static_spt10();
    return {0, 0, nullptr};
}
}
