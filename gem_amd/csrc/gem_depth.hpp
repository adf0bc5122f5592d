// gem_depth.hpp -- the pinhole unprojection of a depth image on the device (internal header): argument block and host launcher of
// gem_depth.hip.  The semantics are the ones include/gem_hip.h states (depth_image_proc::convert<T>, restated).
#pragma once

#include "../../include/gem_hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gem {

struct DepthArgs {
    int width, height;
    int format, color_format;              // GEM_DEPTH_*, GEM_COLOR_* (GEM_COLOR_NONE when there is no rgb output)
    const unsigned char* depth; const unsigned char* color;
    unsigned long long depth_stride, color_stride;     // bytes, never 0
    float kx, ky, cxf, cyf;                // gem_depth_constants
    float unit;                            // U16: metres per count (never 0)
    float intensity;
    bool  mask;                            // GEM_CLEAN_PASSTHROUGH_Z folded in: dropped points get NaN x, y, z
    float z_min, z_max;
    float4* xyzi; uint32_t* rgb;           // [width * height]; xyzi 16-byte aligned
};

// one launch on `st`; width * height == 0 launches nothing
hipError_t launch_depth_unproject(hipStream_t st, const DepthArgs& a);

} // namespace gem
