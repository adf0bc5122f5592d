// gem_clean.hpp -- cleanPointCloud on the device (internal header): argument block and host launchers of gem_clean.hip.
//   stable stream compaction of a raw cloud (gem_compact.hpp) and the masking pass of the fuse path (dropped points get NaN x, y, z;
//   in place behind k_unpack_aos for AoS).
#pragma once

#include "../../include/gem_hip.h"
#include "gem_compact.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gem {

struct CleanArgs {
    long long n;
    int   mode;                        // GEM_CLEAN_*
    float z_min, z_max;                // GEM_CLEAN_PASSTHROUGH_Z, inclusive
    // input: interleaved XYZI (+ optional packed rgb) -- or, SoA form, three coordinate arrays
    const float4* xyzi; const uint32_t* rgb;
    const float* x; const float* y; const float* z;
    // outputs, kept points in input order (each may be NULL): XYZI + rgb, or (SoA form) x, y, z; input position of each
    float4* xyzi_out; uint32_t* rgb_out;
    float* x_out; float* y_out; float* z_out;
    int* orig_out;
    uint32_t* block_cnt;               // [compact_blocks(n)] scratch: kept points per workgroup, then their exclusive prefix
    int* count_out;                    // kept points (device)
};

inline size_t clean_scratch_bytes(long long n) { return (size_t)compact_blocks(n) * sizeof(uint32_t) + 64; }

// the three kernels of one compaction on `st`; n == 0 only writes *count_out = 0
hipError_t launch_clean(hipStream_t st, const CleanArgs& a, bool soa);
// out[i] = in[i], with x, y, z = NaN where the filter drops the point (the pipelines reject it in projection); in == out allowed
hipError_t launch_clean_mask(hipStream_t st, const float4* in, float4* out, long long n, int mode, float z_min, float z_max);

} // namespace gem
