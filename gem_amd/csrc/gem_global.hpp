// gem_global.hpp -- the submap stack on the device (internal header): argument blocks and host launchers of gem_global.hip.
//   transform  every record of one submap through a 4x4 float matrix (pcl::transformPointCloud, PCL >= 1.10 on x86-64, restated)
//   keys       pointCloudtoHash's key of every record of a submap, the first record of a key claimed in a LocalTable (atomicMin)
//   side       stable compaction of one side of a pair step: the first record of every key, NaN keys all kept, each written as
//              localHashtoPointCloud writes its entry, fused with the other side's first record where the match test holds
// The compaction is gem_compact.hpp's.
#pragma once

#include "gem_local.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gem {

struct GlobalXform { float m[16]; };                        // column-major, as Eigen::Matrix4f::data()

// one submap of a pair step: its records and (device) count, its keys and its table
struct GlobalCloud {
    const LocalRecord* rec; const uint32_t* count;
    unsigned long long* keys;           // [count] local_key of the quantised position; the bits of a NaN key as computed
    LocalTable t;                       // key -> position of its first record (INT_MAX while free)
};

struct GlobalSideArgs {
    GlobalCloud self, other;            // the side being written and the side it is fused with
    bool self_is_new;                   // self = `new` (submap k): the fused entry's colour, intensity, travers are self's
    LocalRecord* out;
    uint32_t* fused;                    // keys fused (new side only; NULL on the old side)
};

hipError_t launch_global_transform(hipStream_t st, LocalRecord* rec, long long n, const GlobalXform& m);
// table slots [cap] cleared, then the keys of cloud c (at most `bound` records) computed and inserted; res = the quantum (double)
hipError_t launch_global_keys(hipStream_t st, const GlobalCloud& c, long long bound, double res);
// block_cnt: [compact_blocks(bound)] scratch; *total: records written (device)
hipError_t launch_global_side(hipStream_t st, const GlobalSideArgs& a, long long bound, uint32_t* block_cnt, uint32_t* total);

} // namespace gem
