// gem_voxel.hpp -- the VoxelGrid pre-filter on the device (internal header): argument block, device state and host launcher of
// gem_voxel.hip.  One stage = seven launches, none of which waits for another workgroup (hand-overs inside a launch go to the LAST
// workgroup to arrive, through one returning atomic; nobody spins):
//   k_vox_bounds    min / max of the bounds points, survivor count; the last arriver derives the voxel geometry
//   k_vox_hist      NaN tail (or the pass-through copy), per-workgroup histogram of key digit 0; the last arriver scans it
//   k_vox_scatter   three stable LSD passes of 11 bits over (key, input position); pass k also counts digit k + 1 of every record
//                   into the workgroup that will hold it in pass k + 1, and the last arriver scans those counts
//   k_vox_heads     voxel heads per workgroup of the sorted records; the last arriver scans them and writes m
//   k_vox_centroid  one lane per voxel head: walks the voxel's run in input order, divides, writes the centroid at the voxel's rank
#pragma once

#include "../../include/gem_hip.h"
#include "gem_lsd.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gem {

// the sort's geometry is gem_lsd.hpp's (shared with the octree builder); the other kernels of a stage walk the records the same way
constexpr int kVoxThreads = kLsdThreads;              // 8 waves
constexpr int kVoxItems = kLsdItems;                  // records per thread
constexpr int kVoxTile = kLsdTile;                    // records per workgroup (4096): wave w takes [w * 512, w * 512 + 512)
constexpr int kVoxDigit = kLsdDigit;                  // bits per sort pass (three passes cover the 32-bit key)
constexpr int kVoxBins = kLsdBins;

enum { kVoxSort = 0, kVoxPassThrough = 1, kVoxEmpty = 2 };

// device state of the handle's voxel stages (zeroed once; every kernel leaves its counters zero behind it)
struct VoxState {
    uint32_t acc[8];          // k_vox_bounds: ordered max x, y, z | ordered ~min x, y, z | bounds points | survivors
    uint32_t ticket[8];       // arrivals per kernel
    float    inv[3];
    int      min_b[3];
    uint32_t mul[3];
    int      mode;            // kVoxSort / kVoxPassThrough / kVoxEmpty
    uint32_t S;               // survivors
    uint32_t pad[3];
    int      count[4];        // m of each stage but the last (the next stage's input count)
};

struct VoxStageArgs {
    long long n;                          // points of the call: grid bound and output length
    const int* n_dev;                     // this stage's input count on the device (NULL: n)
    const float4* in; const uint32_t* rgb_in;
    float4* out; uint32_t* rgb_out;       // n points: the m centroids, then NaN (x, y, z) with intensity 0
    int* count_out;
    float leaf[3];
    int   field;                          // GEM_VOXEL_FIELD_*
    double lo, hi;                        // limits of the point test
    float  lo_f, hi_f;                    // ... cast to float, for the bounds (getMinMax3D)
    int   negative;
    VoxState* st;
    uint32_t* hist[2];                    // [nb][kVoxBins] each, all-zero between stages
    uint32_t* key[2]; uint32_t* src[2];   // [n] records of the passes (ping-pong)
    uint32_t* heads;                      // [nb]
    int nb;
};

inline long long vox_blocks(long long n) { return n > 0 ? (n + kVoxTile - 1) / kVoxTile : 0; }
// the arenas of a call of n points: state (zeroed once), the two histograms (zeroed once), the records and the chain's two intermediates
inline size_t vox_state_bytes() { return 256; }
inline size_t vox_hist_bytes(long long n) { return (size_t)vox_blocks(n) * kVoxBins * sizeof(uint32_t) * 2 + 256; }
inline size_t vox_rec_bytes(long long n) { return ((size_t)n * 4 + 256) * 4 + (size_t)vox_blocks(n) * 4 + 256; }
inline size_t vox_tmp_bytes(long long n) { return ((size_t)n * 16 + 256) * 2 + ((size_t)n * 4 + 256) * 2; }

// the seven kernels of one stage on `st` (n > 0)
hipError_t launch_voxel_stage(hipStream_t st, const VoxStageArgs& a);

} // namespace gem
