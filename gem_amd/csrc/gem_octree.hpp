// gem_octree.hpp -- octomap::ColorOcTree insertion and fullMapToMsg on the device (internal header): argument block, device state and
// host launchers of gem_octree.hip.  The contract is stated in include/gem_hip.h (gem_octree_build).  One build, no host round trip:
//   k_oct_keys     48-bit Morton key (or "none") per record, how many have one, which key bits vary; digit-0 histogram; the last
//                  arriver sets the pass count and scans the histogram
//   k_oct_scatter  up to five stable LSD passes of 11 bits over (key, input position) (gem_lsd.hpp); a pass above the count returns
//   k_oct_heads    leaf heads per workgroup of the sorted records, scanned by the last arriver: the leaf count
//   k_oct_leaves   leaf keys and segment starts
//   k_oct_kstar    every leaf's largest full aligned block (k* = 0 .. 3) by index arithmetic on the sorted unique keys; the block lists
//                  of k* = 1 and 2; k* = 0 leaves are walked right here, one lane per leaf
//   k_oct_walk     <false> eight lanes per k* = 1 block (eight blocks a wave), <true> one wave per k* = 2 block: the block's records
//                  merged by input position, prune tests as ballots
//   k_oct_count    nodes every leaf introduces in pre-order (its path from the first depth at which it leaves its predecessor's),
//                  per workgroup, scanned by the last arriver: the node count
//   k_oct_emit     offsets, the terminal nodes' 8 bytes
//   k_oct_inner    depth 15 .. 0, one launch each: value max, colour mean over set colours, child mask from the (up to) eight children,
//                  found by binary search in the sorted leaf keys
#pragma once

#include "gem_local.hpp"
#include "gem_lsd.hpp"

namespace gem {

constexpr int kOctDepth = 16;
constexpr int kOctTable = 65;                    // value / p per hit count 0 .. 64
constexpr int kOctMaxPasses = 5;                 // 5 * 11 >= 48 key bits
constexpr int kOctThreads = 256;                 // the one-item-per-thread kernels
constexpr uint32_t kOctWhite = 0x00ffffffu;      // r | g << 8 | b << 16, all 255: not set
constexpr uint32_t kOctDead = 255u;              // term level of a leaf covered by a pruned block
constexpr int kOctWalkWaves = 512;               // waves of a walker launch (they stride over the block list)

struct OctState {
    uint32_t ticket[8];
    unsigned long long acc_or, acc_and;          // over the valid keys; back to 0 / ~0 behind every build
    uint32_t acc_valid;                          // back to 0
    uint32_t S;                                  // valid records
    uint32_t npass;                              // LSD passes the varying key bits need (1 .. 5)
    uint32_t nleaves;
    uint32_t nblk[3];                            // k* = 1, 2 blocks (list lengths), k* >= 3 blocks
    uint32_t fb_leaves, fb_points;               // leaves / records of the k* >= 3 blocks
    uint32_t nnodes;
    uint32_t n_leaf_nodes, n_pruned;             // terminals at depth 16 / above it
    uint32_t pad[8];
};
static_assert(sizeof(OctState) <= 256, "the state arena");

struct OctTerm { uint32_t col_level; uint32_t cnt; };       // colour | level << 24 (kOctDead: covered), saturating hit count

struct OctArgs {
    const LocalRecord* in; long long n;          // the cloud
    double rf;
    uint32_t sat;                                // hits at which a leaf's value reaches the clamp
    const float* f_tab; const double* p_tab;     // value and blend p per hit count [kOctTable]
    OctState* st;
    unsigned long long* key_in;                  // [n] key per record, ~0 for none
    unsigned long long* key[2]; uint32_t* src[2];            // [n] the passes' records
    uint32_t* hist[2];                           // [nb][kLsdBins], all-zero between builds
    uint32_t* heads;                             // [blocks of 256 over n] per-workgroup counts, then their prefix
    unsigned long long* leaf_key; uint32_t* leaf_start;      // [n], [n + 1]
    OctTerm* term;                               // [n] per leaf
    uint32_t* off; uint8_t* d0;                  // [n] per leaf: first node's index in the stream, first depth it introduces
    uint32_t* blk[2];                            // [n / 8 + 1], [n / 64 + 1] first leaf of every k* = 1 / 2 block
    uint8_t* kstar;                              // [n]
    uint2* out; long long out_cap;               // the stream: 8 bytes per node
    int nb;                                      // workgroups of the 4096-record kernels
};

inline long long oct_blocks(long long n) { return n > 0 ? (n + kLsdTile - 1) / kLsdTile : 0; }
// nodes a tree over n leaves can have at most: at depth d there are at most min(n, 8^d)
inline long long oct_max_nodes(long long n)
{
    long long total = 0, w = 1;
    for (int d = 0; d <= kOctDepth; ++d) { total += n < w ? n : w; if (w <= n) w *= 8; }
    return total;
}

// everything up to the terminals of the k* <= 2 leaves (n > 0)
hipError_t launch_octree_front(hipStream_t st, const OctArgs& a);
// node counts, offsets, terminal and inner nodes (again after the host has patched the k* >= 3 terminals)
hipError_t launch_octree_back(hipStream_t st, const OctArgs& a);

} // namespace gem
