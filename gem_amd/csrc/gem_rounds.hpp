// gem_rounds.hpp -- the host loop of the tiled fixed-point kernels (the potential of gem_costmap_navplan, the labels of
// gem_costmap_frontiers): rounds enqueued in CHUNKS, each chunk closed by a kernel that answers "a tile is still marked" or not through
// pinned host memory.  Pure C++17: no HIP and no handle here, the callers' lambdas launch and wait (tests/cpp/rounds_check.cpp drives
// it on the CPU with counting lambdas).
//
// The round count depends on the data, so the host loops: a chunk of rounds, the closing kernel, a wait, a look at the converged
// word, the next chunk while it is not set.  A round behind convergence finds no active tile and costs one empty launch.  The total
// is bounded by the cell count, as Bellman-Ford's is: after round r every cell whose chain -- its cheapest path to the start, its
// links to its component's smallest cell -- crosses at most r tile seams holds its final value (its tile ran behind the round that
// settled the edge cell the chain last entered through, and a tile's round ends at its local fixed point), a chain has at most
// `cells` cells, and one more round finds nothing to mark.  The bound is in the loop's condition, and the last chunk is cut at it.
#pragma once

#include <algorithm>

namespace gem {

struct RoundsResult {
    long long rounds = 0;               // rounds enqueued
    int chunks = 0;                     // chunks closed: host round trips
    bool converged = false;             // what the last close reported
};

// enqueue_round(int round) enqueues one round; close_chunk(int round, bool& converged) enqueues the closing kernel behind the chunk
// (round: the rounds so far), waits and reads the answer.  Both return 0 to go on; anything else stops the loop and is returned.
// Returns 0 with out.converged false when the bound was reached: the caller's failure.
template <class EnqueueRound, class CloseChunk>
int run_tile_rounds(long long cells, long long chunk, EnqueueRound&& enqueue_round, CloseChunk&& close_chunk, RoundsResult& out)
{
    out = RoundsResult{};
    chunk = std::max(chunk, 1ll);
    const long long max_rounds = cells + 2;                             // (fits an int: a costmap has at most 2^30 cells)
    while (!out.converged && out.rounds < max_rounds) {
        const long long n_rounds = std::min(chunk, max_rounds - out.rounds);
        for (long long r = 0; r < n_rounds; ++r, ++out.rounds)
            if (const int rc = enqueue_round((int)out.rounds)) return rc;
        if (const int rc = close_chunk((int)out.rounds, out.converged)) return rc;
        ++out.chunks;
    }
    return 0;
}

} // namespace gem
