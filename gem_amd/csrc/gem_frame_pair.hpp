// gem_frame_pair.hpp -- two sweeps per k_frame launch: the host's hold / pair / flush decision and the pair kernel's arguments
// (internal header).
//
// A stream of single sweeps that nobody reads in between pays one launch per sweep: its dispatch front, its ramp and one HIP call
// of the host.  None of that is work the map needs per sweep, so once a handle has seen two consecutive pairable calls it HOLDS
// every other call (nothing is enqueued) and the call behind it launches one grid that runs two complete single-sweep halves: the
// tile blocks fuse the (one or two) sweeps binned by the launch before, one after the other, the binning blocks bin the held sweep
// and the new one, each into a pass buffer set of its own.  Whatever observes or modifies the map settles a held sweep first
// (flush_deferred, gem_capi_core.cpp).  The decision is a pure function of three words of state -- no clocks -- and compiles for
// the host alone (tests/cpp/frame_pair_check.cpp runs every sequence of events against a plain model).
#pragma once

#include "gem_frame_lean.hpp"

namespace gem {

// What the handle has put off: `deferred` sweeps are binned and not fused yet (0, 1, or the 2 of a pair launch), `held` is a sweep
// that was accepted and not binned yet, `streak` counts the pairable calls since the last flush.
struct FramePairState { int streak = 0; int deferred = 0; bool held = false; };

enum FrameEvent {
    kFramePairable = 0,     // a gem_add_device call that may share a launch (run_pipeline's `pairable`)
    kFrameSingle   = 1,     // a call that takes k_frame's one-launch-per-sweep path but may not be held or share a launch
    kFrameFlush    = 2,     // anything that observes or modifies the map
};

// The launches an event causes, in order.  A launch fuses the `fuse` sweeps that are deferred when it is enqueued -- all of them,
// oldest first -- and bins `bin` sweeps: the held one first if there is one, then the event's own.  What it bins is deferred behind it.
struct FramePairPlan {
    int  n = 0;
    struct Launch { int fuse, bin; } launch[3] = {};
    bool hold = false;              // the event's sweep is held: nothing is launched
    bool held_flushed = false;      // a held sweep was settled by something other than a pairable call
    int  pairs = 0;                 // launches of the plan that carry two sweeps in either half
};

constexpr int kFramePairStreak = 2;     // pairable calls in a row before the first sweep is held

inline FramePairPlan frame_pair_step(FramePairState& s, FrameEvent e)
{
    FramePairPlan p{};
    auto launch = [&](int fuse, int bin) {
        p.launch[p.n].fuse = fuse; p.launch[p.n].bin = bin; ++p.n;
        if (fuse == 2 || bin == 2) ++p.pairs;
        s.deferred = bin; s.held = false;
    };
    auto flush = [&]() {
        if (s.held) { launch(s.deferred, 1); p.held_flushed = true; }    // fuse(previous) || bin(held) ...
        if (s.deferred) launch(s.deferred, 0);                           // ... and the fuse-only launch, of a pair too
        s.streak = 0;
    };
    if (e == kFrameFlush) { flush(); return p; }
    if (e == kFrameSingle) {
        if (s.held || s.deferred == 2) flush();                          // a launch of the single form fuses one sweep and bins one
        s.streak = 0;
        launch(s.deferred, 1);
        return p;
    }
    if (s.held) { launch(s.deferred, 2); ++s.streak; return p; }         // fuse(previous one or two) || bin(held), bin(this)
    if (s.streak >= kFramePairStreak) { s.held = true; p.hold = true; ++s.streak; return p; }
    launch(s.deferred, 1);                                               // the first calls behind a flush: as a stream of singles
    ++s.streak;
    return p;
}

// The overlapping pair kernel (pairov_k_frame, gem_frame_pair.hip) computes a tile workgroup's tile ONCE for both rounds, from the
// first slot's words: the two fused sweeps must then describe the same map through the same tile map.  They do in every pair the
// policy above forms (whatever moves or resizes the map flushes); launch_frame_pair checks it per launch and picks pair_k_frame
// where it does not hold.
inline bool frame_pair_same_map(const FuseArgs& x, const FuseArgs& y)
{
    return x.elevation == y.elevation && x.variance == y.variance && x.L == y.L && x.row0 == y.row0 && x.row1 == y.row1 &&
           x.mahal == y.mahal && x.var_floor == y.var_floor &&
           x.T == y.T && x.tiles_per_row == y.tiles_per_row && x.center_tr == y.center_tr && x.center_tc == y.center_tc;
}

// The pair kernel's arguments: a small head -- the block counts of the three block ranges -- and one lean argument block per sweep
// slot.  Slot s of the tile half fuses the s-th deferred sweep (T == 0: none), slot s of the binning half bins the s-th new one
// into its own set.  The tile map is each slot's own (FrameLeanTile: the two sweeps of a pair see the same map, the words are copies).
struct FramePairArgs {
    int nf;                         // tile blocks: frame_tile_blocks(T) of the fused sweeps (0: none)
    int nbin[2];                    // binning blocks of slot 0, of slot 1 (four units each)
    int pad_;
    FrameLeanArgs s[2];
};
static_assert(sizeof(FramePairArgs) <= 16 + 2 * 352, "the pair kernel's arguments: a head and two lean blocks");

} // namespace gem
