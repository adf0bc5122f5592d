// frame_pair_overlap_check.cpp -- the one pure host function of the overlapping pair kernel (gem_amd/csrc/gem_frame_pair.hpp):
// frame_pair_same_map, which decides per launch whether one block -> tile computation and one set of map words may serve both fused
// sweeps.  Against a plain statement: two argument blocks describe the same map exactly when every word the tile half reads of the
// map and of the tile map agrees; a difference in any ONE of them is seen, a difference in what belongs to the sweep (its bucket,
// its count, its queued increments, its dense flag) is not.  Host only, built with the address and undefined-behaviour sanitizers.
#include "../../gem_amd/csrc/gem_frame_pair.hpp"

#include <cstdio>

using namespace gem;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main()
{
    static float layer[2][4];
    static uint32_t words[2][4];
    FuseArgs base{};
    base.elevation = layer[0]; base.variance = layer[1]; base.L = 600; base.row0 = 0; base.row1 = 600;
    base.mahal = 5.0f; base.var_floor = 1e-4f; base.T = 1444; base.tiles_per_row = 38; base.center_tr = 7; base.center_tc = 30;
    base.bkt = words[0]; base.bcount = words[1];
    CHECK(frame_pair_same_map(base, base), "a block and itself");
    // ---- one map word differs: never the same map, in either order
    int seen = 0;
    for (int f = 0; f < 11; ++f) {
        FuseArgs o = base;
        switch (f) {
        case 0: o.elevation = layer[1]; break;     case 1: o.variance = layer[0]; break;
        case 2: o.L = 599; break;                  case 3: o.row0 = 16; break;
        case 4: o.row1 = 584; break;               case 5: o.mahal = 4.0f; break;
        case 6: o.var_floor = 2e-4f; break;        case 7: o.T = 1443; break;
        case 8: o.tiles_per_row = 37; break;       case 9: o.center_tr = 8; break;
        case 10: o.center_tc = 29; break;
        }
        CHECK(!frame_pair_same_map(base, o) && !frame_pair_same_map(o, base), "field %d", f);
        ++seen;
    }
    // ---- what belongs to the sweep may differ: the two sweeps of a pair have their own buffer sets, increments and flags
    {
        FuseArgs o = base;
        o.bkt = words[1]; o.bcount = words[0]; o.dense = 1; o.n_pending = 2; o.pending[0] = 1e-4f; o.pending[1] = 2e-4f;
        CHECK(frame_pair_same_map(base, o) && frame_pair_same_map(o, base), "sweep words");
    }
    // ---- an empty slot (launch_frame_pair's no_fuse) is never the map of a filled one
    CHECK(!frame_pair_same_map(base, FuseArgs{}), "empty slot");
    printf("fields %d fails %d\n", seen, fails);
    printf(fails ? "FAILED\n" : "ok\n");
    return fails ? 1 : 0;
}
