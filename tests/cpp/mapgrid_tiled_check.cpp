// The tiled MapGrid side of the C++ facade (gem.hpp): gem::Costmap::prepareMapGridTiled / prepareMapGridFrontTiled and
// gem::MapGridTiledStatus.  Without a GPU ("0") it shows that the facade compiles and links.  With one:
//     mapgrid_tiled_check 1 <grid file> <size_x> <size_y> <resolution> <plan file> <path grid file> <goal grid file>
// writes the bytes of <grid file> into a costmap at the origin, prepares both grids from the plan (pairs of doubles) with the tiled
// call and compares mapGrid's distances with the int32 files the caller computed (tests/test_mapgrid_tiled_gpu.py: a 65 x 2049 map,
// above the cap of the LDS form).
#include "gem/gem.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::Costmap;
using gem::FootprintPoint;

static std::vector<unsigned char> slurp(const char* path)
{
    std::vector<unsigned char> v;
    if (FILE* f = std::fopen(path, "rb")) {
        unsigned char buf[65536];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
        std::fclose(f);
    }
    return v;
}

int main(int argc, char** argv)
{
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        gem::MapGridTiledStatus (Costmap::*both)(const std::vector<FootprintPoint>&, int) = &Costmap::prepareMapGridTiled;
        gem::MapGridTiledStatus (Costmap::*front)(const std::vector<FootprintPoint>&) = &Costmap::prepareMapGridFrontTiled;
        gem_mapgrid_tiled_status raw{};
        raw.started = 1; raw.goal_cell[0] = 3; raw.goal_cell[1] = 4; raw.rounds = 5; raw.chunks = 2;
        const gem::MapGridTiledStatus st = gem::MapGridTiledStatus::from(raw);
        CHECK(both != nullptr && front != nullptr);
        CHECK(st.started && st.goalX == 3 && st.goalY == 4 && st.rounds == 5 && st.chunks == 2);
        std::printf(fails ? "FAILED\n" : "OK (no GPU: built)\n");
        return fails ? 1 : 0;
    }
    if (argc < 9) { std::printf("<grid file> <size_x> <size_y> <resolution> <plan file> <path grid file> <goal grid file>\n"); return 2; }
    const int sx = std::atoi(argv[3]), sy = std::atoi(argv[4]);
    const double res = std::atof(argv[5]);
    const std::vector<unsigned char> g = slurp(argv[2]), pb = slurp(argv[6]), wp = slurp(argv[7]), wg = slurp(argv[8]);
    const size_t cells = (size_t)sx * (size_t)sy;
    if (sx < 1 || sy < 1 || g.size() != cells || pb.empty() || pb.size() % 16 || wp.size() != cells * 4 || wg.size() != cells * 4) { std::printf("bad input\n"); return 2; }
    std::vector<FootprintPoint> plan(pb.size() / 16);
    std::memcpy(&plan.front().x, pb.data(), pb.size());
    std::vector<int> want_path(cells), want_goal(cells);
    std::memcpy(want_path.data(), wp.data(), wp.size());
    std::memcpy(want_goal.data(), wg.data(), wg.size());

    gem::ElevationMap map(32, 0.1f);
    Costmap cm(map, (unsigned)sx, (unsigned)sy, res, 0.0, 0.0, Costmap::FREE_SPACE);
    cm.write(0, 0, sx, sy, g);
    bool threw = false;
    try { cm.prepareMapGrid(plan); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
    CHECK(threw);                                                                 // above the cap: the LDS form still refuses
    threw = false;
    try { cm.mapGrid(Costmap::PathGrid); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
    CHECK(threw);                                                                 // ... and nothing was prepared
    const gem::MapGridTiledStatus st = cm.prepareMapGridTiled(plan);
    CHECK(st.started && st.rounds >= 1 && st.chunks >= 1);
    const Costmap::MapGrid path = cm.mapGrid(Costmap::PathGrid), goal = cm.mapGrid(Costmap::GoalGrid);
    CHECK(path.dist == want_path);
    CHECK(goal.dist == want_goal);
    CHECK(path.started && goal.started && goal.goalX == st.goalX && goal.goalY == st.goalY);
    CHECK(want_goal[(size_t)st.goalY * sx + st.goalX] == 0);
    const gem::MapGridTiledStatus fs = cm.prepareMapGridFrontTiled(plan);         // the front grid of the same plan is its goal grid
    CHECK(fs.started && fs.goalX == st.goalX && fs.goalY == st.goalY);
    CHECK(cm.mapGridFront().dist == want_goal);
    CHECK(cm.mapGrid(Costmap::PathGrid).dist == want_path);                       // PATH is not touched by it
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
