// The MapGrid side of the C++ facade (gem.hpp): gem::Costmap::adjustPlan / prepareMapGrid / mapGrid / scoreMapGrid.  Without a GPU
// ("0") it checks the host-only plan adjustment and shows that the facade compiles and links; with one ("1") it runs against
// hand-derived answers on a 5 x 5 map.  "bench <grid file> <size_x> <size_y> <resolution> <plan file> <rounds>" times the host
// baseline the device grids replace: gem_costmap_read of the whole map plus computeTargetDistance's literal queue, run twice (path,
// goal), and prints the rounds' times in microseconds (tools/bench_mapgrid.py).
#include "gem/gem.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::Costmap;
using gem::FootprintPoint;
using gem::FootprintPose;

// MapGrid::computeTargetDistance as the library runs it: a FIFO queue, neighbours in the order -x, +x, -y, +y, marked on first touch
static void queue_distance(const unsigned char* grid, int sx, int sy, const std::vector<int>& sources, std::vector<int>& dist,
                           std::vector<unsigned char>& marked, std::vector<int>& queue)
{
    const int OB = sx * sy, UN = OB + 1;
    dist.assign((size_t)OB, UN);
    marked.assign((size_t)OB, 0);
    queue.resize((size_t)OB + sources.size());
    size_t head = 0, tail = 0;
    for (int c : sources) { dist[c] = 0; marked[c] = 1; queue[tail++] = c; }
    auto touch = [&](int cur, int nb) {
        if (marked[nb]) return;
        marked[nb] = 1;
        if (grid[nb] >= 253) { dist[nb] = OB; return; }
        dist[nb] = dist[cur] + 1;
        queue[tail++] = nb;
    };
    while (head < tail) {
        const int cur = queue[head++], cx = cur % sx, cy = cur / sx;
        if (cx > 0) touch(cur, cur - 1);
        if (cx < sx - 1) touch(cur, cur + 1);
        if (cy > 0) touch(cur, cur - sx);
        if (cy < sy - 1) touch(cur, cur + sx);
    }
}

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

static int bench(int argc, char** argv)
{
    if (argc < 8) { std::printf("bench: <grid file> <size_x> <size_y> <resolution> <plan file> <rounds>\n"); return 2; }
    const int sx = std::atoi(argv[3]), sy = std::atoi(argv[4]), rounds = std::atoi(argv[7]);
    const double res = std::atof(argv[5]);
    const std::vector<unsigned char> g = slurp(argv[2]), pb = slurp(argv[6]);
    if (sx < 1 || sy < 1 || rounds < 1 || g.size() != (size_t)sx * sy || pb.empty() || pb.size() % 16) { std::printf("bench: bad input\n"); return 2; }
    std::vector<FootprintPoint> plan(pb.size() / 16);
    std::memcpy(&plan.front().x, pb.data(), pb.size());
    gem::ElevationMap map(32, 0.1f);
    Costmap cm(map, (unsigned)sx, (unsigned)sy, res, 0.0, 0.0, Costmap::FREE_SPACE);
    cm.write(0, 0, sx, sy, g);
    std::vector<int> dist, queue, path_src, goal_src;
    std::vector<unsigned char> marked;
    long long check = 0;
    for (int r = 0; r < rounds + 2; ++r) {                           // two rounds of warm-up
        gem_synchronize(map.handle());
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<unsigned char> now = cm.read(0, 0, sx, sy);
        const std::vector<FootprintPoint> adj = Costmap::adjustPlan(plan, res);
        path_src.clear(); goal_src.clear();
        bool started = false;
        for (const FootprintPoint& p : adj) {                         // setTargetCells: the first run of points on the map and not unknown
            const int mx = (int)(p.x / res), my = (int)(p.y / res);
            const bool ok = p.x >= 0.0 && p.y >= 0.0 && mx < sx && my < sy && now[(size_t)my * sx + mx] != 255;
            if (ok) { path_src.push_back(my * sx + mx); started = true; }
            else if (started) break;
        }
        if (started) goal_src.push_back(path_src.back());
        queue_distance(now.data(), sx, sy, path_src, dist, marked, queue);
        check += dist[(size_t)sx * sy / 2];
        queue_distance(now.data(), sx, sy, goal_src, dist, marked, queue);
        check += dist[(size_t)sx * sy / 2];
        const auto t1 = std::chrono::steady_clock::now();
        if (r >= 2) std::printf("%.1f\n", std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    std::printf("check %lld\n", check);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "bench")) return bench(argc, argv);
    {   // (0, 0) -> (0.25, 0): closer than a cell, nothing inserted; -> (1.25, 0): exactly one apart, nothing inserted (the test is >);
        // -> (1.25, 2.5): ceil(2.5) = 3 steps, two points inserted
        const std::vector<FootprintPoint> plan{{0.0, 0.0}, {0.25, 0.0}, {1.25, 0.0}, {1.25, 2.5}};
        const std::vector<FootprintPoint> adj = Costmap::adjustPlan(plan, 1.0);
        CHECK(adj.size() == 6);
        if (adj.size() == 6) {
            CHECK(adj[2].x == 1.25 && adj[2].y == 0.0 && adj[5].y == 2.5);
            CHECK(adj[3].x == 1.25 && adj[3].y == 0.0 + 1 * (2.5 / 3) && adj[4].y == 0.0 + 2 * (2.5 / 3));
        }
        CHECK(Costmap::adjustPlan({}, 1.0).empty());
        bool threw = false;
        try { Costmap::adjustPlan(plan, 0.0); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
    }
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: built)\n");
        return fails ? 1 : 0;
    }
    gem::ElevationMap map(32, 0.1f);
    {
        Costmap cm(map, 5, 5, 1.0, 0.0, 0.0, Costmap::FREE_SPACE);
        std::vector<unsigned char> g(25, 0);
        for (int y = 0; y < 4; ++y) g[y * 5 + 2] = Costmap::LETHAL_OBSTACLE;      // a wall in column 2 with its gap in row 4
        cm.write(0, 0, 5, 5, g);
        bool threw = false;
        try { cm.mapGrid(Costmap::PathGrid); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // never prepared
        cm.prepareMapGrid({{0.5, 0.5}});                                          // the cell (0, 0)
        const int OB = 25;
        const std::vector<int> want{0, 1, OB, 11, 12,     //
                                    1, 2, OB, 10, 11,     //
                                    2, 3, OB, 9,  10,     //
                                    3, 4, OB, 8,  9,      //
                                    4, 5, 6,  7,  8};
        for (Costmap::MapGridWhich w : {Costmap::PathGrid, Costmap::GoalGrid}) {
            const Costmap::MapGrid got = cm.mapGrid(w);
            CHECK(got.dist == want && got.started && got.goalX == 0 && got.goalY == 0);
        }
        // three trajectories of two poses: ends on (4, 4) | passes the wall | leaves the map
        const std::vector<FootprintPose> poses{FootprintPose::fromYaw(0.5, 0.5, 0.0), FootprintPose::fromYaw(4.5, 4.5, 0.0),
                                               FootprintPose::fromYaw(2.5, 1.5, 0.0), FootprintPose::fromYaw(1.5, 1.5, 0.0),
                                               FootprintPose::fromYaw(1.5, 1.5, 0.0), FootprintPose::fromYaw(5.5, 1.5, 0.0)};
        CHECK(cm.scoreMapGrid(Costmap::PathGrid, poses, 2) == (std::vector<long long>{8, 2, -4}));
        CHECK(cm.scoreMapGrid(Costmap::PathGrid, poses, 2, 0.0, GEM_MAPGRID_SUM) == (std::vector<long long>{8, OB + 2, -4}));
        CHECK(cm.scoreMapGrid(Costmap::GoalGrid, poses, 2, 0.0, GEM_MAPGRID_STOP_ON_FAILURE) == (std::vector<long long>{8, -3, -4}));
        CHECK(cm.scoreMapGrid(Costmap::PathGrid, poses, 2, 1.0) == (std::vector<long long>{-4, OB, -4}));     // one cell ahead (cos = 1)
        cm.updateOrigin(1.0, 0.0);                                                // the map moved: the grids are stale
        threw = false;
        try { cm.scoreMapGrid(Costmap::PathGrid, poses, 2); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
        cm.prepareMapGrid({{-3.0, -3.0}}, GEM_MAPGRID_GOAL);                      // never on the map
        const Costmap::MapGrid none = cm.mapGrid(Costmap::GoalGrid);
        CHECK(!none.started && none.goalX == -1 && none.dist == std::vector<int>(25, OB + 1));
        threw = false;
        try { cm.mapGrid(Costmap::PathGrid); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // only the goal grid was prepared again
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
