// The footprint side of the C++ facade (gem.hpp): gem::FootprintPose and gem::Costmap::clearFootprint / footprintCost /
// scoreTrajectories.  Without a GPU ("0") it only shows that the facade compiles and links; with one ("1") it runs against hand-derived
// answers.  An 8 x 8 costmap at 0.5 m with origin (0, 0) covers [0, 4) x [0, 4); the footprint is a 1.5 m square.  At (2, 2) with
// heading 0 its vertices lie at 1.25 and 2.75, cells 2 and 5: edge 0 is the column x = 2 upwards, edge 1 the row y = 5, edge 2 the
// column x = 5 downwards, edge 3 the row y = 2.  With cos = -1, sin = 0 the walk starts at (5, 5) and goes down the column x = 5.
// Every cell holds 10 except (2, 3) = 255 and (5, 3) = 254.
#include "gem/gem.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::Costmap;
using gem::FootprintPose;

int main(int argc, char** argv)
{
    const std::vector<gem::FootprintPoint> square{{-0.75, -0.75}, {-0.75, 0.75}, {0.75, 0.75}, {0.75, -0.75}};
    const FootprintPose yaw0 = FootprintPose::fromYaw(1.0, 2.0, 0.0);
    CHECK(yaw0.x == 1.0 && yaw0.y == 2.0 && yaw0.cos_th == 1.0 && yaw0.sin_th == 0.0);
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: built)\n");
        return fails ? 1 : 0;
    }
    gem::ElevationMap map(32, 0.1f);
    {
        Costmap layer(map, 8, 8, 0.5);
        std::vector<unsigned char> g(64, 10);
        g[3 * 8 + 2] = 255; g[3 * 8 + 5] = 254;
        layer.write(0, 0, 8, 8, g);
        const FootprintPose a(2.0, 2.0, 1.0, 0.0), turned(2.0, 2.0, -1.0, 0.0), off(3.5, 2.0, -1.0, 0.0), b(2.0, 2.5, 1.0, 0.0);   // off: vertex 0 at x = 4.25
        std::vector<int> c = layer.footprintCost({a, turned, off, b}, square);
        CHECK(c == (std::vector<int>{-2, -1, -3, -2}));
        CHECK(layer.footprintCost({}, square).empty());
        // fewer than three vertices: the centre cell (4, 4) alone
        CHECK(layer.footprintCost({a}, {{0.0, 0.0}}) == std::vector<int>{10});
        bool threw = false;
        try { layer.footprintCost({a}, square, 4); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                           // an unknown flag bit

        Costmap::Bounds bd{1e30, 1e30, -1e30, -1e30};
        CHECK(layer.clearFootprint(a, square, &bd));
        CHECK(bd.min_x == 1.25 && bd.min_y == 1.25 && bd.max_x == 2.75 && bd.max_y == 2.75);
        std::vector<unsigned char> want(64, 10);
        for (int y = 2; y <= 5; ++y)
            for (int x = 2; x <= 5; ++x) want[y * 8 + x] = Costmap::FREE_SPACE;
        CHECK(layer.read(0, 0, 8, 8) == want);
        Costmap::Bounds bo{1e30, 1e30, -1e30, -1e30};
        CHECK(!layer.clearFootprint(off, square, &bo) && bo.max_x == 4.25 && layer.read(0, 0, 8, 8) == want);

        // a at (2, 2) walks cleared cells only: 0; b, half a metre up, walks the row y = 6 of tens: 10
        std::vector<int> each;
        std::vector<int> t = layer.scoreTrajectories({a, b, b, off, a, a}, 2, square, 0, &each);
        CHECK(t == (std::vector<int>{10, -3, 0}) && each == (std::vector<int>{0, 10, 10, -3, 0, 0}));
        t = layer.scoreTrajectories({b, b, a, b, off, b}, 3, square, GEM_FOOTPRINT_SUM);
        CHECK(t == (std::vector<int>{20, -3}));
        threw = false;
        try { layer.scoreTrajectories({a, b, b}, 2, square); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
