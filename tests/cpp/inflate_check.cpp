// The inflation side of the C++ facade (gem.hpp): gem::InflationParams and gem::Costmap::inflate / resetWindow.  Without a GPU ("0") it
// checks the host-only table and shows that the facade compiles and links; with one ("1") it runs against hand-derived answers.  At
// resolution 1 with inflation radius 2, inscribed radius 1 and scaling factor 1 the cell radius is 2 and the costs by squared distance
// are 254, 253, 252 e^-0.414.. = 166, (121), 252 e^-1 = 92; a squared distance of 5 is outside.
#include "gem/gem.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::Costmap;
using gem::InflationParams;

int main(int argc, char** argv)
{
    const InflationParams p(2.0, 1.0, 1.0);
    int cells = -1;
    CHECK(p.table(1.0, &cells) == (std::vector<unsigned char>{254, 253, 166, 121, 92}) && cells == 2);
    CHECK(p.table(0.5, &cells).size() == 17 && cells == 4);
    bool threw = false;
    try { InflationParams(6.5, 0.0).table(0.05); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
    CHECK(threw);                                               // 130 cells
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: built)\n");
        return fails ? 1 : 0;
    }
    gem::ElevationMap map(32, 0.1f);
    {
        Costmap master(map, 5, 5, 1.0, 0.0, 0.0, Costmap::FREE_SPACE);
        std::vector<unsigned char> g(25, 0);
        g[2 * 5 + 2] = Costmap::LETHAL_OBSTACLE;
        g[1 * 5 + 1] = Costmap::NO_INFORMATION;                  // squared distance 2: 166 is below INSCRIBED_INFLATED_OBSTACLE
        g[2 * 5 + 3] = Costmap::NO_INFORMATION;                  // squared distance 1: 253 replaces it
        g[0 * 5 + 2] = 200;                                      // an old cost above the new one stays
        master.write(0, 0, 5, 5, g);
        master.inflate(p);
        const std::vector<unsigned char> want{0,   0,   200, 0,   0,      //
                                              0,   255, 253, 166, 0,      //
                                              92,  253, 254, 253, 92,     //
                                              0,   166, 253, 166, 0,      //
                                              0,   0,   92,  0,   0};
        CHECK(master.read(0, 0, 5, 5) == want);
        master.inflate(p, 0, 0, 5, 5);                           // twice is once
        CHECK(master.read(0, 0, 5, 5) == want);
        master.inflate(InflationParams(2.0, 1.0, 1.0, true));    // inflate_unknown: any cost above FREE_SPACE replaces NO_INFORMATION
        std::vector<unsigned char> unknown = want;
        unknown[1 * 5 + 1] = 166;
        CHECK(master.read(0, 0, 5, 5) == unknown);
        master.inflate(p, 4, 4, 4, 5);                           // an empty window
        CHECK(master.read(0, 0, 5, 5) == unknown);
        master.resetWindow(1, 1, 4, 3);
        for (int y = 1; y < 3; ++y)
            for (int x = 1; x < 4; ++x) unknown[y * 5 + x] = Costmap::FREE_SPACE;
        CHECK(master.read(0, 0, 5, 5) == unknown);
        threw = false;
        try { master.inflate(InflationParams(128.0, 1.0)); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
        threw = false;
        try { master.resetWindow(0, 0, 6, 5); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw && master.read(0, 0, 5, 5) == unknown);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
