// The local-map side of the C++ facade (gem.hpp): gem::LocalMap over an ElevationMap.  Without a GPU ("0") it only pins the
// record layout; with one ("1") it runs capture / keepPrevious / gridCloud / spill / exportCloud / size on a map whose cells are
// all valid, against hand-derived answers: L = 32, res = 0.1, centre 0, start 0 -> x = 1.55 - 0.1 ix (doubles of 0.1f); at
// current x 0.3 the window's low edge is 0.3 - 1.6 = -1.3, so the columns ix = 29, 30, 31 leave it (x = -1.35, -1.45, -1.55).
#include "gem/gem.hpp"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static_assert(offsetof(gem::PointXYZRGBICT, x) == 0 && offsetof(gem::PointXYZRGBICT, pad) == 12, "xyz pad");
static_assert(offsetof(gem::PointXYZRGBICT, covariance) == 20 && offsetof(gem::PointXYZRGBICT, intensity) == 24 &&
              offsetof(gem::PointXYZRGBICT, travers) == 28, "covariance intensity travers");

int main(int argc, char** argv)
{
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf("OK (no GPU: layout)\n");
        return 0;
    }
    const int L = 32;
    gem::ElevationMap map(L, 0.1f);
    std::vector<float> elev(L * L), trav(L * L, 0.5f), var(L * L, 0.01f);
    for (int i = 0; i < L * L; ++i) elev[i] = 0.001f * (float)i;
    trav[31 * L + 3] = -0.5f;                                  // storage cell [31][3]: captured, never spilled
    std::vector<int> red(L * L, 200);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_ELEVATION, elev.data()) == GEM_OK);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_TRAVER, trav.data()) == GEM_OK);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_VARIANCE, var.data()) == GEM_OK);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_COLOR_R, red.data()) == GEM_OK);
    {
        gem::LocalMap local(map, 4);
        bool threw = false;
        try { float c[2] = {0.f, 0.f}; local.spill(c, c); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                          // before any capture
        local.capture();
        const std::vector<gem::PointXYZRGBICT> grid = local.gridCloud();
        CHECK(grid.size() == (size_t)(L * L));
        const double r = (double)0.1f, off = 0.5 * (L * r) - 0.5 * r;      // getPositionFromIndex: (p + off) - res * unwrapped index
        CHECK(grid.size() == (size_t)(L * L) && grid[1].x == (float)((0.0 + off) + r * -1.0) && grid[0].pad == 1.0f && grid[0].r == 200 &&
              grid[0].a == 0 && grid[L].y == (float)((0.0 + off) + r * -1.0) && grid[0].x == (float)off);
        local.keepPrevious();
        const float cur[2] = {0.3f, 0.0f}, shift[2] = {0.3f, 0.0f};
        int replaced = -1;
        std::vector<gem::PointXYZRGBICT> s = local.spill(cur, shift, &replaced);
        std::printf("spill: %zu records, %d replaced\n", s.size(), replaced);
        CHECK(s.size() == 3 * (size_t)L - 1 && replaced == 0);
        bool cols = true;
        for (const auto& p : s) cols = cols && p.x < -1.3f && p.travers == 0.5f && p.covariance == 0.01f;
        CHECK(cols);
        CHECK(local.size() == 3 * L - 1);
        s = local.spill(cur, shift, &replaced);
        CHECK(s.size() == 3 * (size_t)L - 1 && replaced == 3 * L - 1);
        const std::vector<gem::PointXYZRGBICT> e = local.exportCloud(true);
        CHECK(e.size() == 3 * (size_t)L - 1);
        CHECK(e.size() == s.size() && e.front().x == s.front().x && e.back().y == s.back().y);
        CHECK(local.size() == 0);
    }
    bool threw = false;                                        // ~LocalMap switched it off
    try { long long n = 0; map.check(gem_local_size(map.handle(), &n), "gem_local_size"); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
    CHECK(threw);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
