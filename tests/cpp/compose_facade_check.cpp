// gem::LocalMap::compose of the C++ facade (gem.hpp).  Without a GPU ("0") it only has to build; with one ("1") it runs the filter
// and split on a flat map of L = 32 cells, all valid, against answers that need no neighbour search to derive:
//   1. a threshold far above every distance (stddevMul = 1e6) removes nothing: the 5 cells with travers -0.5 are the obstacles, the
//      other L^2 - 5 the road, both in grid-cloud order;
//   2. with one cell raised by 50 m and stddevMul = 3 that cell is removed (its neighbours are 50 m away, everyone else's 0.1 m)
//      and it is in neither list; the exact removed count comes from the driver (argv[2]: tests/compose_ref.py on the same scene);
//   3. compose before keepPrevious is GEM_ERR_INVALID.
#include "gem/gem.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main(int argc, char** argv)
{
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        gem_compose_params p{};
        p.mean_k = 20; p.flags = GEM_COMPOSE_SQRT_DOUBLE;
        std::printf("OK (no GPU: built)\n");
        return p.mean_k == 20 ? 0 : 1;
    }
    const int L = 32;
    gem::ElevationMap map(L, 0.1f);
    std::vector<float> elev(L * L, 0.25f), trav(L * L, 0.5f), var(L * L, 0.01f);
    for (int k = 0; k < 5; ++k) trav[(3 + 5 * k) * L + 7] = -0.5f;
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_ELEVATION, elev.data()) == GEM_OK);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_TRAVER, trav.data()) == GEM_OK);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_VARIANCE, var.data()) == GEM_OK);
    gem::LocalMap local(map, 4);
    local.capture();
    bool threw = false;
    try { local.compose(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
    CHECK(threw);
    local.keepPrevious();
    const std::vector<gem::PointXYZRGBICT> grid = local.gridCloud();
    CHECK(grid.size() == (size_t)(L * L));
    gem::LocalMap::Composed c = local.compose(20, 1e6, 0.0);
    std::printf("flat: road %zu obstacle %zu removed %d threshold %.9g\n", c.road.size(), c.obstacle.size(), c.removed, c.threshold);
    CHECK(c.removed == 0 && c.obstacle.size() == 5 && c.road.size() == (size_t)(L * L - 5) && std::isfinite(c.threshold));
    size_t ir = 0, io = 0;
    bool order = true;
    for (const auto& p : grid) {
        if (p.travers > 0.0f) { order = order && ir < c.road.size() && c.road[ir].x == p.x && c.road[ir].y == p.y; ++ir; }
        else { order = order && io < c.obstacle.size() && c.obstacle[io].x == p.x && c.obstacle[io].y == p.y && c.obstacle[io].travers == -0.5f; ++io; }
    }
    CHECK(order && ir == c.road.size() && io == c.obstacle.size());
    elev[16 * L + 16] = 50.25f;
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_ELEVATION, elev.data()) == GEM_OK);
    local.capture();
    local.keepPrevious();
    c = local.compose(20, 3.0, 0.0, true);
    std::printf("spike: road %zu obstacle %zu removed %d threshold %.9g\n", c.road.size(), c.obstacle.size(), c.removed, c.threshold);
    CHECK(c.removed >= 1 && c.road.size() + c.obstacle.size() + (size_t)c.removed == (size_t)(L * L));
    if (argc > 2) CHECK(c.removed == std::atoi(argv[2]));
    bool spike = false;
    for (const auto& p : c.road) spike = spike || p.z == 50.25f;
    for (const auto& p : c.obstacle) spike = spike || p.z == 50.25f;
    CHECK(!spike);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
