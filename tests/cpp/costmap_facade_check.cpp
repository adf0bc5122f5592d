// The costmap side of the C++ facade (gem.hpp): gem::Costmap over an ElevationMap.  Without a GPU ("0") it only shows that the
// facade compiles and links; with one ("1") it runs the marks, the roll, the merge and the read against hand-derived answers:
// L = 32, res = 0.1f, centre 0, start 0 -> cell (ix, iy) lies near x = 1.55 - 0.1 ix, y = 1.55 - 0.1 iy and is visited at
// lin = ix + 32 iy.  An 8 x 8 costmap at 0.4 m with origin (-1.6, -1.6) takes 4 x 4 grid cells per costmap cell:
// mx = 7 - ix / 4, my = 7 - iy / 4.  traver is 0.9 except for ix < 4 (costmap column 7: lethal under both layers' tests), for
// (31, 31), the LAST cell visited of costmap cell (0, 0) (lethal: the last one decides), and for (24, 24), the FIRST one visited
// of costmap cell (1, 1) (free: fifteen later cells overwrite it).
#include "gem/gem.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::Costmap;

static bool expected(const std::vector<unsigned char>& g, int shift)
{
    // column 7 - shift lethal, cell (0 - shift, 0) lethal, columns the roll brought in NO_INFORMATION, everything else free
    bool ok = g.size() == 64;
    for (int my = 0; ok && my < 8; ++my)
        for (int mx = 0; mx < 8; ++mx) {
            const int old_mx = mx + shift;
            unsigned char want = Costmap::FREE_SPACE;
            if (old_mx > 7) want = Costmap::NO_INFORMATION;
            else if (old_mx == 7 || (old_mx == 0 && my == 0)) want = Costmap::LETHAL_OBSTACLE;
            if (g[my * 8 + mx] != want) { std::printf("cell (%d, %d): %d, expected %d\n", mx, my, g[my * 8 + mx], want); ok = false; }
        }
    return ok;
}

int main(int argc, char** argv)
{
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf("OK (no GPU: built)\n");
        return 0;
    }
    const int L = 32;
    gem::ElevationMap map(L, 0.1f);
    std::vector<float> elev(L * L, 0.25f), trav(L * L, 0.9f);
    for (int ix = 0; ix < 4; ++ix)
        for (int iy = 0; iy < L; ++iy) trav[ix * L + iy] = 0.1f;
    trav[31 * L + 31] = 0.1f;
    trav[24 * L + 24] = 0.1f;
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_ELEVATION, elev.data()) == GEM_OK);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_TRAVER, trav.data()) == GEM_OK);
    {
        gem::LocalMap local(map, 4);
        Costmap layer(map, 8, 8, 0.4, -1.6, -1.6), visual(map, 8, 8, 0.4, -1.6, -1.6), master(map, 8, 8, 0.4, -1.6, -1.6, Costmap::FREE_SPACE);
        CHECK(layer.id() != visual.id() && visual.id() != master.id());
        bool threw = false;
        try { layer.markGridCloud(0.5); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                          // no capture yet
        threw = false;
        try { layer.markGlobal(-1, 0.5); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                          // no submap stack
        CHECK(layer.read(0, 0, 8, 8) == std::vector<unsigned char>(64, Costmap::NO_INFORMATION));
        local.capture();
        Costmap::Bounds b{1e30, 1e30, -1e30, -1e30};
        layer.markGridCloud(0.5, &b);
        CHECK(expected(layer.read(0, 0, 8, 8), 0));
        // getPositionFromIndex with the capture's default geometry: r = (double)0.1f, off = 0.5 * (L * r) - 0.5 * r, x = off - r * ux;
        // the grid cloud's records hold them as floats
        const double r = (double)0.1f, off = 0.5 * (L * r) - 0.5 * r, lo = (0.0 + off) + r * (double)(-31), hi = (0.0 + off) + r * (double)(-0);
        CHECK(b.min_x == (double)(float)lo && b.min_y == b.min_x && b.max_x == (double)(float)hi && b.max_y == b.max_x);
        Costmap::Bounds bv{1e30, 1e30, -1e30, -1e30};
        visual.markVisual(0.5, &bv);
        CHECK(expected(visual.read(0, 0, 8, 8), 0));
        CHECK(bv.min_x == lo && bv.max_x == hi && bv.min_y == bv.min_x && bv.max_y == bv.max_x);   // doubles here
        // three records in costmap cell (3, 4): lethal, free, lethal -> the last decides; one outside is skipped
        gem::PointXYZRGBICT p{};
        p.x = -0.3f; p.y = 0.1f; p.travers = 0.2f;
        gem::PointXYZRGBICT q = p; q.x = -0.25f; q.travers = 0.8f;
        gem::PointXYZRGBICT out = p; out.x = 1.7f;
        Costmap::Bounds bp{1e30, 1e30, -1e30, -1e30};
        visual.resetMaps();
        visual.markPoints({p, q, p, out}, 0.5, &bp);
        std::vector<unsigned char> g = visual.read(0, 0, 8, 8);
        CHECK(g[4 * 8 + 3] == Costmap::LETHAL_OBSTACLE && bp.min_x == (double)-0.3f && bp.max_x == (double)-0.25f && bp.max_y == (double)0.1f);
        g[4 * 8 + 3] = Costmap::NO_INFORMATION;
        CHECK(g == std::vector<unsigned char>(64, Costmap::NO_INFORMATION));
        // a roll of 1.5 cells in x moves one cell; the origin follows by whole cells
        layer.updateOrigin(-1.6 + 1.5 * 0.4, -1.6 - 0.9 * 0.4);
        const gem_costmap_config c = layer.geometry();
        CHECK(c.origin_x == -1.6 + 1 * 0.4 && c.origin_y == -1.6 && c.size_x == 8 && c.default_value == Costmap::NO_INFORMATION);
        CHECK(expected(layer.read(0, 0, 8, 8), 1));
        // merged by max onto a free master: the lethal cells arrive, NO_INFORMATION does not
        layer.merge(master, 0, 0, 8, 8, Costmap::Max);
        const std::vector<unsigned char> m = master.read(6, 0, 8, 2);
        CHECK((m == std::vector<unsigned char>{Costmap::LETHAL_OBSTACLE, Costmap::FREE_SPACE, Costmap::LETHAL_OBSTACLE, Costmap::FREE_SPACE}));
        threw = false;
        try { layer.read(0, 0, 9, 8); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
    }
    bool threw = false;                                        // ~Costmap gave the ids back
    try { gem_costmap_config c{}; map.check(gem_costmap_geometry(map.handle(), 0, &c), "gem_costmap_geometry"); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
    CHECK(threw);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
