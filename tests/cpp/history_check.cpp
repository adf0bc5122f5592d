// The history side of the C++ facade (gem.hpp): gem::History over an ElevationMap and gem::Costmap::markHistory.  Without a GPU ("0")
// it only shows that the facade compiles and links; with one ("1") it runs against hand-derived answers.  An 8 x 8 costmap at 0.5 m
// with origin (0, 0) covers [0, 4) x [0, 4).  The history is three appends:
//   A  4096 records at (1.25, 1.25), lethal                   block 0, inside
//   B  4096 records at (100, 100), free                       block 1, far outside: culled
//   C  one record at (1.25, 1.25), free, one at (3.75, 0.25), lethal      block 2, partial
// so cell (2, 2) ends FREE (C's record is the last of its cell), cell (7, 0) LETHAL, everything else NO_INFORMATION, and the touched
// bounds are [1.25, 0.25, 3.75, 1.25].
#include "gem/gem.hpp"
#include "gem_hip_debug.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::Costmap;

static gem::PointXYZRGBICT record(float x, float y, float travers)
{
    gem::PointXYZRGBICT p{};
    p.x = x; p.y = y; p.travers = travers;
    return p;
}

static long long debug_get(gem::ElevationMap& map, const char* key)
{
    long long v = -1;
    map.check(gem_debug_get(map.handle(), key, &v), key);
    return v;
}

int main(int argc, char** argv)
{
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf("OK (no GPU: built)\n");
        return 0;
    }
    gem::ElevationMap map(32, 0.1f);
    {
        Costmap layer(map, 8, 8, 0.5), other(map, 8, 8, 0.5);
        bool threw = false;
        try { layer.markHistory(0.5); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                          // no history yet
        gem::History history(map, 64);                         // grows twice below
        CHECK(history.size() == 0 && history.exportCloud().empty());
        const std::vector<gem::PointXYZRGBICT> a(4096, record(1.25f, 1.25f, 0.1f)), b(4096, record(100.f, 100.f, 0.9f));
        const std::vector<gem::PointXYZRGBICT> c{record(1.25f, 1.25f, 0.9f), record(3.75f, 0.25f, 0.1f)};
        history.append(a);
        history.append(b);
        history.append(c);
        history.append({});
        CHECK(history.size() == 8194);
        const std::vector<gem::PointXYZRGBICT> all = history.exportCloud();
        CHECK(all.size() == 8194 && all[0].x == 1.25f && all[4096].x == 100.f && all[8193].x == 3.75f && all[8192].travers == 0.9f);
        for (int cull = 1; cull >= 0; --cull) {
            map.check(gem_debug_set(map.handle(), "history_cull", cull), "history_cull");
            layer.resetMaps();
            Costmap::Bounds bd{1e30, 1e30, -1e30, -1e30};
            layer.markHistory(0.5, &bd);
            std::vector<unsigned char> g = layer.read(0, 0, 8, 8);
            CHECK(g.size() == 64 && g[2 * 8 + 2] == Costmap::FREE_SPACE && g[0 * 8 + 7] == Costmap::LETHAL_OBSTACLE);
            g[2 * 8 + 2] = g[0 * 8 + 7] = Costmap::NO_INFORMATION;
            CHECK(g == std::vector<unsigned char>(64, Costmap::NO_INFORMATION));
            CHECK(bd.min_x == 1.25 && bd.min_y == 0.25 && bd.max_x == 3.75 && bd.max_y == 1.25);
            CHECK(debug_get(map, "history_blocks") == 3 && debug_get(map, "history_blocks_culled") == (cull ? 1 : 0));
        }
        other.markPoints(all, 0.5);                             // the independent path: the exported cloud as a caller's
        CHECK(other.read(0, 0, 8, 8) == layer.read(0, 0, 8, 8));
        threw = false;
        try { history.exportCloud(true); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                          // no capture
        threw = false;
        try { history.resetFromGlobal(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw && history.size() == 8194);                // no submap stack
        {
            gem::GlobalMap stack(map, 64);
            stack.push(c);
            stack.push(a);
            history.resetFromGlobal();
            CHECK(history.size() == 4098);
            const std::vector<gem::PointXYZRGBICT> r = history.exportCloud();
            CHECK(r.size() == 4098 && r[1].x == 3.75f && r[2].travers == 0.1f);
        }
        history.clear();
        CHECK(history.size() == 0);
    }
    bool threw = false;                                        // ~History switched it off
    try { long long n = 0; map.check(gem_history_size(map.handle(), &n), "gem_history_size"); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
    CHECK(threw);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
