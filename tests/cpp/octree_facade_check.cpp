// gem::LocalMap::compose_octrees / build_octree of the C++ facade (gem.hpp).  Without a GPU ("0") it only has to build; with one ("1"):
//   1. one point gives 17 nodes (136 bytes), every one with the point's colour and value (float)log(0.7 / 0.3), the root's mask 1 << 7;
//   2. eight points, one per leaf of a 2 x 2 x 2 block, collapse to one childless node at depth 15: 16 nodes, pruned_leaves 1;
//   3. compose_octrees on a flat map returns compose()'s counts and threshold, and each tree equals build_octree of compose()'s list;
//   4. compose_octrees before keepPrevious is GEM_ERR_INVALID.
#include "gem/gem.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static gem::PointXYZRGBICT point(float x, float y, float z, int r, int g, int b)
{
    gem::PointXYZRGBICT p{};
    p.x = x; p.y = y; p.z = z; p.pad = 1.0f;
    p.r = (std::uint8_t)r; p.g = (std::uint8_t)g; p.b = (std::uint8_t)b;
    return p;
}

int main(int argc, char** argv)
{
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        gem_octree_params q{};
        q.resolution = 0.1;
        gem::ColorOcTreeData t;
        std::printf("OK (no GPU: built)\n");
        return q.resolution == 0.1 && std::strcmp(t.id(), "ColorOcTree") == 0 ? 0 : 1;
    }
    const int L = 32;
    gem::ElevationMap map(L, 0.1f);
    gem::LocalMap local(map, 4);
    const float hit = (float)std::log(0.7 / 0.3);
    {
        gem::ColorOcTreeData t = local.build_octree({point(0.05f, 0.05f, 0.05f, 10, 20, 30)}, 0.1);
        CHECK(t.data.size() == 136 && t.stats.nodes == 17 && t.stats.leaves_depth16 == 1);
        bool same = t.data.size() == 136;
        for (size_t n = 0; same && n < 17; ++n) {
            float v; std::memcpy(&v, &t.data[8 * n], 4);
            const std::uint8_t* c = reinterpret_cast<const std::uint8_t*>(&t.data[8 * n + 4]);
            same = v == hit && c[0] == 10 && c[1] == 20 && c[2] == 30 && c[3] == (n == 0 ? 128 : (n == 16 ? 0 : 1));
        }
        CHECK(same);
    }
    {
        std::vector<gem::PointXYZRGBICT> c;
        for (int i = 0; i < 8; ++i) c.push_back(point(0.1f * (i & 1) + 0.05f, 0.1f * ((i >> 1) & 1) + 0.05f, 0.1f * ((i >> 2) & 1) + 0.05f, 10 * (i + 1), 100, 200));
        gem::ColorOcTreeData t = local.build_octree(c, 0.1, GEM_OCTREE_USER1);
        CHECK(t.stats.nodes == 16 && t.stats.pruned_leaves == 1 && t.stats.leaves_depth16 == 0 && t.stats.coupled_blocks[0] == 1);
        CHECK(t.data.size() == 128 && t.data[127] == 0);
    }
    std::vector<float> elev(L * L, 0.25f), trav(L * L, 0.5f), var(L * L, 0.01f);
    for (int k = 0; k < 5; ++k) trav[(3 + 5 * k) * L + 7] = -0.5f;
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_ELEVATION, elev.data()) == GEM_OK);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_TRAVER, trav.data()) == GEM_OK);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_VARIANCE, var.data()) == GEM_OK);
    local.capture();
    bool threw = false;
    try { local.compose_octrees(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
    CHECK(threw);
    local.keepPrevious();
    gem::LocalMap::Composed c = local.compose(20, 1e6, 0.0);
    gem::LocalMap::ComposedOcTrees o = local.compose_octrees(0.2, 0.1, 20, 1e6, 0.0);
    std::printf("flat: road %d obstacle %d removed %d | road tree %zu bytes, obstacle tree %zu bytes\n", o.roadPoints, o.obstaclePoints, o.removed,
                o.road.data.size(), o.obstacle.data.size());
    CHECK(o.roadPoints == (int)c.road.size() && o.obstaclePoints == (int)c.obstacle.size() && o.removed == c.removed);
    CHECK(std::memcmp(&o.threshold, &c.threshold, sizeof(double)) == 0);
    CHECK(o.road.resolution == 0.2 && o.obstacle.resolution == 0.1 && !o.road.data.empty() && !o.obstacle.data.empty());
    CHECK(o.road.data == local.build_octree(c.road, 0.2).data);
    CHECK(o.obstacle.data == local.build_octree(c.obstacle, 0.1).data);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
