// The submap-stack side of the C++ facade (gem.hpp): gem::GlobalMap over an ElevationMap.  Without a GPU ("0") it only shows that
// the facade compiles and links; with one ("1") it runs pushLocal / push / loopClosure / exportCloud / size against hand-derived
// answers: L = 32, res = 0.1f, centre 0, start 0 -> cell x = 1.55 - 0.1 ix; the cell at (0.05, 0.05) and a record at (0.01, 0.01)
// both quantise to the key (0.05f, 0.05f) (0.05f / 0.1f = 0.5 and 0.01f / 0.1f = 0.1 both ceil to 1).  Three submaps with centres
// 1 m apart on a line give three lists of three entries, six pair steps, each of which fuses that key once.
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
        std::printf("OK (no GPU: built)\n");
        return 0;
    }
    const int L = 32;
    gem::ElevationMap map(L, 0.1f);
    std::vector<float> elev(L * L), trav(L * L, 0.5f), var(L * L, 0.01f);
    for (int i = 0; i < L * L; ++i) elev[i] = 0.001f * (float)i;
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_ELEVATION, elev.data()) == GEM_OK);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_TRAVER, trav.data()) == GEM_OK);
    CHECK(gem_set_layer(map.handle(), GEM_LAYER_VARIANCE, var.data()) == GEM_OK);
    {
        gem::LocalMap local(map, 4);
        gem::GlobalMap global(map, 16);
        bool threw = false;
        try { global.pushLocal(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                          // no capture yet
        CHECK(global.size() == 0);
        local.capture();
        CHECK(global.pushLocal(true) == 0);
        gem::PointXYZRGBICT p{};
        p.x = 0.01f; p.y = 0.01f; p.z = 2.0f; p.pad = 1.0f; p.r = 7; p.covariance = 0.5f; p.intensity = 3.0f; p.travers = 0.25f;
        CHECK(global.push({p}) == 1);
        CHECK(global.push({p}) == 2);
        CHECK(global.size() == 3 && global.exportCloud(0).size() == (size_t)(L * L) && global.exportCloud(-1).size() == (size_t)(L * L) + 2);
        std::array<float, 16> eye{};
        eye[0] = eye[5] = eye[10] = eye[15] = 1.0f;
        const long long fused = global.loopClosure({eye, eye, eye}, {{0.f, 0.f}, {1.f, 0.f}, {2.f, 0.f}});
        std::printf("loop closure: %lld fused\n", fused);
        CHECK(fused == 6);
        const std::vector<gem::PointXYZRGBICT> s1 = global.exportCloud(1);
        CHECK(s1.size() == 1 && s1[0].x == 0.05f && s1[0].y == 0.05f && s1[0].r == 7 && s1[0].a == 0 && s1[0].travers == 0.25f);
        CHECK(global.exportCloud(-1).size() == (size_t)(L * L) + 2);
        threw = false;
        try { global.exportCloud(3); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
    }
    bool threw = false;                                        // ~GlobalMap switched it off
    try { int n = 0; map.check(gem_global_count(map.handle(), &n), "gem_global_count"); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
    CHECK(threw);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
