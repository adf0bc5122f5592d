// The ObstacleLayer side of the C++ facade (gem.hpp): gem::Observation and gem::Costmap::observe, and the host twin gem_obstacle_host.
// Builds with a plain C++ compiler against the installed headers and the library.
//   obstacle_check 0             no GPU: the host twin against hand-derived answers; shows that the facade compiles and links
//   obstacle_check 1             the same answers from gem::Costmap::observe on the device
//   obstacle_check host IN OUT   the host twin on the cases of a file (tests/test_obstacle_cpu.py writes it and compares)
// The hand-derived case: an 8 x 8 costmap at 0.5 m with origin (0, 0), every cell 10, the sensor at (0.25, 0.25, 0.5) in cell (0, 0),
// costmap_2d's default ranges (obstacle 2.5, raytrace 3.0 = 6 cells).  Three returns at height 0.5:
//   (3.25, 0.25)  cell (6, 0): row 0 is cleared up to x = 6; 3 m away, beyond the obstacle range, not marked
//   (1.25, 0.25)  cell (2, 0): marked
//   (2.25, 2.25)  cell (4, 4): the diagonal (k, k), k = 0 .. 4 (sqrt(32) cells < 6); sqrt(8) m away, not marked
// and one at height 2.5, outside the buffer's window, which does nothing.  Bounds: [0.25, 0.25, 3.25, 2.25].
#include "gem/gem.hpp"
#include "gem_hip_debug.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static gem::PointXYZRGBICT point(float x, float y, float z)
{
    gem::PointXYZRGBICT p{};
    p.x = x; p.y = y; p.z = z;
    return p;
}

static std::vector<unsigned char> wanted()
{
    std::vector<unsigned char> g(64, 10);
    for (int x = 0; x <= 6; ++x) g[x] = 0;
    for (int k = 0; k <= 4; ++k) g[k * 8 + k] = 0;
    g[2] = 254;
    return g;
}

template <class T>
static bool get(std::FILE* f, T* v, size_t n = 1) { return std::fread(v, sizeof(T), n, f) == n; }

// IN: int32 cases; per case uint32 size_x, size_y, double resolution, origin_x, origin_y, layer_max, int32 n_obs, int32 has_bounds,
// double bounds[4], the grid, then per observation int64 n, uint32 step, flags, double origin[3], obstacle_range, raytrace_range,
// min_height, max_height and n * step bytes.  OUT: per case int32 rc, the grid, double bounds[4].
static int run_file(const char* in, const char* out)
{
    std::FILE* f = std::fopen(in, "rb");
    std::FILE* o = std::fopen(out, "wb");
    if (!f || !o) return 2;
    int cases = 0;
    if (!get(f, &cases)) return 2;
    for (int c = 0; c < cases; ++c) {
        gem_costmap_config cfg{};
        double layer_max = 0.0, bounds[4];
        int n_obs = 0, has_bounds = 0;
        if (!get(f, &cfg.size_x) || !get(f, &cfg.size_y) || !get(f, &cfg.resolution) || !get(f, &cfg.origin_x) || !get(f, &cfg.origin_y) ||
            !get(f, &layer_max) || !get(f, &n_obs) || !get(f, &has_bounds) || !get(f, bounds, 4) || n_obs < 0 || n_obs > 64)
            return 2;
        std::vector<unsigned char> grid(static_cast<size_t>(cfg.size_x) * cfg.size_y);
        if (!get(f, grid.data(), grid.size())) return 2;
        std::vector<gem_observation> obs(static_cast<size_t>(n_obs));
        std::vector<std::vector<unsigned char>> clouds(static_cast<size_t>(n_obs));
        for (int k = 0; k < n_obs; ++k) {
            gem_observation& b = obs[static_cast<size_t>(k)];
            if (!get(f, &b.n) || !get(f, &b.point_step) || !get(f, &b.flags) || !get(f, b.origin, 3) || !get(f, &b.obstacle_range) ||
                !get(f, &b.raytrace_range) || !get(f, &b.min_obstacle_height) || !get(f, &b.max_obstacle_height) || b.n < 0)
                return 2;
            clouds[static_cast<size_t>(k)].resize(static_cast<size_t>(b.n) * b.point_step);
            if (!get(f, clouds[static_cast<size_t>(k)].data(), clouds[static_cast<size_t>(k)].size())) return 2;
            b.points = b.n ? clouds[static_cast<size_t>(k)].data() : nullptr;
        }
        const int rc = gem_obstacle_host(grid.data(), &cfg, obs.data(), n_obs, layer_max, has_bounds ? bounds : nullptr);
        std::fwrite(&rc, sizeof(rc), 1, o);
        std::fwrite(grid.data(), 1, grid.size(), o);
        std::fwrite(bounds, sizeof(double), 4, o);
    }
    std::fclose(f);
    return std::fclose(o) == 0 ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc == 4 && std::strcmp(argv[1], "host") == 0) return run_file(argv[2], argv[3]);

    const std::vector<gem::PointXYZRGBICT> cloud{point(3.25f, 0.25f, 0.5f), point(1.25f, 0.25f, 0.5f), point(2.25f, 2.25f, 0.5f), point(1.75f, 3.25f, 2.5f)};
    const gem::Observation seen(cloud, 0.25, 0.25, 0.5);
    CHECK(seen.n == 4 && seen.point_step == 32u && seen.flags == (GEM_OBS_MARKING | GEM_OBS_CLEARING) && seen.raytrace_range == 3.0);

    // the host twin
    gem_costmap_config cfg{};
    cfg.size_x = cfg.size_y = 8; cfg.resolution = 0.5;
    std::vector<unsigned char> g(64, 10);
    double b[4] = {1e30, 1e30, -1e30, -1e30};
    CHECK(gem_obstacle_host(g.data(), &cfg, &seen, 1, 2.0, b) == GEM_OK);
    CHECK(g == wanted());
    CHECK(b[0] == 0.25 && b[1] == 0.25 && b[2] == 3.25 && b[3] == 2.25);
    gem::Observation bad = seen;
    bad.flags = 4u;
    CHECK(gem_obstacle_host(g.data(), &cfg, &bad, 1, 2.0, b) == GEM_ERR_INVALID && g == wanted());
    // marking alone clears nothing; clearing alone marks nothing
    std::vector<unsigned char> g2(64, 10), want2(64, 10);
    const gem::Observation marks(cloud, 0.25, 0.25, 0.5, true, false), clears(cloud, 0.25, 0.25, 0.5, false, true);
    want2[2] = 254;
    CHECK(gem_obstacle_host(g2.data(), &cfg, &marks, 1, 2.0, nullptr) == GEM_OK && g2 == want2);
    std::vector<unsigned char> want3 = wanted();
    want3[2] = 0;
    g2.assign(64, 10);
    CHECK(gem_obstacle_host(g2.data(), &cfg, &clears, 1, 2.0, nullptr) == GEM_OK && g2 == want3);

    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: built)\n");
        return fails ? 1 : 0;
    }
    gem::ElevationMap map(32, 0.1f);
    for (int direct = 0; direct < 2; ++direct) {
        map.check(gem_debug_set(map.handle(), "obstacle_direct", direct), "obstacle_direct");
        gem::Costmap layer(map, 8, 8, 0.5);
        layer.write(0, 0, 8, 8, std::vector<unsigned char>(64, 10));
        gem::Costmap::Bounds bd{1e30, 1e30, -1e30, -1e30};
        layer.observe({seen}, 2.0, &bd);
        CHECK(layer.read(0, 0, 8, 8) == wanted());
        CHECK(bd.min_x == 0.25 && bd.min_y == 0.25 && bd.max_x == 3.25 && bd.max_y == 2.25);
        layer.observe({clears, marks});                                     // two observations, only enqueued: the same answer
        CHECK(layer.read(0, 0, 8, 8) == wanted());
        layer.observe({});
        bool threw = false;
        try { layer.observe({bad}); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw && layer.read(0, 0, 8, 8) == wanted());
        // a plan made before an observation is stale after it
        layer.navPlan({0.25, 0.25}, {3.25, 3.25});
        CHECK(layer.potential().size() == 64u);
        layer.observe({seen});
        threw = false;
        try { layer.potential(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
