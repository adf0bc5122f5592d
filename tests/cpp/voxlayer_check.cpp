// The VoxelLayer side of the C++ facade (gem.hpp): gem::VoxelConfig and gem::Costmap::attachVoxels / voxelObserve / readVoxels, and the
// host twin gem_voxlayer_host.  Builds with a plain C++ compiler against the installed headers and the library.
//   voxlayer_check 0             no GPU: the host twin against hand-derived answers; shows that the facade compiles and links
//   voxlayer_check 1             the same answers from gem::Costmap::voxelObserve on the device
//   voxlayer_check host IN OUT   the host twin on the cases of a file (tests/test_voxlayer_cpu.py writes it and compares)
// The hand-derived case: an 8 x 8 costmap at 0.5 m with origin (0, 0), every cell 10, every column unknown, ten voxels of 0.2 m from
// z = 0, thresholds (15, 0); the sensor at (0.25, 0.25, 0.5) in voxel (0, 0, 2), costmap_2d's default ranges (obstacle 2.5, raytrace
// 3.0 = 6 cells).  Every ray is shortened by 2 * resolution = 1 m.  Three returns at height 0.5:
//   (3.25, 0.25)  3 m away, shortened to x = 2.25 in cell 4: voxel 2 of the cells 0 .. 4 of row 0 is cleared, 15 unknown voxels are
//                 not above the threshold, the cells become 0; beyond the obstacle range, not marked
//   (1.25, 0.25)  1 m away, shortened to the sensor itself: its ray is the sensor's voxel; marked: cell (2, 0), voxel 2, 254
//   (2.25, 2.25)  sqrt(8) m away, shortened to x = y = 1.54 in cell (3, 3): the diagonal (k, k), k = 0 .. 3; not marked
// and one at height 2.5, outside the buffer's window, which does nothing.
#include "gem/gem.hpp"

#include <cmath>
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

static std::vector<unsigned char> wanted_grid()
{
    std::vector<unsigned char> g(64, 10);
    for (int x = 0; x <= 4; ++x) g[x] = 0;
    for (int k = 0; k <= 3; ++k) g[k * 8 + k] = 0;
    g[2] = 254;
    return g;
}

static std::vector<unsigned> wanted_columns()
{
    std::vector<unsigned> c(64, 0xFFFFu);
    for (int x = 0; x <= 4; ++x) c[x] = 0xFFFBu;
    for (int k = 0; k <= 3; ++k) c[k * 8 + k] = 0xFFFBu;
    c[2] = 0x4FFFFu;
    return c;
}

// the point the third return's ray ends at, by the contract's own operations
static double diagonal_end()
{
    volatile double d = std::sqrt(8.0), f = (d - 2 * 0.5) / d, w = f * 2.0 + 0.25, a = w - 0.25, end = 0.25 + a * 1.0, dd = end - 0.25;
    return 0.25 + dd * 1.0;
}

template <class T>
static bool get(std::FILE* f, T* v, size_t n = 1) { return std::fread(v, sizeof(T), n, f) == n; }

// IN: int32 cases; per case uint32 size_x, size_y, double resolution, origin_x, origin_y, layer_max, uint32 size_z, double z_resolution,
// origin_z, uint32 unknown_threshold, mark_threshold, int32 n_obs, int32 has_bounds, double bounds[4], the grid, the columns, then per
// observation int64 n, uint32 step, flags, double origin[3], obstacle_range, raytrace_range, min_height, max_height and n * step bytes.
// OUT: per case int32 rc, the grid, the columns, double bounds[4].
static int run_file(const char* in, const char* out)
{
    std::FILE* f = std::fopen(in, "rb");
    std::FILE* o = std::fopen(out, "wb");
    if (!f || !o) return 2;
    int cases = 0;
    if (!get(f, &cases)) return 2;
    for (int c = 0; c < cases; ++c) {
        gem_costmap_config cfg{};
        gem_voxel_config vox{};
        double layer_max = 0.0, bounds[4];
        int n_obs = 0, has_bounds = 0;
        if (!get(f, &cfg.size_x) || !get(f, &cfg.size_y) || !get(f, &cfg.resolution) || !get(f, &cfg.origin_x) || !get(f, &cfg.origin_y) ||
            !get(f, &layer_max) || !get(f, &vox.size_z) || !get(f, &vox.z_resolution) || !get(f, &vox.origin_z) || !get(f, &vox.unknown_threshold) ||
            !get(f, &vox.mark_threshold) || !get(f, &n_obs) || !get(f, &has_bounds) || !get(f, bounds, 4) || n_obs < 0 || n_obs > 64)
            return 2;
        std::vector<unsigned char> grid(static_cast<size_t>(cfg.size_x) * cfg.size_y);
        std::vector<unsigned> columns(grid.size());
        if (!get(f, grid.data(), grid.size()) || !get(f, columns.data(), columns.size())) return 2;
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
        const int rc = gem_voxlayer_host(grid.data(), columns.data(), &cfg, &vox, obs.data(), n_obs, layer_max, has_bounds ? bounds : nullptr);
        std::fwrite(&rc, sizeof(rc), 1, o);
        std::fwrite(grid.data(), 1, grid.size(), o);
        std::fwrite(columns.data(), sizeof(unsigned), columns.size(), o);
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
    const gem::VoxelConfig vox;
    CHECK(vox.size_z == 10u && vox.z_resolution == 0.2 && vox.origin_z == 0.0 && vox.unknown_threshold == 15u && vox.mark_threshold == 0u);
    const double diag = diagonal_end();
    CHECK(diag > 1.54 && diag < 1.55);

    // the host twin
    gem_costmap_config cfg{};
    cfg.size_x = cfg.size_y = 8; cfg.resolution = 0.5;
    std::vector<unsigned char> g(64, 10);
    std::vector<unsigned> c(64, 0xFFFFu);
    double b[4] = {1e30, 1e30, -1e30, -1e30};
    CHECK(gem_voxlayer_host(g.data(), c.data(), &cfg, &vox, &seen, 1, 2.0, b) == GEM_OK);
    CHECK(g == wanted_grid());
    CHECK(c == wanted_columns());
    CHECK(b[0] == 0.25 && b[1] == 0.25 && b[2] == 2.25 && b[3] == diag);
    gem::Observation bad = seen;
    bad.flags = 4u;
    CHECK(gem_voxlayer_host(g.data(), c.data(), &cfg, &vox, &bad, 1, 2.0, b) == GEM_ERR_INVALID && g == wanted_grid() && c == wanted_columns());
    CHECK(gem_voxlayer_host(g.data(), nullptr, &cfg, &vox, &seen, 1, 2.0, b) == GEM_ERR_INVALID);
    gem::VoxelConfig tall(17);
    CHECK(gem_voxlayer_host(g.data(), c.data(), &cfg, &tall, &seen, 1, 2.0, b) == GEM_ERR_INVALID && g == wanted_grid() && c == wanted_columns());
    // the overhang: a column marked in voxel 6 keeps its cell lethal under a ray through voxel 2
    std::vector<unsigned char> g2(64, 10);
    std::vector<unsigned> c2(64, 0xFFFFu);
    g2[3] = 254; c2[3] = 0xFFFFu | (1u << 22);
    const gem::Observation clears(cloud, 0.25, 0.25, 0.5, false, true);
    CHECK(gem_voxlayer_host(g2.data(), c2.data(), &cfg, &vox, &clears, 1, 2.0, nullptr) == GEM_OK);
    CHECK(g2[3] == 254 && c2[3] == (0xFFFBu | (1u << 22)) && g2[2] == 0 && g2[4] == 0);

    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: built)\n");
        return fails ? 1 : 0;
    }
    gem::ElevationMap map(32, 0.1f);
    {
        gem::Costmap layer(map, 8, 8, 0.5);
        layer.write(0, 0, 8, 8, std::vector<unsigned char>(64, 10));
        bool threw = false;
        try { layer.voxelObserve({seen}); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                       // no voxels attached
        layer.attachVoxels(vox);
        CHECK(layer.readVoxels(0, 0, 8, 8) == std::vector<unsigned>(64, 0xFFFFu));
        threw = false;
        try { layer.attachVoxels(vox); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                       // attached twice
        gem::Costmap::Bounds bd{1e30, 1e30, -1e30, -1e30};
        layer.voxelObserve({seen}, 2.0, &bd);
        CHECK(layer.read(0, 0, 8, 8) == wanted_grid());
        CHECK(layer.readVoxels(0, 0, 8, 8) == wanted_columns());
        CHECK(bd.min_x == 0.25 && bd.min_y == 0.25 && bd.max_x == 2.25 && bd.max_y == diag);
        layer.voxelObserve({seen});                                         // only enqueued: the same answer
        CHECK(layer.read(0, 0, 8, 8) == wanted_grid() && layer.readVoxels(0, 0, 8, 8) == wanted_columns());
        layer.voxelObserve({});
        threw = false;
        try { layer.voxelObserve({bad}); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw && layer.read(0, 0, 8, 8) == wanted_grid());
        // the overhang on the device, and the 2-D layer on the same bytes
        layer.write(0, 0, 8, 8, g2 = [] { std::vector<unsigned char> v(64, 10); v[3] = 254; return v; }());
        layer.writeVoxels(0, 0, 8, 8, [] { std::vector<unsigned> v(64, 0xFFFFu); v[3] |= 1u << 22; return v; }());
        layer.voxelObserve({clears});
        CHECK(layer.read(0, 0, 8, 8)[3] == 254 && layer.readVoxels(3, 0, 4, 1)[0] == (0xFFFBu | (1u << 22)));
        layer.observe({clears});
        CHECK(layer.read(0, 0, 8, 8)[3] == 0);
        // resetMaps resets the columns; a plan made before an observation is stale after it
        layer.resetMaps();
        CHECK(layer.readVoxels(0, 0, 8, 8) == std::vector<unsigned>(64, 0xFFFFu));
        layer.write(0, 0, 8, 8, std::vector<unsigned char>(64, 10));
        layer.navPlan({0.25, 0.25}, {3.25, 3.25});
        CHECK(layer.potential().size() == 64u);
        layer.voxelObserve({seen});
        threw = false;
        try { layer.potential(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
