// The VoxelGrid side of the C++ facade (gem.hpp): the launch-file presets as stages (pure host) and, with a GPU, filterDevice /
// addTo / addToDevice on a random cloud: addTo gives the map of gem_add on the centroids filterDevice returned.
#include "gem/gem.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static gem_frame_params laser_frame()
{
    gem_frame_params p;
    std::memset(&p, 0, sizeof(p));
    for (int i = 0; i < 4; ++i) p.T[i * 5] = 1.0f;
    p.T[11] = 1.0f;                                            // sensor 1 m above the map
    p.lower = -100.0; p.upper = 100.0;
    p.sensor_model = GEM_MODEL_LASER;
    p.sensor_params[0] = 0.0; p.sensor_params[1] = 0.0006; p.sensor_params[2] = 0.0015;
    return p;
}

int main()
{
    const gem::VoxelGrid kitti = gem::VoxelGrid::filterKittiLaunch();
    CHECK(kitti.stages().size() == 3);
    CHECK(kitti.stages()[1].field == GEM_VOXEL_FIELD_Z && kitti.stages()[1].limit_max == 25.0 && kitti.stages()[0].leaf[2] == 0.2f);
    const gem::VoxelGrid one = gem::VoxelGrid::filterLaunch();
    CHECK(one.stages().size() == 1 && one.stages()[0].field == GEM_VOXEL_FIELD_X && one.stages()[0].limit_min == -10.0);
    bool threw = false;
    try { gem::VoxelGrid v; v.setFilterFieldName("rgb"); } catch (const gem::Error&) { threw = true; }
    CHECK(threw);

    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0) {
        std::printf("no device: host checks only\n%s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    const int n = 50000;
    std::mt19937 rng(7);
    std::normal_distribution<float> xy(0.0f, 6.0f), z(0.0f, 0.3f);
    std::uniform_real_distribution<float> in(1.0f, 255.0f);
    std::vector<float> cloud(4 * (size_t)n);
    for (int i = 0; i < n; ++i) { cloud[4 * i] = xy(rng); cloud[4 * i + 1] = xy(rng); cloud[4 * i + 2] = z(rng) - 1.0f; cloud[4 * i + 3] = in(rng); }
    void *d_in = nullptr, *d_out = nullptr, *d_cnt = nullptr;
    CHECK(hipMalloc(&d_in, cloud.size() * 4) == hipSuccess && hipMalloc(&d_out, cloud.size() * 4) == hipSuccess && hipMalloc(&d_cnt, 4) == hipSuccess);
    CHECK(hipMemcpy(d_in, cloud.data(), cloud.size() * 4, hipMemcpyHostToDevice) == hipSuccess);
    gem::ElevationMap filtered(200, 0.1f), plain(200, 0.1f), device(200, 0.1f);
    kitti.filterDevice(filtered, d_in, n, d_out, d_cnt);
    filtered.synchronize();
    int m = -1;
    std::vector<float> cent(cloud.size());
    CHECK(hipMemcpy(&m, d_cnt, 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(cent.data(), d_out, cent.size() * 4, hipMemcpyDeviceToHost) == hipSuccess);
    std::printf("filterDevice: %d of %d points\n", m, n);
    CHECK(m > 0 && m < n);
    for (int i = m; i < n && i < m + 100; ++i) CHECK(std::isnan(cent[4 * i]) && cent[4 * i + 3] == 0.0f);
    const gem_frame_params f = laser_frame();
    kitti.addTo(filtered, f, cloud.data(), n);
    kitti.addToDevice(device, f, d_in, n);
    plain.add(f, cent.data(), m);
    const std::vector<float> a = filtered.layer(GEM_LAYER_ELEVATION), b = plain.layer(GEM_LAYER_ELEVATION), c = device.layer(GEM_LAYER_ELEVATION);
    CHECK(a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0 && std::memcmp(c.data(), b.data(), c.size() * 4) == 0);
    int touched = 0;
    for (float v : b) touched += v != -10.0f;
    CHECK(touched > 1000);
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_cnt);
    std::printf("%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
