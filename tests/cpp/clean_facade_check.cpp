// The raw-cloud side of the C++ facade (gem.hpp): SensorProcessorBase::cleanParams per processor (pure host: no device needed) and,
// with a GPU, processRaw of the structured-light and the stereo processors on an organised cloud with NaN holes and depths outside
// the cutoffs, against a host-side clean followed by gem_process_points on the kept points with their indices.
#include "gem/gem.hpp"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Cleaned { std::vector<float> x, y, z; std::vector<int> orig; };

static Cleaned clean_on_host(const std::vector<gem::PointXYZRGBICT>& c, const gem_clean_params& p)
{
    Cleaned r;
    for (size_t i = 0; i < c.size(); ++i) {
        const float x = c[i].x, y = c[i].y, z = c[i].z;
        bool keep = std::isfinite(x) && std::isfinite(y) && std::isfinite(z);
        if (p.mode == GEM_CLEAN_PASSTHROUGH_Z) keep = keep && z >= p.z_min && z <= p.z_max;
        if (p.mode == GEM_CLEAN_NONE) keep = true;
        if (keep) { r.x.push_back(x); r.y.push_back(y); r.z.push_back(z); r.orig.push_back((int)i); }
    }
    return r;
}

// processRaw of `sp` against the host clean + gem_process_points with the kept indices
static void check_process_raw(gem::SensorProcessorBase& sp, gem::ElevationMap& map, const std::vector<gem::PointXYZRGBICT>& cloud, int width)
{
    const int n = (int)cloud.size();
    std::vector<int> R(n, -7), G(n, -7), B(n, -7), idx(n, -7);
    std::vector<float> I(n, -7.f), hgt(n, -7.f), var(n, -7.f);
    const int kept = sp.processRaw(map, cloud.data(), n, width, R.data(), G.data(), B.data(), idx.data(), I.data(), hgt.data(), var.data());
    const Cleaned c = clean_on_host(cloud, sp.cleanParams());
    std::printf("processRaw: %d of %d kept (host clean: %zu)\n", kept, n, c.orig.size());
    CHECK(kept == (int)c.orig.size());
    CHECK(kept > 0 && kept < n);
    if (kept != (int)c.orig.size()) return;
    const gem_frame_params p = sp.frameParams();
    CHECK(p.original_width == width);
    std::vector<int> e_idx(kept); std::vector<float> e_var(kept), e_h(kept);
    std::vector<float> x = c.x, y = c.y, z = c.z;
    CHECK(gem_process_points(map.handle(), &p, kept, x.data(), y.data(), z.data(), c.orig.data(), 0, e_idx.data(), e_var.data(), nullptr, nullptr,
                             e_h.data()) == GEM_OK);
    int bad = 0, inside = 0;
    for (int k = 0; k < kept; ++k) {
        const gem::PointXYZRGBICT& q = cloud[c.orig[k]];
        bad += idx[k] != e_idx[k] || std::memcmp(&var[k], &e_var[k], 4) != 0 || std::memcmp(&hgt[k], &e_h[k], 4) != 0;
        bad += R[k] != q.r || G[k] != q.g || B[k] != q.b || std::memcmp(&I[k], &q.intensity, 4) != 0;
        inside += idx[k] >= 0;
    }
    std::printf("  %d mismatches, %d kept points inside the map\n", bad, inside);
    CHECK(bad == 0);
    CHECK(inside > kept / 4);
    for (int k = kept; k < n; ++k) CHECK(idx[k] == -7 && R[k] == -7);          // nothing written past the kept points
}

int main(int argc, char** argv)
{
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;

    gem::LaserSensorProcessor laser; gem::StereoSensorProcessor stereo; gem::PerfectSensorProcessor perfect;
    gem::StructuredLightSensorProcessor sl;
    for (gem::SensorProcessorBase* s : {(gem::SensorProcessorBase*)&laser, (gem::SensorProcessorBase*)&stereo, (gem::SensorProcessorBase*)&perfect})
        CHECK(s->cleanParams().mode == GEM_CLEAN_REMOVE_NAN);
    // structured light, the reference's defaults: numeric_limits<double>::min() -> +0.0f, ::max() -> +inf
    gem_clean_params d = sl.cleanParams();
    CHECK(d.mode == GEM_CLEAN_PASSTHROUGH_Z && d.z_min == 0.0f && !std::signbit(d.z_min) && std::isinf(d.z_max) && d.z_max > 0);
    // realsense_d435.yaml
    sl.sensorParameters()["cutoff_min_depth"] = 0.2;
    sl.sensorParameters()["cutoff_max_depth"] = 3.25;
    d = sl.cleanParams();
    CHECK(d.mode == GEM_CLEAN_PASSTHROUGH_Z && d.z_min == 0.2f && d.z_max == 3.25f);

    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: cleanParams)\n");
        return fails;
    }

    // an organised 64 x 48 depth image seen from 0.6 m, pitched down: NaN holes (every 7th pixel, one whole row), one +inf, depths
    // beyond the d435 cutoffs at the top of the image; colours encode the pixel so the kept points' fields can be told apart
    const int W = 64, H = 48;
    std::vector<gem::PointXYZRGBICT> cloud(W * H);
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            const int i = v * W + u;
            gem::PointXYZRGBICT& q = cloud[i];
            const float depth = 0.15f + 0.08f * (float)(H - v);                   // 0.23 .. 3.99 m
            q.x = (u - W / 2) * depth / 60.f; q.y = (v - H / 2) * depth / 60.f; q.z = depth;
            q.r = (std::uint8_t)(i & 255); q.g = (std::uint8_t)(i >> 8); q.b = (std::uint8_t)(u * 3); q.a = 255;
            q.intensity = (float)(i % 97); q.pad = 1.f; q.covariance = 0.f; q.travers = 0.f;
            if (i % 7 == 3 || v == 20) q.x = q.y = q.z = NAN;
            if (i == 100) q.z = INFINITY;
        }
    gem::ElevationMap map(200, 0.05f);
    const float pos[3] = {1.0f, 0.0f, 0.0f};
    map.move(pos);
    const gem::Mat4 T{0, 0, 1, 0,  -1, 0, 0, 0,  0, -1, 0, 0.6,  0, 0, 0, 1};   // optical (x right, y down, z forward) -> map
    const gem::Mat4 I4{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    sl.sensorParameters()["normal_factor_a"] = 0.000611; sl.sensorParameters()["normal_factor_b"] = 0.003587;
    sl.sensorParameters()["normal_factor_c"] = 0.3515; sl.sensorParameters()["normal_factor_e"] = 1.0;
    sl.sensorParameters()["lateral_factor"] = 0.01576;
    sl.updateTransformations(T, T, I4);
    sl.setRejectFilter(gem_reject_filter{0, 1.5f, 1.5f, 1.0f, 0.0f});
    check_process_raw(sl, map, cloud, W);

    for (const char* k : {"p_1", "p_2", "p_3", "p_4", "p_5", "lateral_factor", "depth_to_disparity_factor"}) stereo.sensorParameters()[k] = 0.0;
    stereo.sensorParameters()["p_1"] = 0.1; stereo.sensorParameters()["p_2"] = 0.001; stereo.sensorParameters()["p_3"] = 380.0;
    stereo.sensorParameters()["p_4"] = 1.0; stereo.sensorParameters()["p_5"] = 0.002; stereo.sensorParameters()["lateral_factor"] = 0.001;
    stereo.sensorParameters()["depth_to_disparity_factor"] = 30.0;
    stereo.updateTransformations(T, T, I4);
    stereo.setRejectFilter(gem_reject_filter{0, 1.5f, 1.5f, 1.0f, 0.0f});
    check_process_raw(stereo, map, cloud, W);

    std::printf(fails ? "FAILED\n" : "OK\n");
    return fails;
}
