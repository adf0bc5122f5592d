// The depth-image side of the C++ facade (gem.hpp): gem_depth_constants (pure host: no device needed) and, with a GPU,
// SensorProcessorBase::addDepth of the structured-light and the stereo processors on a 64 x 48 uint16 image with holes and a BGR8 colour
// image, against ElevationMap::addRaw of the cloud this program unprojects itself with the same three float operations per coordinate
// (compile with -ffp-contract=off).
#include "gem/gem.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static void check_add_depth(gem::SensorProcessorBase& sp, const gem::DepthImage& img, const std::vector<std::uint16_t>& depth,
                            const std::vector<std::uint8_t>& bgr, const std::vector<float>& xyzi, const std::vector<std::uint32_t>& rgb)
{
    gem::ElevationMap a(200, 0.05f), b(200, 0.05f);
    const float pos[3] = {1.0f, 0.0f, 0.0f};
    a.move(pos); b.move(pos);
    for (int frame = 0; frame < 2; ++frame) {
        sp.addDepth(a, img, depth.data(), bgr.data());
        const gem_frame_params p = sp.frameParams();
        CHECK(p.original_width == img.width);
        b.addRaw(p, sp.cleanParams(), xyzi.data(), img.width * img.height, rgb.data());
    }
    long long seen = 0;
    for (int l = GEM_LAYER_ELEVATION; l <= GEM_LAYER_SLOPE; ++l) {
        if (l >= GEM_LAYER_COLOR_R && l <= GEM_LAYER_COLOR_B) {
            const std::vector<int> x = a.colorLayer(l), y = b.colorLayer(l);
            CHECK(x == y);
        } else {
            const std::vector<float> x = a.layer(l), y = b.layer(l);
            CHECK(std::memcmp(x.data(), y.data(), x.size() * sizeof(float)) == 0);
            if (l == GEM_LAYER_ELEVATION) for (float e : x) seen += e != -10.f;
        }
    }
    std::printf("addDepth: %lld cells seen\n", seen);
    CHECK(seen > 500);
}

int main(int argc, char** argv)
{
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;

    const int W = 64, H = 48;
    gem::DepthImage img{};
    img.width = W; img.height = H; img.format = GEM_DEPTH_U16;
    img.fx = 60.0; img.fy = 61.5; img.cx = 31.5; img.cy = 23.25;
    img.depth_unit = 0.f; img.intensity = 42.f; img.color_format = GEM_COLOR_BGR8;
    float k[4] = {0, 0, 0, 0};
    CHECK(gem_depth_constants(&img, k) == GEM_OK);
    CHECK(k[0] == (float)((double)0.001f / 60.0) && k[1] == (float)((double)0.001f / 61.5) && k[2] == 31.5f && k[3] == 23.25f);
    gem::DepthImage bad = img; bad.fx = 0.0;
    CHECK(gem_depth_constants(&bad, k) == GEM_ERR_INVALID);
    CHECK(gem_depth_constants(nullptr, k) == GEM_ERR_INVALID);

    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: constants)\n");
        return fails;
    }

    // seen from 0.6 m: depths 0.23 .. 3.99 m in millimetres (beyond the d435 cutoffs at the top), holes every 7th pixel and one row
    std::vector<std::uint16_t> depth(W * H);
    std::vector<std::uint8_t> bgr(W * H * 3);
    std::vector<float> xyzi(W * H * 4);
    std::vector<std::uint32_t> rgb(W * H);
    const float unit = 0.001f;
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            const int i = v * W + u;
            std::uint16_t d = (std::uint16_t)(150 + 80 * (H - v) + (u % 5));
            if (i % 7 == 3 || v == 20) d = 0;
            depth[i] = d;
            bgr[3 * i] = (std::uint8_t)(u * 3); bgr[3 * i + 1] = (std::uint8_t)(i >> 8); bgr[3 * i + 2] = (std::uint8_t)(i & 255);
            rgb[i] = ((std::uint32_t)bgr[3 * i + 2] << 16) | ((std::uint32_t)bgr[3 * i + 1] << 8) | bgr[3 * i];
            const float df = (float)d;
            float t = (float)u - k[2]; t = t * df; const float x = t * k[0];
            float s = (float)v - k[3]; s = s * df; const float y = s * k[1];
            const float z = df * unit;
            xyzi[4 * i] = d ? x : NAN; xyzi[4 * i + 1] = d ? y : NAN; xyzi[4 * i + 2] = d ? z : NAN; xyzi[4 * i + 3] = img.intensity;
        }

    const gem::Mat4 T{0, 0, 1, 0,  -1, 0, 0, 0,  0, -1, 0, 0.6,  0, 0, 0, 1};   // optical (x right, y down, z forward) -> map
    const gem::Mat4 I4{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    gem::StructuredLightSensorProcessor sl;
    sl.sensorParameters()["cutoff_min_depth"] = 0.2; sl.sensorParameters()["cutoff_max_depth"] = 3.25;
    sl.sensorParameters()["normal_factor_a"] = 0.000611; sl.sensorParameters()["normal_factor_b"] = 0.003587;
    sl.sensorParameters()["normal_factor_c"] = 0.3515; sl.sensorParameters()["normal_factor_e"] = 1.0;
    sl.sensorParameters()["lateral_factor"] = 0.01576;
    sl.updateTransformations(T, T, I4);
    sl.setRejectFilter(gem_reject_filter{0, 1.5f, 1.5f, 1.0f, 0.0f});
    check_add_depth(sl, img, depth, bgr, xyzi, rgb);

    gem::StereoSensorProcessor stereo;
    for (const char* q : {"p_1", "p_2", "p_3", "p_4", "p_5", "lateral_factor", "depth_to_disparity_factor"}) stereo.sensorParameters()[q] = 0.0;
    stereo.sensorParameters()["p_1"] = 0.1; stereo.sensorParameters()["p_2"] = 0.001; stereo.sensorParameters()["p_3"] = 380.0;
    stereo.sensorParameters()["p_4"] = 1.0; stereo.sensorParameters()["p_5"] = 0.002; stereo.sensorParameters()["lateral_factor"] = 0.001;
    stereo.sensorParameters()["depth_to_disparity_factor"] = 30.0;
    stereo.updateTransformations(T, T, I4);
    stereo.setRejectFilter(gem_reject_filter{0, 1.5f, 1.5f, 1.0f, 0.0f});
    check_add_depth(stereo, img, depth, bgr, xyzi, rgb);

    std::printf(fails ? "FAILED\n" : "OK\n");
    return fails;
}
