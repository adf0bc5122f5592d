// gem.hpp -- C++ host-side mirror of the reference's interface for the hot path, header-only, on top
// of the C ABI (include/gem_hip.h).  No Eigen / ROS / PCL / kindr types: rotations are row-major
// double[9], transforms row-major double[16]; the unmodified ROS node converts at the call site
//  or uses include/gem/gem_compat_eigen.hpp, which re-creates the nine
// C++-linkage symbols of the reference's libgpu.so.
//
// Mirrors (names and argument meaning):
//   SensorProcessorBase::updateTransformations / readcomputerparam / GPUPointCloudprocess / process
//       elevation_mapping/src/sensor_processors/SensorProcessorBase.cpp:97-124, 270-290, 126-211, 66-94
//   Laser / StructuredLight / Stereo / Perfect ::readParameters  (the *.yaml keys they read)
//   ElevationMapping::processpoints / updateMapLocation           src/ElevationMapping.cpp:254-283, 1001-1044
//   RobotMotionMapUpdater::update (+ computeReducedCovariance / computeRelativeCovariance)
//       src/RobotMotionMapUpdater.cpp:42-90, 92-109, 111-145
//   ElevationMap layer names                                      src/ElevationMap.cpp:43-44
//   ElevationMapping::updateLocalMap / visualPointMap (LocalMap)   src/ElevationMapping.cpp:609-767, 520-530
//   ElevationMapping::updateGlobalMap and globalMap_ (GlobalMap)   src/ElevationMapping.cpp:630-687, 773-905
//   pcl::VoxelGrid of the launch files' nodelets (VoxelGrid)       filter.launch, filter_kitti.launch
//   PointMapLayer / ElevationMapLayer ::updateBounds, ::updateCosts (Costmap)   layers/src/pointMap_layer.cpp:45-100, elevationMap_layer.cpp:42-87
//   costmap_2d::ObstacleLayer::updateBounds, which ElevationMapLayer derives from (Costmap::observe)   layers/src/elevationMap_layer.cpp:16
//   costmap_2d::VoxelLayer::updateBounds, the plugin for a 3-D sensor (Costmap::attachVoxels / voxelObserve)
#pragma once

#include "../gem_hip.h"

#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace gem {

class Error : public std::runtime_error {
public:
    Error(int code, const std::string& what) : std::runtime_error(what), code_(code) {}
    int code() const { return code_; }
private:
    int code_;
};

// PointXYZRGBICT (include/elevation_mapping/PointXYZRGBICT.hpp:26-48): the reference's input record.
struct alignas(16) PointXYZRGBICT {
    float x, y, z, pad;
    union { float rgb; struct { std::uint8_t b, g, r, a; }; };
    float covariance, intensity, travers;
};
static_assert(sizeof(PointXYZRGBICT) == 32, "Anypoint is 32 bytes");

using Mat3 = std::array<double, 9>;     // row-major
using Mat4 = std::array<double, 16>;    // row-major homogeneous transform
using Vec3 = std::array<double, 3>;

inline Mat3 transposed(const Mat3& m) { return {m[0], m[3], m[6], m[1], m[4], m[7], m[2], m[5], m[8]}; }
inline Mat3 mul(const Mat3& a, const Mat3& b)
{
    Mat3 c{};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
    return c;
}
inline Mat3 rotation_of(const Mat4& t) { return {t[0], t[1], t[2], t[4], t[5], t[6], t[8], t[9], t[10]}; }
inline Vec3 translation_of(const Mat4& t) { return {t[3], t[7], t[11]}; }

class ElevationMap;

// A depth image as sensor_msgs/Image + CameraInfo describe it: gem_depth_image, field for field (width, height, format GEM_DEPTH_*,
// row_stride = msg.step, fx = K[0], fy = K[4], cx = K[2], cy = K[5], depth_unit, intensity, color_format GEM_COLOR_*, color_row_stride)
using DepthImage = gem_depth_image;

// ---------------------------------------------------------------------------------------------
// SensorProcessorBase and its four subclasses
// ---------------------------------------------------------------------------------------------
class SensorProcessorBase {
public:
    virtual ~SensorProcessorBase() = default;

    // sensor_processor/ignore_points_above|below (SensorProcessorBase.cpp:61-62)
    void setIgnorePoints(double below, double above) { ignoreLower_ = below; ignoreUpper_ = above; }
    // the hard-coded sensor-frame reject filter of gpu_process.cu:393; on by default like the reference
    void setRejectFilter(const gem_reject_filter& f) { filter_ = f; }
    void setRotationVariance(const std::array<float, 9>& q) { rotationVariance_ = q; }

    // What the three TF lookups of SensorProcessorBase.cpp:97-124 return (map<-sensor, base<-sensor, map<-base).
    void updateTransformations(const Mat4& mapFromSensor, const Mat4& baseFromSensor, const Mat4& mapFromBase)
    {
        transformationSensorToMap_ = mapFromSensor;
        rotationBaseToSensor_ = rotation_of(baseFromSensor);
        translationBaseToSensorInBaseFrame_ = translation_of(baseFromSensor);
        rotationMapToBase_ = rotation_of(mapFromBase);
        translationMapToBaseInMapFrame_ = translation_of(mapFromBase);
    }

    // readcomputerparam (SensorProcessorBase.cpp:270-290) + the casts of GPUPointCloudprocess (:171-184).
    gem_frame_params frameParams() const
    {
        gem_frame_params p{};
        for (int i = 0; i < 16; ++i) p.T[i] = static_cast<float>(transformationSensorToMap_[i]);           // :175-179
        p.lower = translationMapToBaseInMapFrame_[2] + ignoreLower_;                                        // :183
        p.upper = translationMapToBaseInMapFrame_[2] + ignoreUpper_;                                        // :184
        const Mat3 C_BM_T = transposed(rotationMapToBase_);
        const Mat3 C_SB_T = transposed(rotationBaseToSensor_);
        const Mat3 J = mul(C_BM_T, C_SB_T);                                                                  // :275 (double product, float cast)
        for (int j = 0; j < 3; ++j) {
            p.sensor_jacobian[j] = static_cast<float>(J[6 + j]);
            p.P_mul_C_BM_T[j] = static_cast<float>(C_BM_T[6 + j]);                                           // :281-282
        }
        for (int i = 0; i < 9; ++i) { p.C_SB_T[i] = static_cast<float>(C_SB_T[i]); p.rotation_variance[i] = rotationVariance_[i]; }
        const float bx = static_cast<float>(translationBaseToSensorInBaseFrame_[0]);
        const float by = static_cast<float>(translationBaseToSensorInBaseFrame_[1]);
        const float bz = static_cast<float>(translationBaseToSensorInBaseFrame_[2]);
        const float sk[9] = {0.f, -bz, by, bz, 0.f, -bx, -by, bx, 0.f};                                      // :284 (kindr skew)
        std::memcpy(p.B_r_BS_skew, sk, sizeof(sk));
        p.sensor_model = sensorModel();
        fillSensorParams(p.sensor_params);
        p.filter = filter_;
        p.original_width = originalWidth_;
        return p;
    }

    // SensorProcessorBase::process (SensorProcessorBase.cpp:66-94): same out-arrays as the reference,
    // caller-owned, length = cloud size.  The cloud is assumed NaN-free (cleanPointCloud, Laser.cpp:50-59);
    // a raw cloud goes to processRaw, which does that step on the device.
    bool process(ElevationMap& map, const PointXYZRGBICT* cloud, int n,
                 int* point_colorR, int* point_colorG, int* point_colorB, int* point_index,
                 float* point_intensity, float* point_height, float* point_var);

    // ... on the RAW cloud as the driver publishes it (organised, NaN holes): cleanPointCloud (SensorProcessorBase.cpp:89, this
    // processor's cleanParams()) on the device, then Process_points on the kept points.  `width` = cloud->width (the stereo
    // processor's originalWidth_, StereoSensorProcessor.cpp:41).  The out-arrays (n elements each) hold the kept points in order,
    // colours and intensity taken from them -- the arrays the reference hands to Fuse.  Returns the kept count, or -1 on an error.
    int processRaw(ElevationMap& map, const PointXYZRGBICT* cloud, int n, int width,
                   int* point_colorR, int* point_colorG, int* point_colorB, int* point_index,
                   float* point_intensity, float* point_height, float* point_var);

    // SensorProcessorBase::process + Fuse on a depth image (image_rect_raw + camera_info instead of the cloud topic): this processor's
    // frame with originalWidth_ = the image's width (the pixel index is the raw position) and its cleanParams(), the unprojection
    // and the clean step on the device (ElevationMap::addDepth)
    void addDepth(ElevationMap& map, const DepthImage& image, const void* depth, const void* color = nullptr);

    // the cleanPointCloud step of this processor: removeNaNFromPointCloud (Laser.cpp:50-59, Perfect.cpp:41-49, Stereo.cpp:37-48);
    // the structured-light processor overrides it with its PassThrough on z
    virtual gem_clean_params cleanParams() const
    {
        gem_clean_params c{};
        gem_clean_params_for_model(sensorModel(), std::numeric_limits<double>::min(), std::numeric_limits<double>::max(), &c);
        return c;
    }

    std::map<std::string, double>& sensorParameters() { return sensorParameters_; }
    void setOriginalWidth(int w) { originalWidth_ = w; }

protected:
    virtual int  sensorModel() const = 0;
    virtual void fillSensorParams(double out[8]) const = 0;
    double param(const char* k) const { auto it = sensorParameters_.find(k); return it == sensorParameters_.end() ? 0.0 : it->second; }

    Mat4 transformationSensorToMap_{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    Mat3 rotationBaseToSensor_{1, 0, 0, 0, 1, 0, 0, 0, 1};
    Vec3 translationBaseToSensorInBaseFrame_{0, 0, 0};
    Mat3 rotationMapToBase_{1, 0, 0, 0, 1, 0, 0, 0, 1};
    Vec3 translationMapToBaseInMapFrame_{0, 0, 0};
    double ignoreUpper_ = std::numeric_limits<double>::infinity();
    double ignoreLower_ = -std::numeric_limits<double>::infinity();
    gem_reject_filter filter_{1, 1.5f, 1.5f, 1.0f, 0.0f};
    std::array<float, 9> rotationVariance_{};        // zero, SensorProcessorBase.cpp:202-204
    std::map<std::string, double> sensorParameters_;
    int originalWidth_ = 0;
};

class LaserSensorProcessor : public SensorProcessorBase {        // LaserSensorProcessor.cpp:41-48
protected:
    int sensorModel() const override { return GEM_MODEL_LASER; }
    void fillSensorParams(double o[8]) const override { o[0] = param("min_radius"); o[1] = param("beam_angle"); o[2] = param("beam_constant"); }
};
class StructuredLightSensorProcessor : public SensorProcessorBase {   // StructuredLightSensorProcessor.cpp:36-50
public:
    // pcl::PassThrough on z with sensor_processor/cutoff_min_depth | cutoff_max_depth, read with the reference's defaults
    // numeric_limits<double>::min() / ::max() (StructuredLightSensorProcessor.cpp:40-41, 51-66) -- not param()'s 0
    gem_clean_params cleanParams() const override
    {
        auto get = [&](const char* k, double dflt) { auto it = sensorParameters_.find(k); return it == sensorParameters_.end() ? dflt : it->second; };
        gem_clean_params c{};
        gem_clean_params_for_model(GEM_MODEL_STRUCTURED_LIGHT, get("cutoff_min_depth", std::numeric_limits<double>::min()),
                                   get("cutoff_max_depth", std::numeric_limits<double>::max()), &c);
        return c;
    }
protected:
    int sensorModel() const override { return GEM_MODEL_STRUCTURED_LIGHT; }
    void fillSensorParams(double o[8]) const override
    {
        o[0] = param("normal_factor_a"); o[1] = param("normal_factor_b"); o[2] = param("normal_factor_c");
        o[3] = param("normal_factor_d"); o[4] = param("normal_factor_e"); o[5] = param("lateral_factor");
    }
};
class StereoSensorProcessor : public SensorProcessorBase {       // StereoSensorProcessor.cpp:23-34
protected:
    int sensorModel() const override { return GEM_MODEL_STEREO; }
    void fillSensorParams(double o[8]) const override
    {
        o[0] = param("p_1"); o[1] = param("p_2"); o[2] = param("p_3"); o[3] = param("p_4"); o[4] = param("p_5");
        o[5] = param("lateral_factor"); o[6] = param("depth_to_disparity_factor");
    }
};
class PerfectSensorProcessor : public SensorProcessorBase {
protected:
    int sensorModel() const override { return GEM_MODEL_PERFECT; }
    void fillSensorParams(double*) const override {}
};

// ---------------------------------------------------------------------------------------------
// ElevationMap: the device-resident robot-centric map
// ---------------------------------------------------------------------------------------------
class ElevationMap {
public:
    // layer names of the reference's two GridMaps (ElevationMap.cpp:43-44)
    static const std::vector<std::string>& rawMapLayers()
    {
        static const std::vector<std::string> v{"elevation", "min_height", "height", "variance", "horizontal_variance_x",
            "horizontal_variance_y", "horizontal_variance_xy", "color", "timestamp", "time", "lowest_scan_point",
            "sensor_x_at_lowest_scan", "sensor_y_at_lowest_scan", "sensor_z_at_lowest_scan"};
        return v;
    }
    static const std::vector<std::string>& visualMapLayers()
    {
        static const std::vector<std::string> v{"elevation", "variance", "rough", "slope", "traver", "color_r", "color_g", "color_b", "intensity"};
        return v;
    }

    // Init_GPU_elevationmap(length, resolution, mahalanobis, obstacle_threshold)  (ElevationMapping.cpp:199)
    ElevationMap(int length, float resolution, float mahalanobisThreshold = 5.0f, float obstacleThreshold = 0.7f, int device = -1)
    {
        gem_map_config cfg{};
        cfg.length = length; cfg.resolution = resolution; cfg.mahalanobis_threshold = mahalanobisThreshold;
        cfg.variance_floor = 0.0001f; cfg.obstacle_threshold = obstacleThreshold; cfg.device = device;
        const int rc = gem_create(&cfg, &h_);
        if (rc != GEM_OK) throw Error(rc, std::string("gem_create: ") + gem_last_error(nullptr));
        length_ = length; resolution_ = resolution;
    }
    ~ElevationMap() { if (h_) gem_destroy(h_); }
    ElevationMap(const ElevationMap&) = delete;
    ElevationMap& operator=(const ElevationMap&) = delete;

    gem_handle* handle() const { return h_; }
    int length() const { return length_; }
    float resolution() const { return resolution_; }

    // ElevationMapping::updateMapLocation -> Move (ElevationMapping.cpp:1032) + ElevationMap::move (ElevationMap.cpp:172-177)
    void move(const float position[3], float center[2] = nullptr, int startIndex[2] = nullptr, float alignedShift[2] = nullptr)
    { check(gem_move(h_, position, center, startIndex, alignedShift), "gem_move"); }

    // the upstream ElevationMap::add(pointCloud, variances, ...) shape: project + bin + fuse in one call.
    void add(const gem_frame_params& frame, const float* xyzi, int n, const std::uint32_t* rgb = nullptr, const int* origIndex = nullptr)
    { check(gem_add(h_, &frame, n, xyzi, rgb, origIndex), "gem_add"); }
    void addDevice(const gem_frame_params& frame, const void* d_xyzi, int n, const void* d_rgb = nullptr, const void* d_origIndex = nullptr)
    { check(gem_add_device(h_, &frame, n, d_xyzi, d_rgb, d_origIndex), "gem_add_device"); }
    // ... of a RAW cloud: the cleanPointCloud step (SensorProcessorBase::cleanParams()) on the device; raw positions are the orig indices
    void addRaw(const gem_frame_params& frame, const gem_clean_params& clean, const float* xyzi, int n, const std::uint32_t* rgb = nullptr)
    { check(gem_add_raw(h_, &frame, &clean, n, xyzi, rgb), "gem_add_raw"); }
    void addRawDevice(const gem_frame_params& frame, const gem_clean_params& clean, const void* d_xyzi, int n, const void* d_rgb = nullptr)
    { check(gem_add_raw_device(h_, &frame, &clean, n, d_xyzi, d_rgb), "gem_add_raw_device"); }

    // ... of the cloud a DEPTH IMAGE unprojects to (gem_hip.h: depth_image_proc::convert, restated), made on the device: the image
    // crosses the link, not the cloud.  depth / color: host images laid out as `image` says; clean may be NULL
    void addDepth(const gem_frame_params& frame, const DepthImage& image, const void* depth, const void* color = nullptr,
                  const gem_clean_params* clean = nullptr)
    { check(gem_add_depth(h_, &frame, &image, depth, color, clean, nullptr, 0), "gem_add_depth"); }
    void addDepthDevice(const gem_frame_params& frame, const DepthImage& image, const void* d_depth, const void* d_color = nullptr,
                        const gem_clean_params* clean = nullptr)
    { check(gem_add_depth_device(h_, &frame, &image, d_depth, d_color, clean, nullptr, 0), "gem_add_depth_device"); }

    // Fuse(length, point_num, index, R, G, B, intensity, height, var)  (ElevationMapping.cpp:280)
    void fuse(int n, const int* index, const int* R, const int* G, const int* B, const float* intensity, const float* height, const float* var)
    { check(gem_fuse(h_, n, index, R, G, B, intensity, height, var), "gem_fuse"); }

    // Mapvar_update(length, var_update)  (RobotMotionMapUpdater.cpp:81)
    void update(float varianceUpdate) { check(gem_mapvar_update(h_, varianceUpdate), "gem_mapvar_update"); }

    // Map_feature(...) (ElevationMapping.cpp:410): traversability stage on the fused map; computes the ROUGH, SLOPE and
    // TRAVER layers on the device and copies out the arrays that are not null (flat storage order, length^2 floats)
    void mapFeature(float* rough = nullptr, float* slope = nullptr, float* traver = nullptr)
    { check(gem_map_feature(h_, nullptr, nullptr, nullptr, nullptr, nullptr, rough, slope, traver, nullptr), "gem_map_feature"); }

    // Raytracing(length) (ElevationMapping.cpp:421): visibility clean-up; needs trackLowest(true) while the frame is fused
    void trackLowest(bool on) { check(gem_set_lowest_tracking(h_, on ? 1 : 0), "gem_set_lowest_tracking"); }
    void raytracing() { check(gem_raytracing(h_), "gem_raytracing"); }

    // flat [storage_x * length + storage_y] array, the layout ElevationMap::show indexes (ElevationMap.cpp:98-111)
    std::vector<float> layer(int which) const
    {
        std::vector<float> v(static_cast<size_t>(length_) * length_);
        if (which >= GEM_LAYER_COLOR_R && which <= GEM_LAYER_COLOR_B) throw Error(GEM_ERR_INVALID, "colour layers are int32: use colorLayer()");
        check(gem_get_layer(h_, which, GEM_LAYOUT_STORAGE_ROWMAJOR, v.data()), "gem_get_layer");
        return v;
    }
    std::vector<int> colorLayer(int which) const
    {
        std::vector<int> v(static_cast<size_t>(length_) * length_);
        if (which < GEM_LAYER_COLOR_R || which > GEM_LAYER_COLOR_B) throw Error(GEM_ERR_INVALID, "not a colour layer");
        check(gem_get_layer(h_, which, GEM_LAYOUT_STORAGE_ROWMAJOR, v.data()), "gem_get_layer");
        return v;
    }
    // grid_map::Matrix memory (Eigen column-major, NaN for empty cells): memcpy into GridMap::get(layer).data()
    std::vector<float> gridMapLayer(int which) const
    {
        std::vector<float> v(static_cast<size_t>(length_) * length_);
        check(gem_get_layer(h_, which, GEM_LAYOUT_GRIDMAP_COLMAJOR_NAN, v.data()), "gem_get_layer");
        return v;
    }
    void synchronize() { check(gem_synchronize(h_), "gem_synchronize"); }
    // arenas for the largest pass to come (points per call, sweeps per call): no allocation inside the stream of frames afterwards
    void reserve(long long maxPoints, int maxSweeps = 1, bool withColours = false)
    { check(gem_reserve(h_, maxPoints, maxSweeps, withColours ? 1 : 0), "gem_reserve"); }
    // device inputs produced on another stream: everything enqueued from now on waits for this hipEvent_t (gem_wait_event)
    void waitEvent(void* hipEvent) { check(gem_wait_event(h_, hipEvent), "gem_wait_event"); }

    // ElevationMap::show's cell loop (ElevationMap.cpp:85-149) on the resident layers: visualMap_'s nine layers
    // (visualMapLayers() order, grid_map::Matrix memory, NaN for cells without elevation / traversability), the coloured
    // point cloud in grid_map's iteration order and the orthomosaic.  Geometry = visualMap_'s (doubles, ElevationMapping.cpp:178);
    // 0 / 0 / nullptr: length * resolution, the map's resolution and centre.
    struct Shown {
        std::vector<float> visual;            // 9 x length^2
        std::vector<float> pointsXYZ;         // n x 3
        std::vector<unsigned char> pointsRGB; // n x 3
        std::vector<unsigned char> imageBGR;  // length x length x 3
        int count = 0;
    };
    Shown show(double mapLength = 0.0, double resolution = 0.0, const double position[2] = nullptr) const
    {
        const size_t cells = static_cast<size_t>(length_) * length_;
        Shown s;
        s.visual.resize(9 * cells); s.pointsXYZ.resize(3 * cells); s.pointsRGB.resize(3 * cells); s.imageBGR.resize(3 * cells);
        check(gem_show(h_, mapLength, resolution, position, s.visual.data(), s.pointsXYZ.data(), s.pointsRGB.data(), &s.count, s.imageBGR.data()), "gem_show");
        s.pointsXYZ.resize(3 * static_cast<size_t>(s.count)); s.pointsRGB.resize(3 * static_cast<size_t>(s.count));
        return s;
    }

    // The colourisation loop of ElevationMapping::Callback (ElevationMapping.cpp:321-381) on the cloud as the node holds it:
    // P_lidar2img = Tcamera (3x4) * TLidar (4x4), every point takes the BGR pixel it lands on (b, g, r fields), draws its
    // radius-1 circle for the later points, and points outside the image get b = g = r = 0 and intensity 0.
    // image = cv::Mat::data of the BGR8 image, step = cv::Mat::step (0: width * 3); the image is not modified.
    static std::array<double, 12> lidarToImage(const std::array<double, 12>& Tcamera, const Mat4& TLidar)
    {
        std::array<double, 12> P{};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                double acc = Tcamera[4 * r] * TLidar[c];
                for (int k = 1; k < 4; ++k) acc = acc + Tcamera[4 * r + k] * TLidar[4 * k + c];
                P[4 * r + c] = acc;
            }
        return P;
    }
    void colorize(const std::array<double, 12>& lidar2img, int width, int height, const unsigned char* image, size_t step,
                  PointXYZRGBICT* cloud, int n) const
    {
        gem_camera cam{};
        for (int k = 0; k < 12; ++k) cam.lidar_to_image[k] = lidar2img[k];
        cam.width = width; cam.height = height;
        std::vector<float> xyzi(4 * static_cast<size_t>(n));
        std::vector<std::uint32_t> rgb(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) { xyzi[4 * i] = cloud[i].x; xyzi[4 * i + 1] = cloud[i].y; xyzi[4 * i + 2] = cloud[i].z; xyzi[4 * i + 3] = cloud[i].intensity; }
        check(gem_colorize(h_, &cam, n, xyzi.data(), image, step, rgb.data()), "gem_colorize");
        for (int i = 0; i < n; ++i) {
            cloud[i].r = static_cast<std::uint8_t>(rgb[i] >> 16); cloud[i].g = static_cast<std::uint8_t>(rgb[i] >> 8); cloud[i].b = static_cast<std::uint8_t>(rgb[i]);
            cloud[i].intensity = xyzi[4 * i + 3];
        }
    }

    void check(int rc, const char* what) const { if (rc != GEM_OK) throw Error(rc, std::string(what) + ": " + gem_last_error(h_)); }

private:
    gem_handle* h_ = nullptr;
    int length_ = 0;
    float resolution_ = 0.f;
};

// ---------------------------------------------------------------------------------------------
// The rolling-window local map of ElevationMapping::updateLocalMap (ElevationMapping.cpp:609-767) and the grid cloud of
// visualPointMap (:520-530), on the device (gem_local_*).  The flags and the gate of the node stay with the caller, see
// INTEGRATION.md.  Records: PointXYZRGBICT with pad = 1 and a = 0; exported entries carry their intensity (the reference's
// localHashtoPointCloud leaves it unset).
// ---------------------------------------------------------------------------------------------
// What octomap_msgs::fullMapToMsg would put into an Octomap message for the ColorOcTree pointCloudtoOctomap fills
// (ElevationMapping.cpp:1158-1173): msg.data, msg.resolution; msg.id = id(), msg.binary = false.  gem_hip.h states the contract.
struct ColorOcTreeData {
    std::vector<int8_t> data;           // msg.data (octomap_msgs/Octomap: int8[])
    double resolution = 0.0;
    gem_octree_stats stats{};
    static const char* id() { return "ColorOcTree"; }
};

class LocalMap {
public:
    // capacity: initial entries (grows on demand)
    explicit LocalMap(ElevationMap& map, long long capacity = 1 << 16) : map_(map)
    { map_.check(gem_local_enable(map_.handle(), capacity), "gem_local_enable"); }
    ~LocalMap() { gem_local_enable(map_.handle(), 0); }
    LocalMap(const LocalMap&) = delete;
    LocalMap& operator=(const LocalMap&) = delete;

    // map_.show()'s visualMap_ with its geometry (0 / 0 / nullptr: as ElevationMap::show).  Between mapFeature and raytracing.
    void capture(double mapLength = 0.0, double resolution = 0.0, const double position[2] = nullptr)
    { map_.check(gem_local_capture(map_.handle(), mapLength, resolution, position), "gem_local_capture"); }
    // prevMap_ = map_.visualMap_
    void keepPrevious() { map_.check(gem_local_keep_previous(map_.handle()), "gem_local_keep_previous"); }
    // gridMaptoPointCloud(map_.visualMap_, ...)
    std::vector<PointXYZRGBICT> gridCloud()
    {
        std::vector<PointXYZRGBICT> v(cells());
        int n = 0;
        map_.check(gem_local_grid_cloud(map_.handle(), v.data(), &n), "gem_local_grid_cloud");
        v.resize(static_cast<size_t>(n));
        return v;
    }
    // the "Local mapping" block's body (ElevationMapping.cpp:715-764): the cells it pushes to visualCloud_, in order; *replaced
    // (optional) = its `count`
    std::vector<PointXYZRGBICT> spill(const float currentPosition[2], const float positionShift[2], int* replaced = nullptr)
    {
        std::vector<PointXYZRGBICT> v(cells());
        int n = 0, r = 0;
        map_.check(gem_local_spill(map_.handle(), currentPosition, positionShift, v.data(), &n, &r), "gem_local_spill");
        v.resize(static_cast<size_t>(n));
        if (replaced) *replaced = r;
        return v;
    }
    // localHashtoPointCloud(localMap_, ...), in last-write order; clear: then localMap_.swap(tmp)
    std::vector<PointXYZRGBICT> exportCloud(bool clear = false)
    {
        std::vector<PointXYZRGBICT> v(static_cast<size_t>(size()));
        long long n = 0;
        map_.check(gem_local_export(map_.handle(), v.empty() ? nullptr : v.data(), static_cast<long long>(v.size()), &n, clear ? 1 : 0),
                   "gem_local_export");
        v.resize(static_cast<size_t>(n));
        return v;
    }
    long long size() const
    {
        long long n = 0;
        map_.check(gem_local_size(map_.handle(), &n), "gem_local_size");
        return n;
    }
    // pointCloudtoOctomap(gridMaptoPointCloud(prevMap_)) up to the octree insertion (ElevationMapping.cpp:1146-1170), on the capture
    // keepPrevious() kept: StatisticalOutlierRemoval(meanK, stddevMul), then the survivors with travers > traversThreshold (road) and
    // the others (obstacle), both in cloud order.  gem_hip.h states the filter and what of it is not verified against PCL.
    struct Composed {
        std::vector<PointXYZRGBICT> road, obstacle;
        int removed = 0;            // points the filter removed
        double threshold = 0.0;     // its distance threshold
    };
    Composed compose(int meanK = 20, double stddevMul = 1.0, double traversThreshold = 0.0, bool sqrtDouble = false)
    {
        // The library wants room for L * L records per list.  That room is kept between calls (one composing thread per LocalMap),
        // so a call neither allocates nor clears 2 * L * L records; only the records that came back are copied out.
        if (road_.size() < cells()) { road_.resize(cells()); obstacle_.resize(cells()); }
        gem_compose_params p{};
        p.mean_k = meanK; p.stddev_mul = stddevMul; p.travers_threshold = traversThreshold;
        p.flags = sqrtDouble ? GEM_COMPOSE_SQRT_DOUBLE : 0;
        int counts[3] = {0, 0, 0};
        Composed c;
        map_.check(gem_local_compose(map_.handle(), &p, road_.data(), obstacle_.data(), counts, &c.threshold), "gem_local_compose");
        c.road.assign(road_.begin(), road_.begin() + counts[0]);
        c.obstacle.assign(obstacle_.begin(), obstacle_.begin() + counts[1]);
        c.removed = counts[2];
        return c;
    }
    // ... and with the insertion loop: composingGlobalMap's two trees as their message bytes.  The two lists never leave the device.
    struct ComposedOcTrees {
        ColorOcTreeData road, obstacle;
        int roadPoints = 0, obstaclePoints = 0, removed = 0;
        double threshold = 0.0;
    };
    ComposedOcTrees compose_octrees(double roadResolution = 0.2, double obstacleResolution = 0.1, int meanK = 20, double stddevMul = 1.0,
                                   double traversThreshold = 0.0, bool sqrtDouble = false)
    {
        gem_compose_params p{};
        p.mean_k = meanK; p.stddev_mul = stddevMul; p.travers_threshold = traversThreshold;
        p.flags = sqrtDouble ? GEM_COMPOSE_SQRT_DOUBLE : 0;
        gem_octree_params rp{}, op{};
        rp.resolution = roadResolution; op.resolution = obstacleResolution;
        int counts[3] = {0, 0, 0};
        gem_octree_stats st[2] = {};
        ComposedOcTrees c;
        map_.check(gem_local_compose_octrees(map_.handle(), &p, &rp, &op, counts, &c.threshold, st), "gem_local_compose_octrees");
        c.roadPoints = counts[0]; c.obstaclePoints = counts[1]; c.removed = counts[2];
        c.road = readOcTree(GEM_OCTREE_ROAD, roadResolution, st[0]);
        c.obstacle = readOcTree(GEM_OCTREE_OBSTACLE, obstacleResolution, st[1]);
        return c;
    }
    // pointCloudtoOctomap's loop over a caller's cloud (e.g. visualOctomap's visualCloud_) in slot GEM_OCTREE_USER0 / _USER1
    ColorOcTreeData build_octree(const std::vector<PointXYZRGBICT>& cloud, double resolution, int slot = GEM_OCTREE_USER0)
    {
        gem_octree_params q{};
        q.resolution = resolution;
        gem_octree_stats st{};
        map_.check(gem_octree_build(map_.handle(), slot, &q, cloud.data(), static_cast<long long>(cloud.size()), &st), "gem_octree_build");
        return readOcTree(slot, resolution, st);
    }

private:
    ColorOcTreeData readOcTree(int slot, double resolution, const gem_octree_stats& st)
    {
        ColorOcTreeData t;
        t.resolution = resolution; t.stats = st;
        t.data.resize(static_cast<size_t>(st.bytes));
        size_t n = 0;
        map_.check(gem_octree_read(map_.handle(), slot, t.data.empty() ? nullptr : t.data.data(), t.data.size(), &n), "gem_octree_read");
        if (n != t.data.size()) throw Error(GEM_ERR_INVALID, "gem_octree_read: the slot was rebuilt by another thread");
        return t;
    }
    size_t cells() const { const size_t L = static_cast<size_t>(map_.length()); return L * L; }
    ElevationMap& map_;
    std::vector<PointXYZRGBICT> road_, obstacle_;      // compose()'s landing room, L * L records each once it has been called
};

// ---------------------------------------------------------------------------------------------
// The submap stack globalMap_ of ElevationMapping (ElevationMapping.cpp:630-687 push, :773-905 updateGlobalMap) on the device
// (gem_global_*).  The pose bookkeeping (trajectory_, localMapLoc_, optGlobalMapLoc_, the flags) stays with the caller, see
// INTEGRATION.md; the handle's lock replaces GlobalMapMutex_.
// ---------------------------------------------------------------------------------------------
class GlobalMap {
public:
    // capacity: initial records (grows on demand)
    explicit GlobalMap(ElevationMap& map, long long capacity = 1 << 20) : map_(map)
    { map_.check(gem_global_enable(map_.handle(), capacity), "gem_global_enable"); }
    ~GlobalMap() { gem_global_enable(map_.handle(), 0); }
    GlobalMap(const GlobalMap&) = delete;
    GlobalMap& operator=(const GlobalMap&) = delete;

    // globalMap_.push_back(*out_pc + *grid_pc), device to device; clearLocal: then localMap_.swap(tmp).  Returns the submap's index.
    int pushLocal(bool clearLocal = true)
    {
        int i = -1;
        map_.check(gem_global_push_local(map_.handle(), clearLocal ? 1 : 0, &i), "gem_global_push_local");
        return i;
    }
    // a cloud of the caller's (the denseSubmap branch: pointcloudinterpolation's output)
    int push(const std::vector<PointXYZRGBICT>& cloud)
    {
        int i = -1;
        map_.check(gem_global_push(map_.handle(), cloud.empty() ? nullptr : cloud.data(), static_cast<long long>(cloud.size()), &i),
                   "gem_global_push");
        return i;
    }
    // updateGlobalMap's body: transforms[i] = (optGlobalMapLoc_[i] * trajectory_[i].inverse()).matrix() as Matrix4f::data()
    // (column-major), centres[i] = localMapLoc_[i]; one of each per optimised keyframe.  Returns the fused count.
    long long loopClosure(const std::vector<std::array<float, 16>>& transforms, const std::vector<std::array<float, 2>>& centres,
                          float radius = 25.f, double resolution = 0.0)
    {
        static_assert(sizeof(std::array<float, 16>) == 64 && sizeof(std::array<float, 2>) == 8, "packed matrices and centres");
        if (transforms.size() != centres.size()) throw Error(GEM_ERR_INVALID, "GlobalMap::loopClosure: one centre per transform");
        long long fused = 0;
        map_.check(gem_global_loop_closure(map_.handle(), static_cast<int>(transforms.size()),
                                           transforms.empty() ? nullptr : transforms[0].data(), centres.empty() ? nullptr : centres[0].data(),
                                           radius, resolution, &fused), "gem_global_loop_closure");
        return fused;
    }
    // submap `index`, or all of them in stack order (-1: visualCloud_, composingGlobalMap, savingMap)
    std::vector<PointXYZRGBICT> exportCloud(int index = -1)
    {
        long long n = 0;
        map_.check(gem_global_export(map_.handle(), index, nullptr, 0, &n), "gem_global_export");
        std::vector<PointXYZRGBICT> v(static_cast<size_t>(n));
        map_.check(gem_global_export(map_.handle(), index, v.empty() ? nullptr : v.data(), n, &n), "gem_global_export");
        return v;
    }
    int size() const
    {
        int n = 0;
        map_.check(gem_global_count(map_.handle(), &n), "gem_global_count");
        return n;
    }

private:
    ElevationMap& map_;
};

// ---------------------------------------------------------------------------------------------
// visualCloud_ of ElevationMapping on the device (gem_history_*): while a History lives, LocalMap::spill appends what it selects
// (ElevationMapping.cpp:750-760), resetFromGlobal is visualCloud_.clear() plus the "Visual step" of updateGlobalMap (:788, :894-897),
// exportCloud(true) is visualPointMap's visualCloud_ + grid_pc (:524-526), and Costmap::markHistory marks it where it lies.
// ---------------------------------------------------------------------------------------------
class History {
public:
    // capacity: initial records (grows on demand)
    explicit History(ElevationMap& map, long long capacity = 1 << 20) : map_(map)
    { map_.check(gem_history_enable(map_.handle(), capacity), "gem_history_enable"); }
    ~History() { gem_history_enable(map_.handle(), 0); }
    History(const History&) = delete;
    History& operator=(const History&) = delete;

    // records of the caller's behind the history (a saved map loaded again)
    void append(const std::vector<PointXYZRGBICT>& cloud)
    {
        map_.check(gem_history_append(map_.handle(), cloud.empty() ? nullptr : cloud.data(), static_cast<long long>(cloud.size())),
                   "gem_history_append");
    }
    // ... in device memory: only enqueued, the buffer is untouched until ElevationMap::synchronize
    void appendDevice(const void* d_points, long long n)
    { map_.check(gem_history_append_device(map_.handle(), d_points, n), "gem_history_append_device"); }
    void resetFromGlobal() { map_.check(gem_history_reset_from_global(map_.handle()), "gem_history_reset_from_global"); }
    void clear() { map_.check(gem_history_clear(map_.handle()), "gem_history_clear"); }
    long long size() const
    {
        long long n = 0;
        map_.check(gem_history_size(map_.handle(), &n), "gem_history_size");
        return n;
    }
    // the history (savingMap); withGridCloud: followed by the last capture's grid cloud (visualPointMap)
    std::vector<PointXYZRGBICT> exportCloud(bool withGridCloud = false)
    {
        long long n = 0;
        map_.check(gem_history_export(map_.handle(), withGridCloud ? 1 : 0, nullptr, 0, &n), "gem_history_export");
        std::vector<PointXYZRGBICT> v(static_cast<size_t>(n));
        map_.check(gem_history_export(map_.handle(), withGridCloud ? 1 : 0, v.empty() ? nullptr : v.data(), n, &n), "gem_history_export");
        return v;
    }

private:
    ElevationMap& map_;
};

// ---------------------------------------------------------------------------------------------
// A layer costmap on the device (gem_costmap_*): the updateBounds bodies of the reference's two costmap_2d plugins
// (layers/src/pointMap_layer.cpp:45-100, elevationMap_layer.cpp:42-87) as marking passes, Costmap2D::updateOrigin as the rolling
// step, the two updateCosts rules and a window read-back.  costmap_2d itself is restated in gem_hip.h, unverified against the
// library.  Extra bounds, enabled_ and the layered costmap stay with the caller, see INTEGRATION.md.  The footprint calls
// (gem_hip_footprint.h) clear the robot's outline out of a layer and answer base_local_planner's footprintCost in batches; the MapGrid
// calls (gem_hip_mapgrid.h) keep its path and goal distance grids and score trajectories against them; bestTrajectory
// (gem_hip_critics.h) combines the critics as SimpleScoredSamplingPlanner does and picks the winner.
// ---------------------------------------------------------------------------------------------
// a pose as the footprint calls take it: the heading as its cosine and sine (the kernels hold no transcendental)
struct FootprintPose : gem_footprint_pose {
    FootprintPose() : gem_footprint_pose{0.0, 0.0, 1.0, 0.0} {}
    FootprintPose(double x_, double y_, double cosTheta, double sinTheta) : gem_footprint_pose{x_, y_, cosTheta, sinTheta} {}
    static FootprintPose fromYaw(double x_, double y_, double theta) { return FootprintPose(x_, y_, std::cos(theta), std::sin(theta)); }
};
static_assert(sizeof(FootprintPose) == sizeof(gem_footprint_pose), "an array of FootprintPose is an array of gem_footprint_pose");
// a footprint specification: the polygon's vertices in the robot's frame, at most GEM_FOOTPRINT_MAX_VERTICES
struct FootprintPoint { double x, y; };
// InflationLayer's parameters (gem_hip_inflate.h): inflation_radius, the robot's inscribed radius, cost_scaling_factor, inflate_unknown
struct InflationParams : gem_inflation_params {
    InflationParams() : gem_inflation_params{0.55, 0.0, 10.0, 0} {}
    InflationParams(double inflationRadius, double inscribedRadius, double costScalingFactor = 10.0, bool inflateUnknown = false)
        : gem_inflation_params{inflationRadius, inscribedRadius, costScalingFactor, inflateUnknown ? 1 : 0} {}
    // cell_inflation_radius_ at this resolution and the costs by squared cell distance, [0 .. R * R] (host only)
    std::vector<unsigned char> table(double resolution, int* cells = nullptr) const
    {
        int r = 0;
        if (gem_inflation_table(this, resolution, nullptr, &r) != GEM_OK) throw Error(GEM_ERR_INVALID, "InflationParams::table: unusable parameters");
        std::vector<unsigned char> t(static_cast<size_t>(r) * static_cast<size_t>(r) + 1);
        gem_inflation_table(this, resolution, t.data(), nullptr);
        if (cells) *cells = r;
        return t;
    }
};

// one observation of an ObservationBuffer as ObstacleLayer::updateBounds reads it (gem_hip_obstacle.h): the cloud in the global frame,
// the sensor's origin, the two ranges and the buffer's height window, with costmap_2d's defaults
struct Observation : gem_observation {
    Observation() : gem_observation{nullptr, 0, 12u, GEM_OBS_MARKING | GEM_OBS_CLEARING, {0.0, 0.0, 0.0}, 2.5, 3.0, 0.0, 2.0} {}
    // `cloud` must outlive the call that takes the observation
    Observation(const std::vector<PointXYZRGBICT>& cloud, double originX, double originY, double originZ, bool marking = true, bool clearing = true)
        : Observation()
    {
        points = cloud.empty() ? nullptr : cloud.data(); n = static_cast<long long>(cloud.size()); point_step = sizeof(PointXYZRGBICT);
        flags = (marking ? GEM_OBS_MARKING : 0u) | (clearing ? GEM_OBS_CLEARING : 0u);
        origin[0] = originX; origin[1] = originY; origin[2] = originZ;
    }
};
static_assert(sizeof(Observation) == sizeof(gem_observation), "an array of Observation is an array of gem_observation");

// the voxel grid of a VoxelLayer (gem_hip_voxlayer.h) with costmap_2d's defaults: ten voxels of 0.2 m from z = 0, unknown_threshold 15,
// mark_threshold 0
struct VoxelConfig : gem_voxel_config {
    VoxelConfig(unsigned sizeZ = 10, double zResolution = 0.2, double originZ = 0.0, unsigned unknownThreshold = 15, unsigned markThreshold = 0)
        : gem_voxel_config{sizeZ, zResolution, originZ, unknownThreshold, markThreshold} {}
};

// a critic of the best-trajectory call (gem_hip_critics.h): its kind, what it reads and its scale, in the order the planner sums them
struct Critic : gem_critic {
    Critic() : gem_critic{GEM_CRITIC_EXTERNAL, 0, 0, 0, 0.0, 0.0} {}
    // ObstacleCostFunction: flags of GEM_FOOTPRINT_INSCRIBED_LETHAL | GEM_FOOTPRINT_SUM | GEM_CRITIC_CENTRE_COST
    static Critic obstacle(double scale, int flags = 0) { return make(GEM_CRITIC_OBSTACLE, 0, flags, 0, scale, 0.0); }
    // MapGridCostFunction on GEM_CRITIC_GRID_PATH / _GOAL / _FRONT: flags of GEM_MAPGRID_STOP_ON_FAILURE | GEM_MAPGRID_SUM
    static Critic mapGrid(double scale, int grid, double xshift = 0.0, int flags = 0) { return make(GEM_CRITIC_MAPGRID, grid, flags, 0, scale, xshift); }
    // a critic the caller scored (oscillation, twirling, prefer-forward): column `column` of the ext array
    static Critic external(double scale, int column) { return make(GEM_CRITIC_EXTERNAL, 0, 0, column, scale, 0.0); }
private:
    static Critic make(int kind, int grid, int flags, int column, double scale, double xshift)
    {
        Critic c;
        c.kind = kind; c.grid = grid; c.flags = flags; c.column = column; c.scale = scale; c.xshift = xshift;
        return c;
    }
};
static_assert(sizeof(Critic) == sizeof(gem_critic), "an array of Critic is an array of gem_critic");
// findBestTrajectory's answer: index -1 and cost -1.0 without a valid trajectory
struct BestTrajectory : gem_best_trajectory {
    BestTrajectory() : gem_best_trajectory{-1, 0, -1.0, 0} {}
    bool valid() const { return index >= 0; }
};
static_assert(sizeof(BestTrajectory) == sizeof(gem_best_trajectory), "a BestTrajectory is a gem_best_trajectory");
// The combination and the winner over scores the caller holds, scores[k * n + t] of critic k and trajectory t (host only, no device)
inline BestTrajectory selectTrajectory(const std::vector<Critic>& critics, const std::vector<double>& scores, std::vector<double>* totals = nullptr)
{
    if (critics.empty() || scores.size() % critics.size()) throw Error(GEM_ERR_INVALID, "selectTrajectory: one score per critic and trajectory");
    const long long n = static_cast<long long>(scores.size() / critics.size());
    if (totals) totals->assign(static_cast<size_t>(n), 0.0);
    BestTrajectory b;
    if (gem_critics_select(critics.data(), static_cast<int>(critics.size()), scores.empty() ? nullptr : scores.data(), n,
                           totals && n ? totals->data() : nullptr, &b) != GEM_OK)
        throw Error(GEM_ERR_INVALID, "selectTrajectory: 1 .. 8 critics, every scale finite and not negative");
    return b;
}

// DWA's sampled trajectories (gem_hip_trajgen.h): SimpleTrajectoryGenerator's limits and configuration, the plan (the velocity window's
// three sample lists), the host twin of the generating kernel, and the velocity of a sample.  The contract is restated there, unverified
// against base_local_planner.
struct TrajectoryLimits : gem_trajgen_limits {
    TrajectoryLimits() : gem_trajgen_limits{0.55, 0.0, 0.1, -0.1, 1.0, 0.4, 0.55, 0.1, 2.5, 2.5, 3.2} {}      // dwa_local_planner's defaults
};
struct TrajectoryConfig : gem_trajgen_config {
    TrajectoryConfig() : gem_trajgen_config{1.7, 0.025, 0.1, 0.05, 1, 0, 0, 0, {6, 1, 20}, 0} {}
};
struct TrajectoryState { float pos[3], vel[3]; };            // (x, y, theta) and (vx, vy, vtheta)
struct TrajectoryPlan : gem_dwa_plan {
    TrajectoryPlan() : gem_dwa_plan{} {}
    // initialise: the window and the lists for this state; goal is read without use_dwa only
    TrajectoryPlan(const TrajectoryLimits& limits, const TrajectoryConfig& config, const TrajectoryState& s, float goalX = 0.f, float goalY = 0.f)
        : gem_dwa_plan{}
    {
        const float goal[2] = {goalX, goalY};
        if (gem_trajgen_plan(&limits, &config, s.pos, s.vel, goal, this) != GEM_OK)
            throw Error(GEM_ERR_INVALID, "TrajectoryPlan: a parameter that is not finite, a time or granularity <= 0, unknown oscillation bits, or lists of more than 256 values");
    }
    std::vector<float> list(int axis) const                  // 0: x, 1: y, 2: theta
    {
        const int at[4] = {0, n_x, n_x + n_y, n_x + n_y + n_th};
        return std::vector<float>(samples + at[axis], samples + at[axis + 1]);
    }
    // (xv, yv, thetav) of a sample: the command of dwaBest's winner
    std::array<float, 3> velocity(const TrajectoryState& s, long long index) const
    {
        std::array<float, 3> v{};
        if (gem_trajgen_velocity(this, s.vel, index, v.data()) != GEM_OK) throw Error(GEM_ERR_INVALID, "TrajectoryPlan::velocity: no such sample");
        return v;
    }
};
static_assert(sizeof(TrajectoryPlan) == sizeof(gem_dwa_plan), "a TrajectoryPlan is a gem_dwa_plan");
struct Trajectories {
    int posesPerTrajectory = 0;
    std::vector<FootprintPose> poses;                        // [trajectories * posesPerTrajectory]: slot t is sample t
    std::vector<int> length;                                 // poses each trajectory uses; 0: not generated
    std::vector<double> ext;                                 // [2][trajectories]: oscillation | twirling
    std::vector<float> velocity;                             // [trajectories][3]: xv, yv, thetav
};
// generateTrajectory for every sample of the plan on the host (gem_trajgen_generate: the twin of the kernel); posesPerTrajectory 0: the
// plan's max_steps
inline Trajectories generateTrajectories(const TrajectoryPlan& plan, const TrajectoryState& s, int posesPerTrajectory = 0)
{
    Trajectories out;
    out.posesPerTrajectory = posesPerTrajectory > 0 ? posesPerTrajectory : (plan.max_steps > 0 ? plan.max_steps : 1);
    const size_t n = static_cast<size_t>(plan.n_traj > 0 ? plan.n_traj : 0);
    out.poses.resize(n * static_cast<size_t>(out.posesPerTrajectory));
    out.length.assign(n, 0); out.ext.assign(2 * n, 0.0); out.velocity.assign(3 * n, 0.f);
    if (gem_trajgen_generate(&plan, s.pos, s.vel, out.poses.data(), out.length.data(), out.ext.data(), out.velocity.data(), out.posesPerTrajectory) != GEM_OK)
        throw Error(GEM_ERR_INVALID, "generateTrajectories: a plan or state the call refuses, posesPerTrajectory below the plan's max_steps, or |theta| beyond 64 pi");
    return out;
}

// Trajectory rollout (gem_hip_rollout.h): base_local_planner's TrajectoryPlanner::createTrajectories, the planner move_base runs when
// none is named -- the configuration, the plan (the window and the candidates' lists for a state and the caller's state flags), the
// answer, the host twin and the pick alone.  The contract is restated there from memory, unverified against base_local_planner.
struct RolloutConfig : gem_rollout_config {
    RolloutConfig()                                          // TrajectoryPlannerROS's defaults (meter_scoring off)
        : gem_rollout_config{1.0, 0.025, 0.025, 0.05, 0.6, 0.8, 0.01, 0.325, 0.5, 0.1, 1.0, -1.0, 0.4, -0.1, 2.5, 2.5, 3.2, 0.0, 0.0,
                             3, 20, 1, 1, 0, 4, {-0.3, -0.1, 0.1, 0.3, 0.0, 0.0, 0.0, 0.0}} {}
    void finalGoal(double x, double y) { final_goal_x = x; final_goal_y = y; final_goal_valid = 1; }
};
struct RolloutState { double pos[3], vel[3]; };              // (x, y, theta) and (vx, vy, vtheta)
struct RolloutBest : gem_rollout_best {
    RolloutBest() : gem_rollout_best{-1, 0, 0, -1.0, -1.0, 0.0, 0.0, 0.0, 0} {}
};
static_assert(sizeof(RolloutBest) == 64, "the answer is 64 bytes");
typedef struct ::gem_rollout_plan RolloutPlanData;          // (the C call of the same name hides the bare struct name)
struct RolloutPlan : RolloutPlanData {
    RolloutPlan() : RolloutPlanData{} {}
    RolloutPlan(const RolloutConfig& config, const RolloutState& s, int stateFlags = 0) : RolloutPlanData{}
    {
        if (::gem_rollout_plan(&config, s.pos, s.vel, stateFlags, this) != GEM_OK)
            throw Error(GEM_ERR_INVALID, "RolloutPlan: a parameter that is not finite, a time or granularity <= 0, fewer than two samples, more than 256 list "
                                         "values, a negative scale, a zero y_vel, unknown state bits, more than 4096 steps, or |theta| beyond 64 pi");
    }
    // the pick alone over the candidates' costs and `ahead` (host only); the ESCAPING bit of stateFlags must be the plan's
    RolloutBest pick(int stateFlags, const std::vector<double>& cost, const std::vector<int>& ahead) const
    {
        RolloutBest b;
        if (cost.size() != static_cast<size_t>(n_cand) || ahead.size() != cost.size() || gem_rollout_pick(this, stateFlags, cost.data(), ahead.data(), &b) != GEM_OK)
            throw Error(GEM_ERR_INVALID, "RolloutPlan::pick: one cost and one ahead per candidate, the plan's ESCAPING bit");
        return b;
    }
};
static_assert(sizeof(RolloutPlan) == sizeof(RolloutPlanData), "a RolloutPlan is a gem_rollout_plan");
struct Rollout {
    RolloutBest best;
    std::vector<double> cost;                                // [candidates]
    std::vector<int> ahead, steps;                           // [candidates]: GOAL ahead of the end pose (-1: none) | poses recorded (host twin only)
    std::vector<FootprintPose> poses;                        // [candidates * plan.max_steps] (host twin, on request)
};
// The host twin of Costmap::rolloutBest (gem_rollout_host) over the caller's bytes and PATH / GOAL grids, row-major [size_y * size_x]
inline Rollout rolloutHost(const RolloutPlan& plan, const RolloutState& s, const gem_costmap_config& geometry, const std::vector<unsigned char>& bytes,
                           const std::vector<int>& path, const std::vector<int>& goal, const std::vector<FootprintPoint>& spec, int flags = 0,
                           bool wantPoses = false)
{
    const size_t cells = static_cast<size_t>(geometry.size_x) * geometry.size_y, n = static_cast<size_t>(plan.n_cand > 0 ? plan.n_cand : 0);
    if (bytes.size() != cells || path.size() != cells || goal.size() != cells) throw Error(GEM_ERR_INVALID, "rolloutHost: one byte and two distances per cell");
    Rollout out;
    out.cost.assign(n, 0.0); out.ahead.assign(n, -1); out.steps.assign(n, 0);
    if (wantPoses) out.poses.assign(n * static_cast<size_t>(plan.max_steps > 0 ? plan.max_steps : 1), FootprintPose{0.0, 0.0, 0.0, 0.0});
    if (gem_rollout_host(&plan, s.pos, s.vel, &geometry, bytes.data(), path.data(), goal.data(), spec.empty() ? nullptr : &spec.front().x,
                         static_cast<int>(spec.size()), flags, out.cost.data(), out.ahead.data(), out.steps.data(), wantPoses ? out.poses.data() : nullptr,
                         &out.best) != GEM_OK)
        throw Error(GEM_ERR_INVALID, "rolloutHost: an argument the contract of gem_hip_rollout.h refuses");
    return out;
}

// A global plan (gem_hip_navplan.h): global_planner's makePlan in its order-free configuration -- Dijkstra, the non-quadratic
// potential, the grid path -- restated from memory and unverified against the library.  The weight table is indexed by the cost
// byte, 0 = impassable.
struct NavPlan {
    bool found = false;
    std::vector<FootprintPoint> path;                        // cell centres from the start to the goal, both included
    gem_navplan_status status{};
    // Expander::getCost as a table (host only); a factor under which a traversable cost is not a whole number is refused
    static std::vector<int> weights(int neutralCost = 50, double costFactor = 3.0, int lethalCost = 253, bool allowUnknown = true)
    {
        std::vector<int> w(256, 0);
        if (gem_navplan_weights(neutralCost, costFactor, lethalCost, allowUnknown ? 1 : 0, w.data()) != GEM_OK)
            throw Error(GEM_ERR_INVALID, "NavPlan::weights: parameters out of range, or a traversable cost that is not a positive whole number");
        return w;
    }
};

// Paths on the last plan's potential for a batch of goals (gem_hip_navpath.h): the grid path, or global_planner's default, the gradient
// path -- sub-cell points half a cell apart, restated from memory and unverified against the library.  One entry per goal, in order.
struct NavPaths {
    std::vector<gem_navpath_result> results;                 // status (GEM_NAVPATH_FOUND ...), n_points, the goal's cell and potential
    std::vector<std::vector<FootprintPoint>> paths;          // world points from the start to the goal; what was walked, when not found
    bool found(size_t i) const { return results[i].status == GEM_NAVPATH_FOUND; }
};

// What Costmap::prepareMapGridTiled / prepareMapGridFrontTiled answer (gem_hip_mapgrid.h): rounds depends on timing, the grids do not.
struct MapGridTiledStatus {
    bool started = false;                                    // a point of the plan was accepted
    int goalX = -1, goalY = -1;                              // the local goal's cell
    int rounds = 0, chunks = 0;                              // launches that found an active tile | host round trips
    static MapGridTiledStatus from(const gem_mapgrid_tiled_status& s)
    {
        MapGridTiledStatus r;
        r.started = s.started != 0; r.goalX = s.goal_cell[0]; r.goalY = s.goal_cell[1]; r.rounds = s.rounds; r.chunks = s.chunks;
        return r;
    }
};

// A frontier (gem_hip_frontier.h): an 8-connected component of the unknown cells that have a known 4-neighbour the last plan reached;
// in the manner of explore_lite's FrontierSearch, restated from memory and unverified against the library.
struct Frontier {
    gem_frontier record{};
    double originX = 0.0, originY = 0.0, resolution = 0.0;   // the costmap's geometry when the search ran
    // the mean of its cells' centres: origin + ((double)sum / (double)size + 0.5) * resolution
    FootprintPoint centroid() const
    {
        return FootprintPoint{originX + (static_cast<double>(record.sum_x) / static_cast<double>(record.size) + 0.5) * resolution,
                              originY + (static_cast<double>(record.sum_y) / static_cast<double>(record.size) + 0.5) * resolution};
    }
};

struct FrontierSearch {
    gem_frontier_status status{};
    bool found = false;                                      // a frontier was kept
    Frontier best;                                           // the kept frontier of least cost, when found
};

class Costmap {
public:
    static constexpr unsigned char FREE_SPACE = 0, INSCRIBED_INFLATED_OBSTACLE = 253, LETHAL_OBSTACLE = 254, NO_INFORMATION = 255;
    enum MergeMode { Overwrite = 0, Max = 1 };
    // a mark's bounds, in / out as updateBounds' four pointers
    struct Bounds { double min_x, min_y, max_x, max_y; };

    // defaultValue: NO_INFORMATION with track_unknown_space, FREE_SPACE without (ObstacleLayer); PointMapLayer never sets it
    Costmap(ElevationMap& map, unsigned sizeX, unsigned sizeY, double resolution, double originX = 0.0, double originY = 0.0,
            unsigned char defaultValue = NO_INFORMATION) : map_(map)
    {
        gem_costmap_config c{};
        c.size_x = sizeX; c.size_y = sizeY; c.resolution = resolution; c.origin_x = originX; c.origin_y = originY;
        c.default_value = defaultValue;
        map_.check(gem_costmap_create(map_.handle(), &c, &id_), "gem_costmap_create");
    }
    ~Costmap() { gem_costmap_destroy(map_.handle(), id_); }
    Costmap(const Costmap&) = delete;
    Costmap& operator=(const Costmap&) = delete;

    int id() const { return id_; }
    gem_costmap_config geometry() const
    {
        gem_costmap_config c{};
        map_.check(gem_costmap_geometry(map_.handle(), id_, &c), "gem_costmap_geometry");
        return c;
    }
    void resetMaps() { map_.check(gem_costmap_reset(map_.handle(), id_), "gem_costmap_reset"); }
    void updateOrigin(double newOriginX, double newOriginY)
    { map_.check(gem_costmap_update_origin(map_.handle(), id_, newOriginX, newOriginY), "gem_costmap_update_origin"); }
    // if (rolling_window_) updateOrigin(robot_x - getSizeInMetersX() / 2, robot_y - getSizeInMetersY() / 2)
    void rollTo(double robotX, double robotY) { map_.check(gem_costmap_roll_to(map_.handle(), id_, robotX, robotY), "gem_costmap_roll_to"); }

    // PointMapLayer::updateBounds' loop over a cloud of the caller's; bounds nullptr: only enqueued
    void markPoints(const std::vector<PointXYZRGBICT>& cloud, double traversThresh, Bounds* bounds = nullptr)
    {
        map_.check(gem_costmap_mark_points(map_.handle(), id_, cloud.empty() ? nullptr : cloud.data(), static_cast<long long>(cloud.size()),
                                           traversThresh, ptr(bounds)), "gem_costmap_mark_points");
    }
    // ... over the last capture's grid cloud, and over submap `index` of the stack (-1: all, in stack order), where they lie
    void markGridCloud(double traversThresh, Bounds* bounds = nullptr)
    { map_.check(gem_costmap_mark_grid_cloud(map_.handle(), id_, traversThresh, ptr(bounds)), "gem_costmap_mark_grid_cloud"); }
    void markGlobal(int index, double traversThresh, Bounds* bounds = nullptr)
    { map_.check(gem_costmap_mark_global(map_.handle(), id_, index, traversThresh, ptr(bounds)), "gem_costmap_mark_global"); }
    // ... over the history cloud (gem::History) where it lies, as one input; markGridCloud after it is visualCloud_ + grid_pc
    void markHistory(double traversThresh, Bounds* bounds = nullptr)
    { map_.check(gem_costmap_mark_history(map_.handle(), id_, traversThresh, ptr(bounds)), "gem_costmap_mark_history"); }
    // ElevationMapLayer::updateBounds' loop over the last capture standing for visualMap_
    void markVisual(double traversThresh, Bounds* bounds = nullptr)
    { map_.check(gem_costmap_mark_visual(map_.handle(), id_, traversThresh, ptr(bounds)), "gem_costmap_mark_visual"); }

    // updateCosts onto a master of the same size inside [minI, maxI) x [minJ, maxJ)
    void merge(Costmap& master, int minI, int minJ, int maxI, int maxJ, MergeMode mode = Overwrite)
    { map_.check(gem_costmap_merge(map_.handle(), id_, master.id_, minI, minJ, maxI, maxJ, mode), "gem_costmap_merge"); }
    // the window's bytes, row-major, (maxI - minI) per row
    std::vector<unsigned char> read(int minI, int minJ, int maxI, int maxJ) const
    {
        const size_t w = maxI > minI ? static_cast<size_t>(maxI - minI) : 0, rows = maxJ > minJ ? static_cast<size_t>(maxJ - minJ) : 0;
        std::vector<unsigned char> v(w * rows);
        map_.check(gem_costmap_read(map_.handle(), id_, minI, minJ, maxI, maxJ, v.empty() ? nullptr : v.data(), w), "gem_costmap_read");
        return v;
    }

    // ... and the reverse: (maxI - minI) * (maxJ - minJ) bytes, row-major, into the window (costs of the caller's other layers)
    void write(int minI, int minJ, int maxI, int maxJ, const std::vector<unsigned char>& values)
    {
        const size_t w = maxI > minI ? static_cast<size_t>(maxI - minI) : 0, rows = maxJ > minJ ? static_cast<size_t>(maxJ - minJ) : 0;
        if (values.size() != w * rows) throw Error(GEM_ERR_INVALID, "Costmap::write: one byte per cell of the window");
        map_.check(gem_costmap_write(map_.handle(), id_, minI, minJ, maxI, maxJ, values.empty() ? nullptr : values.data(), w), "gem_costmap_write");
    }

    // updateFootprint + setConvexPolygonCost(FREE_SPACE) of ObstacleLayer: every transformed vertex is touched into bounds, the
    // polygon's cells become FREE_SPACE.  Only enqueued.  False (nothing written) when a vertex is off the map.
    bool clearFootprint(const FootprintPose& pose, const std::vector<FootprintPoint>& spec, Bounds* bounds = nullptr)
    {
        int ok = 0;
        map_.check(gem_costmap_clear_footprint(map_.handle(), id_, &pose, xy(spec), static_cast<int>(spec.size()), ptr(bounds), &ok),
                   "gem_costmap_clear_footprint");
        return ok != 0;
    }
    // ObstacleLayer::updateBounds over the observations (gem_hip_obstacle.h): every clearing observation's rays free the cells they cross,
    // then every marking observation's records become LETHAL_OBSTACLE.  bounds nullptr: only enqueued.  Plans, searches and distance
    // grids made before it are stale afterwards.
    void observe(const std::vector<Observation>& observations, double layerMaxObstacleHeight = 2.0, Bounds* bounds = nullptr)
    {
        map_.check(gem_costmap_observe(map_.handle(), id_, observations.empty() ? nullptr : observations.data(), static_cast<int>(observations.size()),
                                       layerMaxObstacleHeight, ptr(bounds)), "gem_costmap_observe");
    }
    // VoxelLayer (gem_hip_voxlayer.h): a voxel column per cell, every voxel unknown; resetMaps, updateOrigin and rollTo then move the
    // columns with the bytes
    void attachVoxels(const VoxelConfig& config = VoxelConfig())
    { map_.check(gem_costmap_voxels_create(map_.handle(), id_, &config), "gem_costmap_voxels_create"); }
    // VoxelLayer::updateBounds over the observations: 3-D rays clear the voxels they cross, then the records mark theirs; a cell becomes
    // FREE_SPACE, NO_INFORMATION or LETHAL_OBSTACLE by its column's bit counts.  bounds nullptr: only enqueued.  Plans, searches and
    // distance grids made before it are stale afterwards.
    void voxelObserve(const std::vector<Observation>& observations, double layerMaxObstacleHeight = 2.0, Bounds* bounds = nullptr)
    {
        map_.check(gem_costmap_voxel_observe(map_.handle(), id_, observations.empty() ? nullptr : observations.data(), static_cast<int>(observations.size()),
                                             layerMaxObstacleHeight, ptr(bounds)), "gem_costmap_voxel_observe");
    }
    // the window's columns, row-major, (maxI - minI) per row: bit z "not known free", bit 16 + z "marked"
    std::vector<unsigned> readVoxels(int minI, int minJ, int maxI, int maxJ) const
    {
        const size_t w = maxI > minI ? static_cast<size_t>(maxI - minI) : 0, rows = maxJ > minJ ? static_cast<size_t>(maxJ - minJ) : 0;
        std::vector<unsigned> v(w * rows);
        map_.check(gem_costmap_voxels_read(map_.handle(), id_, minI, minJ, maxI, maxJ, v.empty() ? nullptr : v.data(), w), "gem_costmap_voxels_read");
        return v;
    }
    void writeVoxels(int minI, int minJ, int maxI, int maxJ, const std::vector<unsigned>& columns)
    {
        const size_t w = maxI > minI ? static_cast<size_t>(maxI - minI) : 0, rows = maxJ > minJ ? static_cast<size_t>(maxJ - minJ) : 0;
        if (columns.size() != w * rows) throw Error(GEM_ERR_INVALID, "Costmap::writeVoxels: one column per cell of the window");
        map_.check(gem_costmap_voxels_write(map_.handle(), id_, minI, minJ, maxI, maxJ, columns.empty() ? nullptr : columns.data(), w), "gem_costmap_voxels_write");
    }
    // CostmapModel::footprintCost of every pose: -3 off the map, -2 unknown, -1 lethal, else the largest cost on the outline
    std::vector<int> footprintCost(const std::vector<FootprintPose>& poses, const std::vector<FootprintPoint>& spec, int flags = 0) const
    {
        std::vector<int> cost(poses.size());
        map_.check(gem_costmap_footprint_cost(map_.handle(), id_, poses.empty() ? nullptr : poses.data(), static_cast<long long>(poses.size()),
                                              xy(spec), static_cast<int>(spec.size()), flags, cost.empty() ? nullptr : cost.data()),
                   "gem_costmap_footprint_cost");
        return cost;
    }
    // trajectories of posesPerTrajectory consecutive poses: the first negative pose cost, else the maximum (GEM_FOOTPRINT_SUM: the
    // sum), as ObstacleCostFunction::scoreTrajectory; poseCosts, if given, receives every pose's footprintCost
    std::vector<int> scoreTrajectories(const std::vector<FootprintPose>& poses, int posesPerTrajectory, const std::vector<FootprintPoint>& spec,
                                       int flags = 0, std::vector<int>* poseCosts = nullptr) const
    {
        if (posesPerTrajectory < 1 || poses.size() % static_cast<size_t>(posesPerTrajectory))
            throw Error(GEM_ERR_INVALID, "Costmap::scoreTrajectories: the poses are not a whole number of trajectories");
        std::vector<int> cost(poses.size() / static_cast<size_t>(posesPerTrajectory));
        if (poseCosts) poseCosts->assign(poses.size(), 0);
        map_.check(gem_costmap_score_trajectories(map_.handle(), id_, poses.empty() ? nullptr : poses.data(), static_cast<long long>(cost.size()),
                                                  posesPerTrajectory, xy(spec), static_cast<int>(spec.size()), flags,
                                                  poseCosts && !poseCosts->empty() ? poseCosts->data() : nullptr, cost.empty() ? nullptr : cost.data()),
                   "gem_costmap_score_trajectories");
        return cost;
    }

    // InflationLayer::updateCosts around the LETHAL_OBSTACLE cells inside [minI, maxI) x [minJ, maxJ) widened by the cell radius, from
    // the exact nearest lethal cell (the library's brushfire can over-estimate a distance: gem_hip_inflate.h).  Only enqueued.
    void inflate(const InflationParams& params, int minI, int minJ, int maxI, int maxJ)
    { map_.check(gem_costmap_inflate(map_.handle(), id_, &params, minI, minJ, maxI, maxJ), "gem_costmap_inflate"); }
    void inflate(const InflationParams& params)
    {
        const gem_costmap_config c = geometry();
        inflate(params, 0, 0, static_cast<int>(c.size_x), static_cast<int>(c.size_y));
    }
    // Costmap2D::resetMap(x0, y0, xn, yn): what LayeredCostmap::updateMap does to the master before the layers write
    void resetWindow(int x0, int y0, int xn, int yn)
    { map_.check(gem_costmap_reset_window(map_.handle(), id_, x0, y0, xn, yn), "gem_costmap_reset_window"); }

    // base_local_planner's MapGrid (gem_hip_mapgrid.h): the path and goal distance grids from a global plan through the cells that are
    // not 253, 254 or 255, as the costmap is when the call runs on the stream.  Only enqueued.
    enum MapGridWhich { PathGrid = GEM_MAPGRID_PATH, GoalGrid = GEM_MAPGRID_GOAL };
    struct MapGrid {
        std::vector<int> dist;          // size_y rows of size_x
        bool started = false;           // a point of the plan was accepted
        int goalX = -1, goalY = -1;     // the local goal's cell
    };
    // MapGrid::adjustPlanResolution (host only)
    static std::vector<FootprintPoint> adjustPlan(const std::vector<FootprintPoint>& plan, double resolution)
    {
        long long n = 0;
        if (gem_mapgrid_adjust_plan(xy(plan), static_cast<long long>(plan.size()), resolution, nullptr, 0, &n) != GEM_OK)
            throw Error(GEM_ERR_INVALID, "Costmap::adjustPlan: an unusable coordinate or resolution, or more than 2^20 points");
        std::vector<FootprintPoint> out(static_cast<size_t>(n));
        if (n) gem_mapgrid_adjust_plan(xy(plan), static_cast<long long>(plan.size()), resolution, &out.front().x, n, nullptr);
        return out;
    }
    void prepareMapGrid(const std::vector<FootprintPoint>& plan, int which = GEM_MAPGRID_PATH | GEM_MAPGRID_GOAL)
    { map_.check(gem_costmap_mapgrid_prepare(map_.handle(), id_, xy(plan), static_cast<long long>(plan.size()), which), "gem_costmap_mapgrid_prepare"); }
    // The same grids on a costmap of any size (gem_costmap_mapgrid_prepare_tiled): relaxed tile by tile in global memory.  Waits.
    MapGridTiledStatus prepareMapGridTiled(const std::vector<FootprintPoint>& plan, int which = GEM_MAPGRID_PATH | GEM_MAPGRID_GOAL)
    {
        gem_mapgrid_tiled_status st{};
        map_.check(gem_costmap_mapgrid_prepare_tiled(map_.handle(), id_, xy(plan), static_cast<long long>(plan.size()), which, &st),
                   "gem_costmap_mapgrid_prepare_tiled");
        return MapGridTiledStatus::from(st);
    }
    // waits
    MapGrid mapGrid(MapGridWhich which) const
    {
        const gem_costmap_config c = geometry();
        MapGrid g;
        g.dist.assign(static_cast<size_t>(c.size_x) * c.size_y, 0);
        int started = 0, goal[2] = {-1, -1};
        map_.check(gem_costmap_mapgrid_read(map_.handle(), id_, which, g.dist.data(), &started, goal), "gem_costmap_mapgrid_read");
        g.started = started != 0; g.goalX = goal[0]; g.goalY = goal[1];
        return g;
    }
    // MapGridCostFunction::scoreTrajectory over trajectories of posesPerTrajectory consecutive poses: -4 off the map, with
    // GEM_MAPGRID_STOP_ON_FAILURE -3 / -2 on an obstacle / unreachable cell, else the last pose's distance (GEM_MAPGRID_SUM: the sum).
    // The poses' cos / sin are the host's (FootprintPose::fromYaw); xshift moves the scored point along the heading (goal_front,
    // alignment); there is no yshift.
    std::vector<long long> scoreMapGrid(MapGridWhich which, const std::vector<FootprintPose>& poses, int posesPerTrajectory, double xshift = 0.0,
                                        int flags = 0) const
    {
        if (posesPerTrajectory < 1 || poses.size() % static_cast<size_t>(posesPerTrajectory))
            throw Error(GEM_ERR_INVALID, "Costmap::scoreMapGrid: the poses are not a whole number of trajectories");
        std::vector<long long> cost(poses.size() / static_cast<size_t>(posesPerTrajectory));
        map_.check(gem_costmap_mapgrid_score(map_.handle(), id_, which, poses.empty() ? nullptr : poses.data(), static_cast<long long>(cost.size()),
                                             posesPerTrajectory, xshift, flags, cost.empty() ? nullptr : cost.data()),
                   "gem_costmap_mapgrid_score");
        return cost;
    }

    // The FRONT grid (gem_hip_critics.h): the goal grid of the caller's front plan (its last point already moved forward) in a slot of
    // its own, for DWA's goal_front critic; PATH and GOAL are not touched.  Only enqueued; mapGridFront waits.
    void prepareMapGridFront(const std::vector<FootprintPoint>& plan)
    { map_.check(gem_costmap_mapgrid_prepare_front(map_.handle(), id_, xy(plan), static_cast<long long>(plan.size())), "gem_costmap_mapgrid_prepare_front"); }
    // ... on a costmap of any size (gem_costmap_mapgrid_prepare_front_tiled).  Waits.
    MapGridTiledStatus prepareMapGridFrontTiled(const std::vector<FootprintPoint>& plan)
    {
        gem_mapgrid_tiled_status st{};
        map_.check(gem_costmap_mapgrid_prepare_front_tiled(map_.handle(), id_, xy(plan), static_cast<long long>(plan.size()), &st),
                   "gem_costmap_mapgrid_prepare_front_tiled");
        return MapGridTiledStatus::from(st);
    }
    MapGrid mapGridFront() const
    {
        const gem_costmap_config c = geometry();
        MapGrid g;
        g.dist.assign(static_cast<size_t>(c.size_x) * c.size_y, 0);
        int started = 0, goal[2] = {-1, -1};
        map_.check(gem_costmap_mapgrid_read_front(map_.handle(), id_, g.dist.data(), &started, goal), "gem_costmap_mapgrid_read_front");
        g.started = started != 0; g.goalX = goal[0]; g.goalY = goal[1];
        return g;
    }
    // The global plan from the world point start to goal over the costmap's bytes as they are when the call runs on the stream
    // (gem_hip_navplan.h); weights empty: NavPlan::weights().  Waits.  potential() reads the last plan's potential back, size_y rows of
    // size_x, GEM_NAV_UNREACHED where the search did not come.
    NavPlan navPlan(const FootprintPoint& start, const FootprintPoint& goal, const std::vector<int>& weights = {}, bool outline = true)
    {
        const std::vector<int> w = weights.empty() ? NavPlan::weights() : weights;
        if (w.size() != 256) throw Error(GEM_ERR_INVALID, "Costmap::navPlan: the weight table has 256 entries");
        NavPlan p;
        const int flags = outline ? GEM_NAV_OUTLINE : 0;
        map_.check(gem_costmap_navplan(map_.handle(), id_, &start.x, &goal.x, w.data(), flags, nullptr, 0, &p.status), "gem_costmap_navplan");
        p.found = p.status.found != 0;
        std::vector<int> cells(static_cast<size_t>(p.status.n_path));
        map_.check(gem_costmap_navplan_read(map_.handle(), id_, nullptr, cells.empty() ? nullptr : cells.data(), static_cast<long long>(cells.size())),
                   "gem_costmap_navplan_read");
        const gem_costmap_config c = geometry();
        p.path.reserve(cells.size());
        for (int cell : cells)                                // cell centres, in double, as the C entry computes them
            p.path.push_back(FootprintPoint{c.origin_x + (static_cast<double>(cell % static_cast<int>(c.size_x)) + 0.5) * c.resolution,
                                            c.origin_y + (static_cast<double>(cell / static_cast<int>(c.size_x)) + 0.5) * c.resolution});
        return p;
    }
    // navPlan on the QUADRATIC potential (gem_hip_navquad.h): the two-axis update in exact integers, order-free, nowhere above the
    // linear potential; weights at most 462.  The plan takes the linear plan's place: potential(), navPlanTo, navPaths and the frontier
    // search work on it.  Waits.
    NavPlan navPlanQuadratic(const FootprintPoint& start, const FootprintPoint& goal, const std::vector<int>& weights = {}, bool outline = true)
    {
        const std::vector<int> w = weights.empty() ? NavPlan::weights() : weights;
        if (w.size() != 256) throw Error(GEM_ERR_INVALID, "Costmap::navPlanQuadratic: the weight table has 256 entries");
        NavPlan p;
        const int flags = outline ? GEM_NAV_OUTLINE : 0;
        map_.check(gem_costmap_navplan_quadratic(map_.handle(), id_, &start.x, &goal.x, w.data(), flags, nullptr, 0, &p.status),
                   "gem_costmap_navplan_quadratic");
        p.found = p.status.found != 0;
        std::vector<int> cells(static_cast<size_t>(p.status.n_path));
        map_.check(gem_costmap_navplan_read(map_.handle(), id_, nullptr, cells.empty() ? nullptr : cells.data(), static_cast<long long>(cells.size())),
                   "gem_costmap_navplan_read");
        const gem_costmap_config c = geometry();
        p.path.reserve(cells.size());
        for (int cell : cells)                                // cell centres, in double, as the C entry computes them
            p.path.push_back(FootprintPoint{c.origin_x + (static_cast<double>(cell % static_cast<int>(c.size_x)) + 0.5) * c.resolution,
                                            c.origin_y + (static_cast<double>(cell / static_cast<int>(c.size_x)) + 0.5) * c.resolution});
        return p;
    }
    std::vector<int> potential() const
    {
        const gem_costmap_config c = geometry();
        std::vector<int> pot(static_cast<size_t>(c.size_x) * c.size_y, 0);
        map_.check(gem_costmap_navplan_read(map_.handle(), id_, pot.data(), nullptr, 0), "gem_costmap_navplan_read");
        return pot;
    }
    // The path from the last plan's start to another goal on the last plan's potential, which stays as it is (gem_hip_frontier.h): one
    // walk, no second search.  Waits.
    NavPlan navPlanTo(const FootprintPoint& goal)
    {
        NavPlan p;
        map_.check(gem_costmap_navplan_goal(map_.handle(), id_, &goal.x, nullptr, 0, &p.status), "gem_costmap_navplan_goal");
        p.found = p.status.found != 0;
        std::vector<int> cells(static_cast<size_t>(p.status.n_path));
        map_.check(gem_costmap_navplan_read(map_.handle(), id_, nullptr, cells.empty() ? nullptr : cells.data(), static_cast<long long>(cells.size())),
                   "gem_costmap_navplan_read");
        const gem_costmap_config c = geometry();
        p.path.reserve(cells.size());
        for (int cell : cells)
            p.path.push_back(FootprintPoint{c.origin_x + (static_cast<double>(cell % static_cast<int>(c.size_x)) + 0.5) * c.resolution,
                                            c.origin_y + (static_cast<double>(cell / static_cast<int>(c.size_x)) + 0.5) * c.resolution});
        return p;
    }
    // Paths from the last plan's start to up to 1024 goals on the last plan's potential, in one launch, one wave per goal
    // (gem_hip_navpath.h); form GEM_NAVPATH_GRADIENT or GEM_NAVPATH_GRID.  The potential, the last path and status and the frontier
    // search stay as they are.  Waits.  The walks' cell coordinates p are reversed and become origin + (p + 0.5) * resolution, in double.
    NavPaths navPaths(const std::vector<FootprintPoint>& goals, int form = GEM_NAVPATH_GRADIENT, int maxPoints = 4096)
    {
        // the library's limits, before anything is sized by them: 1 .. 1024 goals, 2 .. 2^20 points, at most 2^24 points in all
        if (goals.empty() || goals.size() > 1024 || maxPoints < 2 || maxPoints > (1 << 20) || goals.size() * static_cast<size_t>(maxPoints) > (size_t(1) << 24))
            throw Error(GEM_ERR_INVALID, "Costmap::navPaths: goals outside 1 .. 1024, maxPoints outside 2 .. 2^20, or more than 2^24 points in all");
        NavPaths r;
        r.results.resize(goals.size());
        std::vector<float> pts(goals.size() * static_cast<size_t>(maxPoints) * 2);
        map_.check(gem_costmap_navplan_paths(map_.handle(), id_, &goals[0].x, static_cast<int>(goals.size()), form, maxPoints, pts.data(), r.results.data()),
                   "gem_costmap_navplan_paths");
        const gem_costmap_config c = geometry();
        r.paths.resize(goals.size());
        for (size_t g = 0; g < goals.size(); ++g) {
            const float* p = pts.data() + g * static_cast<size_t>(maxPoints) * 2;
            for (int i = r.results[g].n_points - 1; i >= 0; --i)
                r.paths[g].push_back(FootprintPoint{c.origin_x + (static_cast<double>(p[2 * i]) + 0.5) * c.resolution,
                                                    c.origin_y + (static_cast<double>(p[2 * i + 1]) + 0.5) * c.resolution});
        }
        return r;
    }
    // Frontier search over the costmap's bytes and the potential of its last plan (gem_hip_frontier.h).  Waits.  readFrontiers() reads
    // the last search's kept frontiers back in ascending root order and, with labels, the label grid (a cell's root, -1 for a cell
    // that is no frontier cell).
    FrontierSearch frontiers(double minFrontierSize = 0.0, double potentialScale = 1.0, double gainScale = 1.0)
    {
        const gem_frontier_params prm{minFrontierSize, potentialScale, gainScale};
        FrontierSearch s;
        map_.check(gem_costmap_frontiers(map_.handle(), id_, &prm, &s.status), "gem_costmap_frontiers");
        lastKept_ = s.status.n_kept;
        s.found = s.status.best >= 0;
        if (s.found) s.best = frontierOf(s.status.best_frontier);
        return s;
    }
    std::vector<Frontier> readFrontiers(std::vector<int>* labels = nullptr) const
    {
        const gem_costmap_config c = geometry();
        if (labels) labels->assign(static_cast<size_t>(c.size_x) * c.size_y, 0);
        std::vector<gem_frontier> rec(static_cast<size_t>(lastKept_));
        map_.check(gem_costmap_frontiers_read(map_.handle(), id_, rec.empty() ? nullptr : rec.data(), static_cast<long long>(rec.size()),
                                              labels ? labels->data() : nullptr),
                   "gem_costmap_frontiers_read");
        std::vector<Frontier> out;
        out.reserve(rec.size());
        for (const gem_frontier& r : rec) out.push_back(frontierOf(r));
        return out;
    }

    // SimpleScoredSamplingPlanner's scoreTrajectory + findBestTrajectory over trajectories of posesPerTrajectory pose slots: the critics
    // in order, ext = the external critics' raw scores [columns][trajectories], trajLen (empty: all) the poses each trajectory uses.
    // The smallest total among the valid trajectories wins, ties to the smallest index.  Waits.
    BestTrajectory bestTrajectory(const std::vector<Critic>& critics, const std::vector<FootprintPose>& poses, int posesPerTrajectory,
                                  const std::vector<FootprintPoint>& spec, const std::vector<double>& ext = {}, const std::vector<int>& trajLen = {},
                                  std::vector<double>* totals = nullptr) const
    {
        if (posesPerTrajectory < 1 || poses.size() % static_cast<size_t>(posesPerTrajectory))
            throw Error(GEM_ERR_INVALID, "Costmap::bestTrajectory: the poses are not a whole number of trajectories");
        const size_t n = poses.size() / static_cast<size_t>(posesPerTrajectory);
        if ((!trajLen.empty() && trajLen.size() != n) || (n ? ext.size() % n != 0 : !ext.empty()))
            throw Error(GEM_ERR_INVALID, "Costmap::bestTrajectory: one length per trajectory, whole columns of external scores");
        if (totals) totals->assign(n, 0.0);
        BestTrajectory b;
        map_.check(gem_costmap_best_trajectory(map_.handle(), id_, critics.empty() ? nullptr : critics.data(), static_cast<int>(critics.size()),
                                               poses.empty() ? nullptr : poses.data(), trajLen.empty() ? nullptr : trajLen.data(),
                                               static_cast<long long>(n), posesPerTrajectory, xy(spec), static_cast<int>(spec.size()),
                                               ext.empty() ? nullptr : ext.data(), n ? static_cast<int>(ext.size() / n) : 0,
                                               totals && n ? totals->data() : nullptr, &b),
                   "gem_costmap_best_trajectory");
        return b;
    }
    // The trajectories of the plan generated on the device (gem_hip_trajgen.h), then bestTrajectory over them: an external critic's
    // column 0 / 1 is the generated oscillation / twirling score.  One call, three launches, 32 bytes back.  Waits.
    BestTrajectory dwaBest(const std::vector<Critic>& critics, const TrajectoryPlan& plan, const TrajectoryState& s, int posesPerTrajectory,
                           const std::vector<FootprintPoint>& spec, std::vector<double>* totals = nullptr) const
    {
        const size_t n = static_cast<size_t>(plan.n_traj > 0 ? plan.n_traj : 0);
        if (totals) totals->assign(n, 0.0);
        BestTrajectory b;
        map_.check(gem_costmap_dwa_best(map_.handle(), id_, critics.empty() ? nullptr : critics.data(), static_cast<int>(critics.size()), &plan,
                                        s.pos, s.vel, posesPerTrajectory, xy(spec), static_cast<int>(spec.size()),
                                        totals && n ? totals->data() : nullptr, &b),
                   "gem_costmap_dwa_best");
        return b;
    }
    // createTrajectories on this costmap (gem_hip_rollout.h): every candidate of the plan rolled out against the bytes and the PATH and
    // GOAL grids (prepareMapGrid first), then the pick.  One call, two launches, 64 bytes back.  Waits.
    RolloutBest rolloutBest(const RolloutPlan& plan, const RolloutState& s, int stateFlags, const std::vector<FootprintPoint>& spec, int flags = 0,
                            std::vector<double>* cost = nullptr, std::vector<int>* ahead = nullptr) const
    {
        const size_t n = static_cast<size_t>(plan.n_cand > 0 ? plan.n_cand : 0);
        if (cost) cost->assign(n, 0.0);
        if (ahead) ahead->assign(n, -1);
        RolloutBest b;
        map_.check(gem_costmap_rollout_best(map_.handle(), id_, &plan, s.pos, s.vel, stateFlags, xy(spec), static_cast<int>(spec.size()), flags,
                                            cost ? cost->data() : nullptr, ahead ? ahead->data() : nullptr, &b),
                   "gem_costmap_rollout_best");
        return b;
    }

private:
    static_assert(sizeof(Bounds) == 4 * sizeof(double), "bounds are four packed doubles");
    static_assert(sizeof(FootprintPoint) == 2 * sizeof(double), "a spec is packed pairs of doubles");
    static double* ptr(Bounds* b) { return b ? &b->min_x : nullptr; }
    static const double* xy(const std::vector<FootprintPoint>& spec) { return spec.empty() ? nullptr : &spec.front().x; }
    Frontier frontierOf(const gem_frontier& r) const
    {
        const gem_costmap_config c = geometry();
        Frontier f;
        f.record = r; f.originX = c.origin_x; f.originY = c.origin_y; f.resolution = c.resolution;
        return f;
    }
    ElevationMap& map_;
    int id_ = -1;
    int lastKept_ = 0;                                       // the kept list's length of the last frontiers() of this object
};

// ---------------------------------------------------------------------------------------------
// The pcl/VoxelGrid nodelets of the launch files (filter.launch, filter_kitti.launch) on the device (gem_voxel_*): the setters
// of pcl::VoxelGrid; each addStage() appends the current settings as one more stage of the chain (at most four).  The contract
// is in gem_hip.h (gem_voxel_device).
// ---------------------------------------------------------------------------------------------
class VoxelGrid {
public:
    VoxelGrid() { reset(); }
    void setLeafSize(float lx, float ly, float lz) { cur_.leaf[0] = lx; cur_.leaf[1] = ly; cur_.leaf[2] = lz; }
    // "" (none), "x", "y", "z" or "intensity"
    void setFilterFieldName(const std::string& name)
    {
        static const std::map<std::string, int> fields = {{"", GEM_VOXEL_FIELD_NONE}, {"x", GEM_VOXEL_FIELD_X}, {"y", GEM_VOXEL_FIELD_Y},
                                                          {"z", GEM_VOXEL_FIELD_Z}, {"intensity", GEM_VOXEL_FIELD_INTENSITY}};
        const auto it = fields.find(name);
        if (it == fields.end()) throw Error(GEM_ERR_INVALID, "VoxelGrid: filter field " + name + " (none, x, y, z or intensity)");
        cur_.field = it->second;
    }
    void setFilterLimits(double limitMin, double limitMax) { cur_.limit_min = limitMin; cur_.limit_max = limitMax; }
    void setFilterLimitsNegative(bool negative) { cur_.limit_negative = negative ? 1 : 0; }
    // the current settings become the next stage; the setters then start from PCL's defaults again
    VoxelGrid& addStage()
    {
        if (stages_.size() >= 4) throw Error(GEM_ERR_INVALID, "VoxelGrid: at most four stages");
        stages_.push_back(cur_);
        reset();
        return *this;
    }
    const std::vector<gem_voxel_params>& stages() const { return stages_; }
    // n XYZI points on the device -> d_xyzi_out (n points: the m centroids, then the NaN tail), m in *d_count (device int);
    // enqueued on the map's stream.  Without addStage() the current settings are the one stage.
    void filterDevice(ElevationMap& map, const void* d_xyzi, int n, void* d_xyzi_out, void* d_count, const void* d_rgb = nullptr,
                      void* d_rgb_out = nullptr) const
    {
        const std::vector<gem_voxel_params> s = chain();
        map.check(gem_voxel_device(map.handle(), s.data(), static_cast<int>(s.size()), n, d_xyzi, d_rgb, d_xyzi_out, d_rgb_out, d_count),
                  "gem_voxel_device");
    }
    // ElevationMap::add behind the filter: host XYZI (gem_add_voxel) or device XYZI (addToDevice, gem_add_voxel_device)
    void addTo(ElevationMap& map, const gem_frame_params& frame, const float* xyzi, int n, const uint32_t* rgb = nullptr) const
    {
        const std::vector<gem_voxel_params> s = chain();
        map.check(gem_add_voxel(map.handle(), &frame, s.data(), static_cast<int>(s.size()), n, xyzi, rgb), "gem_add_voxel");
    }
    void addToDevice(ElevationMap& map, const gem_frame_params& frame, const void* d_xyzi, int n, const void* d_rgb = nullptr) const
    {
        const std::vector<gem_voxel_params> s = chain();
        map.check(gem_add_voxel_device(map.handle(), &frame, s.data(), static_cast<int>(s.size()), n, d_xyzi, d_rgb), "gem_add_voxel_device");
    }
    static VoxelGrid filterLaunch()                  // filter.launch
    {
        VoxelGrid v;
        v.setLeafSize(0.1f, 0.1f, 0.1f); v.setFilterFieldName("x"); v.setFilterLimits(-10.0, 10.0);
        return v.addStage();
    }
    static VoxelGrid filterKittiLaunch()             // filter_kitti.launch
    {
        VoxelGrid v;
        const char* f[3] = {"x", "z", "y"};
        const double lim[3] = {40.0, 25.0, 40.0};
        for (int i = 0; i < 3; ++i) { v.setLeafSize(0.2f, 0.2f, 0.2f); v.setFilterFieldName(f[i]); v.setFilterLimits(-lim[i], lim[i]); v.addStage(); }
        return v;
    }

private:
    void reset()
    {
        cur_ = gem_voxel_params{};
        cur_.leaf[0] = cur_.leaf[1] = cur_.leaf[2] = 0.01f;                  // (pcl::VoxelGrid's default leaf is 0: set one)
        cur_.field = GEM_VOXEL_FIELD_NONE;
        cur_.limit_min = -static_cast<double>(std::numeric_limits<float>::max());
        cur_.limit_max = static_cast<double>(std::numeric_limits<float>::max());
    }
    std::vector<gem_voxel_params> chain() const { return stages_.empty() ? std::vector<gem_voxel_params>{cur_} : stages_; }
    gem_voxel_params cur_{};
    std::vector<gem_voxel_params> stages_;
};

inline bool SensorProcessorBase::process(ElevationMap& map, const PointXYZRGBICT* cloud, int n,
                                         int* point_colorR, int* point_colorG, int* point_colorB, int* point_index,
                                         float* point_intensity, float* point_height, float* point_var)
{
    // AoS -> SoA split of GPUPointCloudprocess (SensorProcessorBase.cpp:160-169)
    std::vector<float> x(n), y(n), z(n);
    for (int i = 0; i < n; ++i) {
        x[i] = cloud[i].x; y[i] = cloud[i].y; z[i] = cloud[i].z;
        point_colorR[i] = cloud[i].r; point_colorG[i] = cloud[i].g; point_colorB[i] = cloud[i].b;
        point_intensity[i] = cloud[i].intensity;
    }
    const gem_frame_params p = frameParams();
    const int rc = gem_process_points(map.handle(), &p, n, x.data(), y.data(), z.data(), nullptr, 0,
                                      point_index, point_var, nullptr, nullptr, point_height);     // SensorProcessorBase.cpp:208
    return rc == GEM_OK;
}

inline void SensorProcessorBase::addDepth(ElevationMap& map, const DepthImage& image, const void* depth, const void* color)
{
    originalWidth_ = image.width;                                                            // StereoSensorProcessor.cpp:41
    const gem_frame_params p = frameParams();
    const gem_clean_params c = cleanParams();
    map.addDepth(p, image, depth, color, &c);
}

inline int SensorProcessorBase::processRaw(ElevationMap& map, const PointXYZRGBICT* cloud, int n, int width,
                                           int* point_colorR, int* point_colorG, int* point_colorB, int* point_index,
                                           float* point_intensity, float* point_height, float* point_var)
{
    if (n < 0 || (n > 0 && !cloud)) return -1;
    originalWidth_ = width;                                                                  // StereoSensorProcessor.cpp:41
    std::vector<float> x(n), y(n), z(n);
    for (int i = 0; i < n; ++i) { x[i] = cloud[i].x; y[i] = cloud[i].y; z[i] = cloud[i].z; }
    std::vector<int> orig(n > 0 ? n : 1);
    const gem_frame_params p = frameParams();
    const gem_clean_params c = cleanParams();
    int kept = 0;
    const int rc = gem_process_points_raw(map.handle(), &p, &c, n, x.data(), y.data(), z.data(), &kept, orig.data(),
                                          point_index, point_var, nullptr, nullptr, point_height);
    if (rc != GEM_OK) return -1;
    for (int k = 0; k < kept; ++k) {                                                         // the kept points' fields (SPB.cpp:160-169)
        const PointXYZRGBICT& q = cloud[orig[k]];
        if (point_colorR) point_colorR[k] = q.r;
        if (point_colorG) point_colorG[k] = q.g;
        if (point_colorB) point_colorB[k] = q.b;
        if (point_intensity) point_intensity[k] = q.intensity;
    }
    return kept;
}

// ---------------------------------------------------------------------------------------------
// RobotMotionMapUpdater (RobotMotionMapUpdater.cpp:42-145), plain arrays instead of kindr types.
// Rotations follow kindr-1.x conventions: C_IB maps base to inertial coordinates.
// ---------------------------------------------------------------------------------------------
class RobotMotionMapUpdater {
public:
    explicit RobotMotionMapUpdater(double covarianceScale = 1.0) : covarianceScale_(covarianceScale)
    {
        previousReducedCovariance_.fill(0.0);
        previousRotation_ = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        previousPosition_ = {0, 0, 0};
    }

    // returns the variance increment handed to Mapvar_update (RobotMotionMapUpdater.cpp:80-81)
    float update(ElevationMap& map, const Vec3& position, const Mat3& R_IB, const std::array<double, 36>& poseCovariance,
                 const Mat3& mapRotation = {1, 0, 0, 0, 1, 0, 0, 0, 1})
    {
        const float u = compute(position, R_IB, poseCovariance, mapRotation);
        map.update(u);
        return u;
    }

    float compute(const Vec3& position, const Mat3& R, const std::array<double, 36>& poseCovariance, const Mat3& mapRotation)
    {
        // computeReducedCovariance (:92-109)
        const double yaw = std::atan2(R[3], R[0]);
        const double pitch = std::atan2(-R[6], std::sqrt(R[0] * R[0] + R[3] * R[3]));
        const double tp = std::tan(pitch);
        double J[4][6] = {};
        J[0][0] = J[1][1] = J[2][2] = 1.0;
        J[3][3] = std::cos(yaw) * tp; J[3][4] = std::sin(yaw) * tp; J[3][5] = 1.0;
        double reduced[4][4] = {};
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) s += J[i][a] * covarianceScale_ * poseCovariance[a * 6 + b] * J[j][b];
            reduced[i][j] = s;
        }
        // computeRelativeCovariance (:111-145)
        double c = 0.5 * (R[0] + R[4] + R[8] - 1.0); c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
        const double angle = std::acos(c);
        const double wz = 0.5 * (R[3] - R[1]);
        const double rz = angle < 1e-12 ? wz : wz * angle / std::sin(angle);
        const double Rt[3][3] = {{std::cos(rz), -std::sin(rz), 0}, {std::sin(rz), std::cos(rz), 0}, {0, 0, 1}};
        const double dp[3] = {position[0] - previousPosition_[0], position[1] - previousPosition_[1], position[2] - previousPosition_[2]};
        double v[3];
        for (int i = 0; i < 3; ++i) v[i] = previousRotation_[i] * dp[0] + previousRotation_[3 + i] * dp[1] + previousRotation_[6 + i] * dp[2];
        double Rv[3];
        for (int i = 0; i < 3; ++i) Rv[i] = Rt[i][0] * v[0] + Rt[i][1] * v[1] + Rt[i][2] * v[2];
        double F[4][4] = {{1, 0, 0, -Rv[1]}, {0, 1, 0, Rv[0]}, {0, 0, 1, 0}, {0, 0, 0, 1}};
        double G[4][4] = {}, Gt[4][4] = {};
        G[3][3] = Gt[3][3] = 1.0;
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { G[i][j] = Rt[j][i]; Gt[i][j] = Rt[i][j]; }
        double D[4][4];
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) s += F[i][a] * previousReducedCovariance_[a * 4 + b] * F[j][b];
            D[i][j] = reduced[i][j] - s;
        }
        double rel[4][4];
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) s += G[i][a] * D[a][b] * Gt[b][j];
            rel[i][j] = s;
        }
        // update (:58-80): R_B_M = R_I_B^T R_I_M;  J_r = -R_B_M^T;  var = (J_r Sigma J_r^T)_zz
        const Mat3 RBM = mul(transposed(R), mapRotation);
        double Jr[3][3];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Jr[i][j] = -RBM[j * 3 + i];
        double out = 0.0;
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) out += Jr[2][a] * rel[a][b] * Jr[2][b];
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) previousReducedCovariance_[i * 4 + j] = reduced[i][j];
        previousPosition_ = position; previousRotation_ = R;
        return static_cast<float>(out);
    }

private:
    double covarianceScale_;
    std::array<double, 16> previousReducedCovariance_;
    Vec3 previousPosition_;
    Mat3 previousRotation_;
};

} // namespace gem
