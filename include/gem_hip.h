/*
 * gem_hip.h -- C ABI of libgem_hip.so: the MI355X (gfx950) implementation of GEM's
 * point-cloud -> elevation-grid hot path.  This is the drop-in boundary: plain pointers and
 * sizes, no C++ / Eigen / torch types.  Each entry point cites the reference interface it
 * replaces (GPU = elevation_mapping/elevation_mapping/cuda/gpu_process.cu, EMg.cpp =
 * .../src/ElevationMapping.cpp, SPB.cpp = .../src/sensor_processors/SensorProcessorBase.cpp,
 * RMU.cpp = .../src/RobotMotionMapUpdater.cpp).  The nine C++-linkage symbols the unmodified
 * ROS node links against are re-created on top of this ABI in include/gem/gem_compat_eigen.hpp.
 *
 * Conventions
 *   - every function returns GEM_OK (0) or a negative gem_status; gem_last_error() gives text.
 *   - one gem_handle == one robot-centric map (the reference keeps this as hidden process-global
 *     __device__ state, GPU:20-33); a handle is internally locked, so the reference's
 *     {Process_points -> Fuse} || {Mapvar_update} thread pair (EMg.cpp:391-394) is safe.
 *   - host-pointer entry points copy in/out and are synchronous w.r.t. the caller's buffers;
 *     *_device entry points take device pointers, enqueue on the handle's stream and return.
 *   - there is NO CPU fallback: without a HIP device gem_create fails with GEM_ERR_NO_DEVICE.
 */
#ifndef GEM_HIP_H
#define GEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEM_ABI_VERSION 9

typedef enum gem_status {
    GEM_OK = 0,
    GEM_ERR_INVALID = -1,      /* bad argument */
    GEM_ERR_NO_DEVICE = -2,    /* no HIP device / HIP runtime error at create */
    GEM_ERR_HIP = -3,          /* HIP runtime error (text in gem_last_error) */
    GEM_ERR_NOMEM = -4,
    GEM_ERR_COMM = -5          /* RCCL error */
} gem_status;

/* sensor noise models.  Laser is the only model on the reference's GPU path (GPU:403-425,
 * SPB.cpp:286-288); the others are the reference's CPU computeVariances() bodies
 * (StructuredLightSensorProcessor.cpp:121-153, StereoSensorProcessor.cpp:72-104,
 * PerfectSensorProcessor.cpp:74-102). */
enum { GEM_MODEL_LASER = 0, GEM_MODEL_STRUCTURED_LIGHT = 1, GEM_MODEL_STEREO = 2, GEM_MODEL_PERFECT = 3 };

/* map layers (device layout GPU:20-28; GridMap names EM.cpp:43-44) */
enum {
    GEM_LAYER_ELEVATION = 0, GEM_LAYER_VARIANCE = 1, GEM_LAYER_INTENSITY = 2, GEM_LAYER_TRAVER = 3,
    GEM_LAYER_LOWEST = 4, GEM_LAYER_COLOR_R = 5, GEM_LAYER_COLOR_G = 6, GEM_LAYER_COLOR_B = 7,
    GEM_LAYER_ROUGH = 8, GEM_LAYER_SLOPE = 9,      /* outputs of gem_map_feature (visualMap_ layers "rough", "slope", EM.cpp:44) */
    GEM_LAYER_COUNT = 10
};
/* GEM_LAYER_LOWEST is the reference's map_lowest: indexed by the GEOGRAPHIC cell [gx * L + gy] (GPU:430, 676-679), NOT by the
 * circular-buffer cell like the other layers, and not shifted by gem_move; the GRIDMAP layout does not apply to it. */
/* layouts for gem_get_layer / gem_set_layer */
enum {
    GEM_LAYOUT_STORAGE_ROWMAJOR = 0,   /* the reference's flat [storage_x * L + storage_y] arrays (EM.cpp:98-111)   */
    GEM_LAYOUT_GRIDMAP_COLMAJOR_NAN = 1 /* grid_map::Matrix (Eigen column-major, buffer order), NaN for empty cells */
};

typedef struct gem_map_config {
    int   length;                  /* cells per side, = length_in_x / resolution (EMg.cpp:195)                 */
    float resolution;              /* metres per cell (GPU:36)                                                 */
    float mahalanobis_threshold;   /* the reference uploads one (GPU:977) but uses the literal 5 (GPU:504): pass 5 */
    float variance_floor;          /* literal 0.0001 in the reference (GPU:500,533)                            */
    float obstacle_threshold;      /* GPU:940 4th argument: cells with traversability below it are ray-traced (GPU:712)     */
    int   strip_row0, strip_rows;  /* storage-row strip this handle owns (multi-GPU tiling); 0,0 = whole map   */
    int   device;                  /* HIP device ordinal; -1 = current device                                  */
} gem_map_config;

/* the hard-coded sensor-frame reject filter of GPU:393, parameterised; defaults 1.5,1.5,1.0,0.0 */
typedef struct gem_reject_filter {
    int   enabled;
    float box_x, box_y;            /* reject |x|<box_x && |y|<box_y */
    float band_y;                  /* reject |y|<band_y             */
    float plane_y;                 /* reject y>plane_y              */
} gem_reject_filter;

/* per-frame constants: exactly what SensorProcessorBase::GPUPointCloudprocess hands to
 * Process_points (SPB.cpp:171-208): transform, height window, model parameters, Jacobian pieces. */
typedef struct gem_frame_params {
    float  T[16];                  /* sensor->map, row-major (Eigen::Matrix4f Transform, SPB.cpp:175-179)      */
    double lower, upper;           /* relativeLower/UpperThreshold (SPB.cpp:183-184)                          */
    int    sensor_model;           /* GEM_MODEL_*                                                              */
    double sensor_params[8];       /* laser: min_radius, beam_angle, beam_constant (SPB.cpp:286-288);
                                      structured light: normal_factor_a..e, lateral_factor;
                                      stereo: p_1..p_5, lateral_factor, depth_to_disparity_factor            */
    float  sensor_jacobian[3];     /* SPB.cpp:275 */
    float  rotation_variance[9];   /* row-major; zero in the reference (SPB.cpp:202-204) */
    float  C_SB_T[9];              /* row-major, SPB.cpp:283 */
    float  P_mul_C_BM_T[3];        /* SPB.cpp:281-282 */
    float  B_r_BS_skew[9];         /* row-major, SPB.cpp:284 */
    gem_reject_filter filter;
    int    original_width;         /* stereo: image width for getI/getJ (StereoSensorProcessor.cpp:108-116)  */
} gem_frame_params;

typedef struct gem_handle gem_handle;

/* counters of the most recent add/fuse call (read back lazily; forces a stream sync) */
typedef struct gem_stats {
    long long points_in;
    long long points_binned;       /* accepted AND inside the map (and inside this handle's strip)             */
    long long cells_touched;       /* distinct cells that received >= 1 point                                  */
    float     ms_bin, ms_fuse;     /* accumulated kernel time of the two pipeline kernels since reset          */
    int       launches_bin, launches_fuse;
    float     ms_frame;            /* ... and of k_frame (fuse of the previous sweep + bin of the new one)     */
    int       launches_frame;      /* SWEEPS that passed through a k_frame launch: a launch that carries two   */
                                   /* adds 2, so ms_frame / launches_frame stays the device time per sweep     */
    float     ms_sort[6];          /* the sorted pipeline of big passes: count1, scan1, scatter1, count2, scan2, scatter2 */
    int       launches_sort;       /* passes through it                                                        */
    float     ms_walk;             /* ... and its k_fuse_walk                                                  */
    int       launches_walk;
} gem_stats;

/* ---- lifecycle: replaces Init_GPU_elevationmap (GPU:940-994, called EMg.cpp:199) --------------- */
int  gem_create(const gem_map_config* cfg, gem_handle** out);
void gem_destroy(gem_handle* h);
const char* gem_last_error(const gem_handle* h);      /* h may be NULL: error of the last failed gem_create */
int  gem_abi_version(void);

/* stream the handle enqueues on (a hipStream_t passed as void*); NULL = the handle's own stream */
int  gem_set_stream(gem_handle* h, void* hip_stream);
int  gem_synchronize(gem_handle* h);
/* Stream-ordered device inputs: a caller whose cloud is produced on ANOTHER stream records a hipEvent_t there and hands it over
 * before the *_device call; all work the handle enqueues afterwards (on either of its internal streams) waits for it on the
 * device -- no host synchronisation.  Without it, device buffers must be complete when a *_device entry is called.          */
int  gem_wait_event(gem_handle* h, void* hip_event);

/* ---- Move (GPU:1004-1083, called EMg.cpp:1032) -------------------------------------------------- */
int  gem_move(gem_handle* h, const float position[3], float out_center[2], int out_start[2],
              float out_aligned_shift[2]);
int  gem_get_pose(gem_handle* h, float out_center[2], int out_start[2]);

/* ---- Process_points (GPU:1085-1144, called SPB.cpp:208): host SoA arrays in, host arrays out.
 *      x,y,z are overwritten with -1 for rejected points like the reference's device copies
 *      (GPU:443-446) only if write_back_xyz != 0.  Any output pointer may be NULL.              */
int  gem_process_points(gem_handle* h, const gem_frame_params* p, int n,
                        float* x, float* y, float* z, const int* orig_index, int write_back_xyz,
                        int* map_index, float* var, float* x_ts, float* y_ts, float* z_ts);

/* ---- Fuse (GPU:1154-1193, called EMg.cpp:280): host arrays in.  R,G,B,intensity may be NULL. -- */
int  gem_fuse(gem_handle* h, int n, const int* index, const int* R, const int* G, const int* B,
              const float* intensity, const float* height, const float* var);

/* ---- the fused path: SensorProcessorBase::process + Fuse (EMg.cpp:254-283) in one call on an
 *      interleaved XYZI cloud (16 B / point); rgb = packed 0x00RRGGBB per point or NULL.
 *      Nothing returns to the host.  This is the ElevationMap::add-shaped entry.                  */
int  gem_add(gem_handle* h, const gem_frame_params* p, int n, const float* xyzi,
             const uint32_t* rgb, const int* orig_index);
/*      gem_add_device takes device pointers and only enqueues.  The buffers must be complete when the call is made -- or
 *      their producer's event must have been passed to gem_wait_event -- and stay untouched until gem_synchronize (or
 *      any call that returns map data).  The order of operations the caller issues is the order the map sees;
 *      underneath, a stream of single colourless sweeps runs as ONE launch per frame (binning of the new cloud next
 *      to the fusion of the previous frame's records), the newest frame's fusion being launched by the next call
 *      that needs it; a cloud big enough for the sorted pipeline (a depth image) likewise leaves its last kernel, the walk
 *      over its sorted records, to the next call -- which can then launch it without a stream wait.  A gem_add_device call
 *      may enqueue NOTHING until the next call or the next observation of the map: where two sweeps share a launch (a stream
 *      nobody reads in between; gem_hip_debug.h, "frame_pair") every other call is held.  The rule above -- the caller's buffer
 *      stays untouched until gem_synchronize -- already covers it.                                                          */
int  gem_add_device(gem_handle* h, const gem_frame_params* p, int n, const void* d_xyzi,
                    const void* d_rgb, const void* d_orig_index);

/* ---- AoS ingest: the cloud as an array of point structs, e.g. pcl::PointCloud<PointXYZRGBICT>::points
 *      (PointXYZRGBICT.hpp:28-46: 32-byte structs, x y z at 0 4 8, rgb at 16 -- PCL's b g r a bytes --, intensity at 24).
 *      Replaces the host loop that pulls the fields into seven arrays (SPB.cpp:160-169) and the packing that gem_add
 *      expects: the structs are copied to the device as they are and unpacked there.  Offsets are byte offsets of 4-byte
 *      fields inside a struct of point_step bytes; off_intensity / off_rgb may be -1 (intensity 0 / no colours).
 *      Same result as gem_add on the unpacked arrays.                                                            */
int  gem_add_aos(gem_handle* h, const gem_frame_params* p, int n, const void* points_host, int point_step,
                 int off_x, int off_y, int off_z, int off_intensity, int off_rgb);

/* ---- cleanPointCloud (SPB.cpp:89, the first step of SensorProcessorBase::process) on the device: a raw cloud as the sensor
 *      driver publishes it -- an organised depth image with its NaN holes -- goes to the GPU with nothing done on the host.
 *        GEM_CLEAN_REMOVE_NAN      keep point i iff x, y and z are all finite, in input order: pcl::removeNaNFromPointCloud on a cloud
 *                                  with is_dense == false (Laser LaserSensorProcessor.cpp:50-59, Perfect PerfectSensorProcessor.cpp:41-49,
 *                                  Stereo StereoSensorProcessor.cpp:37-48, which also keeps each kept point's position in the organised
 *                                  cloud -- indices_ -- for getI / getJ, StereoSensorProcessor.cpp:108-116).  An is_dense cloud is kept
 *                                  whole by the reference: pass GEM_CLEAN_NONE for it.
 *        GEM_CLEAN_PASSTHROUGH_Z   ... and z_min <= z <= z_max, compared in FLOAT: pcl::PassThrough<PointT> on "z" with cutoff_min_depth /
 *                                  cutoff_max_depth (StructuredLightSensorProcessor.cpp:40-41, 51-66), whose limits PCL stores as float.
 *      Every compaction here is stable: kept points keep their order, orig[k] = input position of the k-th kept point.
 *      The fuse entries (gem_add_raw*, gem_add_aos_raw) compact nothing.  The pipelines already reject a point with a non-finite
 *      coordinate in projection: h = T[8] x + T[9] y + T[10] z + T[11] is then NaN or +-inf (0 * inf is NaN), and the height window
 *      h > lower && h < upper is false for NaN, for +inf (inf < upper fails even for upper = +inf) and for -inf (-inf > lower fails
 *      even for lower = -inf) -- in project_point and project_bin_laser_fast alike.  So REMOVE_NAN costs no pass at all, and
 *      PASSTHROUGH_Z one copy of the cloud in which every dropped point has x = y = z = NaN.  The orig index a stereo frame derives its
 *      pixel from stays the RAW position (no orig array = "first + i"), which is what the reference's indices_ hold: fusing a raw
 *      cloud gives the map of fusing the cleaned cloud, of the cleaned count, with its indices (the reference's intended behaviour;
 *      not its hazard of Fuse'ing point_num = the RAW count over arrays whose tail is uninitialised, EMg.cpp:259,280).
 *      gem_stats.points_in counts the RAW points of a gem_add_raw* call.                                                        */
enum { GEM_CLEAN_NONE = 0, GEM_CLEAN_REMOVE_NAN = 1, GEM_CLEAN_PASSTHROUGH_Z = 2 };
typedef struct gem_clean_params {
    int   mode;                    /* GEM_CLEAN_* */
    float z_min, z_max;            /* GEM_CLEAN_PASSTHROUGH_Z: inclusive float limits */
} gem_clean_params;
/*      What SensorProcessorBase::process runs for a sensor model: laser / stereo / perfect -> REMOVE_NAN; structured light ->
 *      PASSTHROUGH_Z with the cutoffs rounded to float (round to nearest).  The reference's defaults numeric_limits<double>::min() /
 *      ::max() become +0.0f (so z = -0.0 is kept) and +inf.  Pure host function: needs no device.                            */
int  gem_clean_params_for_model(int sensor_model, double cutoff_min_depth, double cutoff_max_depth, gem_clean_params* out);
/*      The compaction itself, device pointers, enqueued on the handle's stream (behind gem_wait_event's events; the host is never
 *      synchronised): n XYZI points (+ packed rgb, may be NULL) -> the kept points in order in d_xyzi_out / d_rgb_out, their input
 *      positions in d_orig_out (int), their number in *d_count_out (an int in DEVICE memory).  Outputs other than d_count_out may be
 *      NULL; each holds n elements.  Any n >= 0.                                                                                 */
int  gem_clean_device(gem_handle* h, const gem_clean_params* clean, int n, const void* d_xyzi, const void* d_rgb,
                      void* d_xyzi_out, void* d_rgb_out, void* d_orig_out, void* d_count_out);
/*      gem_add / gem_add_device / gem_add_aos on a RAW cloud (staging, arenas and gem_reserve rules as theirs; no orig array: the raw
 *      position is every point's orig index).  Same map as the plain entry on the cleaned cloud with the kept indices.          */
int  gem_add_raw(gem_handle* h, const gem_frame_params* p, const gem_clean_params* clean, int n, const float* xyzi, const uint32_t* rgb);
int  gem_add_raw_device(gem_handle* h, const gem_frame_params* p, const gem_clean_params* clean, int n, const void* d_xyzi, const void* d_rgb);
int  gem_add_aos_raw(gem_handle* h, const gem_frame_params* p, const gem_clean_params* clean, int n, const void* points_host, int point_step,
                     int off_x, int off_y, int off_z, int off_intensity, int off_rgb);
/*      SensorProcessorBase::process on a raw cloud (SPB.cpp:66-94): clean, then Process_points on the kept points.  The per-point
 *      outputs (each may be NULL; each holds n elements) cover the *n_kept kept points in order; orig_out = their raw positions.
 *      Host arrays: the kept count is read back.                                                                                 */
int  gem_process_points_raw(gem_handle* h, const gem_frame_params* p, const gem_clean_params* clean, int n,
                            const float* x, const float* y, const float* z, int* n_kept, int* orig_out,
                            int* map_index, float* var, float* x_ts, float* y_ts, float* height);

/* ---- the VoxelGrid pre-filter of the launch files (filter.launch: one stage; filter_kitti.launch: three) on the device: one
 *      pcl::VoxelGrid<pcl::PCLPointCloud2> stage as pcl_ros's nodelet runs it (PCL 1.7 / 1.8, downsample_all_data, no minimum
 *      points per voxel), up to four stages per call.  One stage on n XYZI points, inv[k] = 1.0f / leaf[k] in float:
 *        1. bounds (getMinMax3D): over the points with finite x, y, z whose field value passes the limit test against the limits
 *           CAST TO FLOAT -- normal: skip if v > max || v < min; negative: skip if v < max && v > min (a NaN value is kept) --
 *           the float min_p / max_p per coordinate.  No such point: the output is empty.
 *        2. point test: the same test against the DOUBLE limits (v promoted), and x, y, z finite.  (At a limit float cannot hold,
 *           say 0.1, a point may shape the bounds and not be output.)  GEM_VOXEL_FIELD_NONE: finite x, y, z only.
 *        3. overflow: d_k = (int64)((max_p[k] - min_p[k]) * inv[k]) + 1 in float; d0 * d1 * d2 > INT32_MAX: the stage's output
 *           is its input unchanged, all n points in order (PCL's output = *input_).
 *        4. voxel: min_b = (int)floorf(min_p * inv), div = (int)floorf(max_p * inv) - min_b + 1, mul = (1, div0, div0 * div1);
 *           ijk_k = (int)floorf(p_k * inv_k) - min_b_k, idx = ijk . mul in wrapping int32, taken as uint32.  (int) of a float
 *           outside the int range is INT_MIN, as x86 converts it.
 *        5. order: ascending idx; inside a voxel, input order.  (PCL's std::sort is not stable: PCL itself may sum a voxel of
 *           three or more points in another order, last-bit differences there.)
 *        6. centroid: x, y, z, intensity summed sequentially in float from +0.0f, divided by (float)count; with rgb, r, g, b
 *           summed as floats, divided, truncated to int, repacked (r << 16) | (g << 8) | b.
 *      The output holds n points: the m centroids, then x = y = z = NaN, intensity 0 (rgb 0), which the pipelines reject in
 *      projection (above) and gem_colorize_device gives pixel -1.  Stage s + 1 reads stage s's m points.                     */
enum { GEM_VOXEL_FIELD_NONE = 0, GEM_VOXEL_FIELD_X = 1, GEM_VOXEL_FIELD_Y = 2, GEM_VOXEL_FIELD_Z = 3, GEM_VOXEL_FIELD_INTENSITY = 4 };
typedef struct gem_voxel_params {
    float  leaf[3];                /* leaf size (the nodelet's double leaf_size cast to float); finite, > 0 */
    int    field;                  /* GEM_VOXEL_FIELD_* */
    double limit_min, limit_max;   /* filter limits (PCL's defaults: -FLT_MAX, FLT_MAX) */
    int    limit_negative;         /* keep the points OUTSIDE the limits */
    int    reserved;               /* 0 */
} gem_voxel_params;
/*      n_stages (1..4) stages on n XYZI points (+ packed rgb, may be NULL), device pointers, enqueued on the handle's stream (the
 *      host is never synchronised): the result in d_xyzi_out / d_rgb_out (n elements each; d_rgb_out may be NULL; neither may
 *      overlap an input), m in *d_count_out (an int in DEVICE memory).  Any n >= 0.  GEM_ERR_INVALID for a leaf that is not
 *      finite or not > 0, n_stages outside 1..4, a field outside the enum, and on a handle that joined a communicator.        */
int  gem_voxel_device(gem_handle* h, const gem_voxel_params* stages, int n_stages, int n, const void* d_xyzi, const void* d_rgb,
                      void* d_xyzi_out, void* d_rgb_out, void* d_count_out);
/*      gem_add (host XYZI, staged as gem_add stages it) / gem_add_device behind the filter: the same map as gem_add on the m
 *      centroids with orig index = output position.  The filtered cloud lives in the handle's arenas (gem_reserve sizes them);
 *      the rules of those entries hold otherwise.                                                                               */
int  gem_add_voxel(gem_handle* h, const gem_frame_params* p, const gem_voxel_params* stages, int n_stages, int n, const float* xyzi,
                   const uint32_t* rgb);
int  gem_add_voxel_device(gem_handle* h, const gem_frame_params* p, const gem_voxel_params* stages, int n_stages, int n,
                          const void* d_xyzi, const void* d_rgb);

/* ---- depth images: the pinhole unprojection in front of the fused path.  A depth camera produces a depth image; the organised XYZ
 *      cloud the node receives was made from it on the host (depth_image_proc, or the driver's point-cloud filter) at 16 B a pixel
 *      (+ 4 B packed colour), where the image is 2 B (uint16 millimetres; + 3 B BGR8).  These entries take the image itself.
 *      The semantics RESTATE depth_image_proc::convert<T> (ROS noetic, depth_conversions.h, range_max = 0) and are NOT verified against
 *      an installation (there is none here); tests/depth_ref.py is the same statement in numpy.
 *        host constants (double, then one rounding each; gem_depth_constants):
 *          unit = (double)depth_unit for GEM_DEPTH_U16, a depth_unit of 0 replaced by 0.001f first (DepthTraits<uint16_t>); 1.0 for F32
 *          kx = (float)(unit / fx), ky = (float)(unit / fy), cxf = (float)cx, cyf = (float)cy
 *        per pixel (u, v), point i = v * width + u, all arithmetic in float, every operation rounded:
 *          U16  d = the count; invalid iff d == 0; df = (float)d; z = df * depth_unit (0 -> 0.001f)
 *          F32  d = the value; invalid iff !isfinite(d) -- negative depths, zeros and denormals are valid, as in the original;
 *               df = d; z = d
 *          valid    x = (((float)u - cxf) * df) * kx,  y = (((float)v - cyf) * df) * ky
 *          invalid  x = y = z = NaN (the quiet NaN 0x7fc00000)
 *          I = intensity for every pixel; rgb = 0x00RRGGBB from the pixel of the colour image (taken as registered to the depth
 *          image: same width x height), for every pixel, valid or not.  GEM_COLOR_NONE: no rgb array.
 *      NOT covered: range_max substitution for invalid pixels, depth-to-colour registration, lens distortion (the input is rectified,
 *      as depth_image_proc assumes), disparity images.                                                                             */
enum { GEM_DEPTH_U16 = 0, GEM_DEPTH_F32 = 1 };
enum { GEM_COLOR_NONE = 0, GEM_COLOR_BGR8 = 1, GEM_COLOR_RGB8 = 2 };
typedef struct gem_depth_image {
    int    width, height;         /* pixels; width * height <= 2^26 */
    int    format;                /* GEM_DEPTH_* */
    size_t row_stride;            /* bytes; 0 = tight; a multiple of the element size, >= width * element size */
    double fx, fy, cx, cy;        /* CameraInfo K, as image_geometry returns them */
    float  depth_unit;            /* U16: metres per count; 0 -> 0.001f (DepthTraits<uint16_t>).  F32: ignored */
    float  intensity;             /* written to the I channel of every pixel */
    int    color_format;          /* GEM_COLOR_*: a registered colour image of the same width x height */
    size_t color_row_stride;      /* bytes; 0 = tight (width * 3) */
} gem_depth_image;
/*      GEM_ERR_INVALID from every entry below, nothing changed: a NULL image, NULL depth with pixels present, color_format != NONE
 *      with NULL colour (pixels present), a negative size, more than 2^26 pixels, an unknown format, a bad stride, fx or fy zero or not
 *      finite, cx or cy not finite, a non-finite or negative depth_unit, a bad clean mode.  An image with width == 0 or height == 0
 *      is not an error: it holds no pixels and adds nothing (as n == 0 of gem_add).
 *      The four constants kx, ky, cxf, cyf.  Pure host function: needs no device.                                               */
int  gem_depth_constants(const gem_depth_image* img, float out[4]);
/*      The organised cloud: width * height XYZI points in row-major pixel order into d_xyzi_out (16-byte aligned; + packed rgb into
 *      d_rgb_out unless GEM_COLOR_NONE or d_rgb_out is NULL), device pointers, enqueued on the handle's stream (the host is never
 *      synchronised).  It takes nothing from the map.  With clean->mode == GEM_CLEAN_PASSTHROUGH_Z every point the filter drops has
 *      x = y = z = NaN: the cleanPointCloud mask of the fuse entries applied to the plain output, bit for bit, in the same kernel.
 *      NONE, REMOVE_NAN and a NULL clean change nothing.                                                                         */
int  gem_depth_unproject_device(gem_handle* h, const gem_depth_image* img, const void* d_depth, const void* d_color,
                                const gem_clean_params* clean /* may be NULL */, void* d_xyzi_out, void* d_rgb_out /* may be NULL */);
/*      gem_add_raw_device on that cloud (clean; may be NULL) or gem_add_voxel_device on it (stages, n_stages > 0) -- the same map --
 *      from an image in host memory (read when the call returns, as for gem_add_aos) or in device memory (complete at the call,
 *      untouched until gem_synchronize, as for gem_add_device).  There is no orig array: the raw position is the pixel index, so a
 *      stereo frame's getI / getJ need p->original_width == img->width (GEM_ERR_INVALID otherwise).  clean and stages both non-NULL:
 *      GEM_ERR_INVALID (the front ends are exclusive).  The image is unprojected into the handle's staging arena, the PASSTHROUGH_Z
 *      mask in the same kernel; gem_reserve(width * height, 1, with_colours) covers images with tight rows.  gem_stats.points_in
 *      counts width * height.                                                                                                    */
int  gem_add_depth(gem_handle* h, const gem_frame_params* p, const gem_depth_image* img, const void* depth, const void* color,
                   const gem_clean_params* clean, const gem_voxel_params* stages, int n_stages);
int  gem_add_depth_device(gem_handle* h, const gem_frame_params* p, const gem_depth_image* img, const void* d_depth, const void* d_color,
                          const gem_clean_params* clean, const gem_voxel_params* stages, int n_stages);

/* ---- batched sweeps (BASELINE config 4): for s in 0..n_sweeps-1:
 *        Mapvar_update(var_updates[s]) ; add(params[s], cloud s)
 *      with the map pose fixed for the batch.  Clouds are device-resident, concatenated:
 *      cloud s = d_xyzi + 16*offsets[s], offsets has n_sweeps+1 entries.                           */
int  gem_add_batch_device(gem_handle* h, int n_sweeps, const gem_frame_params* params,
                          const void* d_xyzi, const long long* offsets, const float* var_updates);

/* ... the same from HOST memory (the reference's caller owns host arrays, EMg.cpp:260-283, GPU:1096-1141):
 *      sweep s = clouds_host[s][0 .. 4 * counts[s]) floats (XYZI points).  The sweeps are copied into the handle's own
 *      device arena one behind the other -- the staging copy of a sweep beside the DMA of the one before -- and fused by
 *      one batched pass; the caller's arrays have been read when the call returns.                                */
int  gem_add_batch(gem_handle* h, int n_sweeps, const gem_frame_params* params, const float* const* clouds_host,
                   const int* counts, const float* var_updates);

/* ---- Mapvar_update (GPU:1146-1152, called RMU.cpp:81) ------------------------------------------ */
int  gem_mapvar_update(gem_handle* h, float var_update);

/* ---- layer access (what the dead G_get_mapinfo / G_set_mapinfo hinted at, GPU:457-475; feeds
 *      ElevationMap::show, EM.cpp:85-149).  dst/src hold L*L 4-byte elements (float, or int32 for
 *      the colour layers in STORAGE_ROWMAJOR; float in GRIDMAP layout).                            */
int  gem_get_layer(gem_handle* h, int layer, int layout, void* dst_host);
int  gem_set_layer(gem_handle* h, int layer, const void* src_host);     /* STORAGE_ROWMAJOR only */
int  gem_layer_device_ptr(gem_handle* h, int layer, void** out_device_ptr);

/* ---- traversability stage that follows the fusion every frame: Map_feature (GPU:1256-1302, kernel
 *      G_Mapfeature GPU:549-670 with the Jacobi eigen-solver GPU:66-187; called EMg.cpp:410).  Computes the
 *      ROUGH, SLOPE and TRAVER layers on the device from ELEVATION.  Each host pointer may be NULL (nothing is
 *      copied for it); with all NULL the call only enqueues the kernel.  Like the reference, the nine arrays
 *      hold L*L elements in STORAGE_ROWMAJOR order.  Cells without elevation report rough = slope = 0 and
 *      keep their stored traversability (the reference leaves its output arrays uninitialised there).       */
int  gem_map_feature(gem_handle* h, float* elevation, float* variance, int* colorR, int* colorG, int* colorB,
                     float* rough, float* slope, float* traver, float* intensity);

/* ---- the feed of ElevationMap::show (EM.cpp:85-149, called EMg.cpp:413 right after Map_feature): the reference copies
 *      nine L*L arrays to the host and loops over all cells there.  gem_show does that loop on the resident layers:
 *        visual      9 x L*L floats, grid_map::Matrix layout (Eigen column-major by BUFFER index) of visualMap_'s layers in the order
 *                    elevation, variance, rough, slope, traver, color_r, color_g, color_b, intensity (EM.cpp:44); NaN where the cell
 *                    has no elevation or no traversability (EM.cpp:89, 101)
 *        points_*    the coloured cloud of EM.cpp:113-122, one point per kept cell in grid_map's iteration order, compacted on the
 *                    device: xyz n x 3 floats (x, y from grid_map's getPositionFromIndex in double, z = elevation), rgb n x 3 bytes;
 *                    both arrays must hold L*L points; *out_count = n
 *        image_bgr   the L x L x 3 orthomosaic of EM.cpp:87, 124-126 (unwrapped row, column; b, g, r)
 *      map_length / resolution / position are visualMap_'s geometry (doubles, EMg.cpp:178; position = what Move returned,
 *      EM.cpp:172-177); pass 0 / 0 / NULL to use length * resolution, the handle's resolution and centre.  Any output may be NULL.
 *      Run gem_map_feature first: rough / slope / traver are its layers.                                                      */
int  gem_show(gem_handle* h, double map_length, double resolution, const double position[2],
              float* visual, float* points_xyz, unsigned char* points_rgb, int* out_count, unsigned char* image_bgr);

/* ---- input colourisation (EMg.cpp:349-381, the loop of ElevationMapping::Callback in front of the path): every
 *      point is projected into the camera image with P_lidar2img = T.camera (3x4) * T.lidar (4x4) (doubles, EMg.cpp:342-345;
 *      row-major here), takes the BGR pixel it lands on, and draws cv::circle(img, pixel, 1, that colour) into the image the
 *      later points sample -- gem_colorize reproduces that order dependence (the latest earlier point on a 4-neighbour pixel
 *      hands its colour on).  Points that fall outside the image (or behind the camera) get colour 0 and INTENSITY 0
 *      (EMg.cpp:372-377): xyzi is updated in place.  rgb[i] = 0x00RRGGBB, the `rgb` input of gem_add*.  row_stride = bytes per
 *      image row (0 = width * 3).  The image itself is left as it was (the reference's drawn-on copy is discarded, EMg.cpp:316). */
typedef struct gem_camera {
    double lidar_to_image[12];   /* row-major 3 x 4 */
    int    width, height;
} gem_camera;
int  gem_colorize(gem_handle* h, const gem_camera* cam, int n, float* xyzi, const unsigned char* image_bgr, size_t row_stride, uint32_t* rgb);
int  gem_colorize_device(gem_handle* h, const gem_camera* cam, int n, float* d_xyzi, const unsigned char* d_image_bgr, size_t row_stride,
                         uint32_t* d_rgb);           /* device pointers; only enqueues on the handle's stream */

/* ---- loop-closure re-anchoring: Map_optmove (GPU:1215-1233, called EMg.cpp:1020) relabels the
 *      map centre to opt_position snapped to the old centre's cell lattice (the circular buffer is not shifted,
 *      nothing is cleared) and adds height_update to every valid elevation (G_update_mapheight, GPU:1195-1202);
 *      Map_closeloop (GPU:1235-1254) moves the centre by the aligned shift instead.                         */
int  gem_map_optmove(gem_handle* h, const float opt_position[2], float height_update, float out_aligned_position[2]);
int  gem_map_closeloop(gem_handle* h, const float update_position[2], float height_update);

/* ---- visibility clean-up: Raytracing (GPU:1304-1318, called EMg.cpp:421) = G_Raytracing (GPU:708-891):
 *      every cell with traversability below obstacle_threshold walks away from the map centre along the centre->cell
 *      ray; crossed cells with a lowest scan point this frame bound its height by the sensor's line of sight, and the
 *      cell is deleted (elevation = -10) if elevation - 3 sigma exceeds the tightest bound -- then G_Clear_maplowest
 *      (GPU:232-239) resets the LOWEST layer to 10.
 *      The LOWEST layer is the side output of G_pointsprocess (GPU:430-439: lowest = min(lowest, h); if (h == lowest)
 *      lowest += 3 * var, per GEOGRAPHIC cell).  It is maintained -- in input order per cell, the result of running the
 *      reference's grid sequentially -- by the fuse kernels of gem_fuse / gem_add* ONLY while lowest tracking is on
 *      (default off: the LiDAR hot path is not slowed down); gem_process_points alone does not touch it.              */
int  gem_set_lowest_tracking(gem_handle* h, int enabled);
int  gem_raytracing(gem_handle* h);

/* ---- statistics / timing (bench harness) --------------------------------------------------------- */
int  gem_set_timing(gem_handle* h, int enabled);      /* record hipEvents around each pipeline kernel */
int  gem_set_counting(gem_handle* h, int enabled);    /* count binned points / touched cells on device */
int  gem_get_stats(gem_handle* h, gem_stats* out, int reset);

/* Pre-size the handle's device arenas for the largest pass that is going to come: max_points points in at most max_sweeps sweeps
 * per call (1 for gem_add / gem_add_device / gem_fuse), with or without colours.  The arenas only ever grow, but growing in the
 * middle of a stream -- the first bigger cloud after smaller ones -- waits for everything in flight and re-allocates; after
 * gem_reserve no pass within these bounds allocates, whichever pipeline it takes (the sorted forms from their thresholds on, the
 * tile pipeline below them -- a single cloud of more than 131 072 points is fused there as several sweeps, which max_sweeps = 1
 * covers; the sweeps of a batch below the sorted threshold are taken to be at most twice their mean length).
 * On a handle that joined a communicator with gem_comm_init_tiles the bounds are those of a gem_add_sharded_device STEP -- the
 * GLOBAL points and sweeps: the shard's sort (its W-th of the points), both sets of receive buffers (no strip gets more records
 * than the step has points) and the staging tables are sized.  Synchronous; call it once after gem_create / gem_comm_init*.    */
int  gem_reserve(gem_handle* h, long long max_points, int max_sweeps, int with_colours);

/* ---- multi-GPU: RCCL all-gather of the fused strips over xGMI ------------------------
 *      One process per GPU, one handle per process.  gem_comm_init splits the map into row strips in STORAGE coordinates
 *      (rank r owns rows [L r / W, L (r+1) / W): Move never migrates data); gem_comm_init_tiles makes the strips whole rows of
 *      32 x 32-cell tiles, which the sharded path below needs.  gem_allgather_layers completes every rank's copy of the layers:
 *      every rank's strip goes DIRECTLY to every other rank (one grouped ncclSend / ncclRecv pair per peer and layer: each peer
 *      has its own xGMI link; strips of any sizes), read from a published copy of the strip and carried by the handle's
 *      communication stream -- the call returns at once, later passes over this rank's own strip run beside the transfers, and
 *      whatever observes the whole map (gem_get_layer, gem_synchronize, gem_move, ...) waits for them.
 *      Stage A (replicated binning): every rank calls gem_add* with the WHOLE cloud and fuses only its strip.             */
int  gem_comm_unique_id(void* out_128_bytes);
int  gem_comm_init(gem_handle* h, const void* unique_id_128_bytes, int nranks, int rank);
int  gem_comm_init_tiles(gem_handle* h, const void* unique_id_128_bytes, int nranks, int rank);
int  gem_get_strip(gem_handle* h, int* out_row0, int* out_row1);
int  gem_allgather_layers(gem_handle* h, int with_attributes);   /* elevation+variance (+intensity, colours) */

/*      Stage B (points sharded): rank r holds a contiguous index range of the batch -- sweeps first_global_sweep ..
 *      first_global_sweep + n_local_sweeps - 1 of n_global_sweeps (a sweep may be split between two neighbouring ranks: both
 *      pass it, the lower rank holds its head; first_point_in_sweep = index, inside its sweep, of this rank's first point --
 *      the camera sensor models derive the pixel row / column from it).  gem_add_sharded_device = for s:
 *      Mapvar_update(var_updates_global[s]); add(sweep s) on the map tiled over the ranks: each rank projects / bins / sorts its
 *      own points for the whole map (block-sorted: the records of a strip, and of every block of 256 cells, are one contiguous
 *      range), the sorted records of every strip travel to the strip's owner together with their block ranges (ncclSend /
 *      ncclRecv, one group, on the handle's communication stream; a rank's own records stay where they are), and the owner takes
 *      every block's records source by source in rank order -- ascending index ranges, so rank order is input order and every
 *      cell sees its points exactly as on one device.  With one rank nothing is exchanged and nothing returns to the host.  With
 *      more, the call enqueues the step's sort and the all-gather of its strip boundaries (16 words per rank, copied to the host)
 *      and returns; the step's SECOND HALF -- the exchange on the communication stream, the fusion on the handle's stream, and the
 *      all-gather of the layers on a stream and communicator of their own if gem_allgather_layers followed the step -- is enqueued by
 *      the NEXT call, or by whatever observes or modifies the map (gem_synchronize, gem_get_layer, gem_move, gem_mapvar_update,
 *      ...): nothing ever waits for work the same call enqueued, and consecutive steps overlap stage by stage.  All of these are
 *      collectives: every rank makes the same sequence of calls.  var_updates_global (n_global_sweeps <= 512 values, identical on
 *      all ranks) may be NULL.  No colours, no lowest tracking on this path.  Arguments, geometry and every allocation -- the receive
 *      buffers included, sized from gem_reserve's bound or from W shares like this rank's -- are checked before the step's first
 *      collective; a rank that still cannot go on in the middle of a step (a step that brings more records than foreseen, and no
 *      memory to grow) aborts both communicators, so that its peers fail instead of waiting.
 *      The two halves are exported for hosts that carry the exchange themselves (gem_amd/tiling.py with torch.distributed):
 *      gem_shard_sort_device returns the device arrays of the sorted records {h, var} (8 bytes) / keys (4 bytes),
 *      out_bounds[nstrips + 1] = the first record of every strip, and (optional) the device array of the block ranges
 *      {first, end} (8 bytes per block of 256 cells, 4 x tiles entries, positions in the sorted arrays; empty block = {0, 0});
 *      gem_shard_fuse_device walks this handle's strip through n_src sources in input order: device pointers and record counts,
 *      and optionally (d_ranges, bases -- both or neither) every source's block ranges with entry 0 = the first block of this
 *      handle's strip, and the position in the source's own arrays that d_hv[s] / d_key[s] point at; without them the blocks'
 *      records are found by search.                                                                                        */
int  gem_add_sharded_device(gem_handle* h, int n_local_sweeps, const gem_frame_params* params, const void* d_xyzi,
                            const long long* offsets, int first_global_sweep, int n_global_sweeps, int first_point_in_sweep,
                            const float* var_updates_global);
int  gem_shard_sort_device(gem_handle* h, int n_local_sweeps, const gem_frame_params* params, const void* d_xyzi,
                           const long long* offsets, int first_global_sweep, int n_global_sweeps, int first_point_in_sweep,
                           int nstrips, const int* strip_rows,
                           uint32_t* out_bounds, const void** out_d_hv, const void** out_d_key, const void** out_d_ranges);
int  gem_shard_fuse_device(gem_handle* h, int n_src, const void* const* d_hv, const void* const* d_key, const uint32_t* counts,
                           const void* const* d_ranges, const uint32_t* bases, int n_global_sweeps, const float* var_updates_global);


/* ---- the rolling-window local map (ElevationMapping::updateLocalMap, EMg.cpp:609-767; visualPointMap, :520-530) -----------------
 *   gem_local_enable           capacity > 0: switch the local map on, empty, with room for `capacity` entries (it grows on demand);
 *                              on an enabled handle it starts over (empty map, no capture).  0: switch it off and free its memory.
 *   gem_local_capture          what map_.show() leaves in visualMap_ (EM.cpp:89-111): the cells with elevation != -10, traver != -10
 *                              and traver not NaN, in grid_map's iteration order, with the geometry (gem_show's rules: map_length <= 0
 *                              -> L * resolution, resolution <= 0 -> the map's, position NULL -> the map's centre) and the start
 *                              index at the time of the call.  Take it between gem_map_feature and gem_raytracing: prevMap_ is a copy
 *                              of the show output, so cells raytracing deletes afterwards are still in it (EMg.cpp:413-422).
 *   gem_local_keep_previous    prevMap_ = map_.visualMap_ (EMg.cpp:422, :621, :1025): the last capture becomes the previous one.
 *   gem_local_grid_cloud       gridMaptoPointCloud (EMg.cpp:1198-1224) of the last capture: every kept cell, in iteration order.
 *   gem_local_spill            the body of the "Local mapping" block (EMg.cpp:715-764) without its gate: every cell of the PREVIOUS
 *                              capture with traver >= 0.0 (double; NaN fails) whose position -- grid_map's getPositionFromIndex in
 *                              double from that capture's geometry -- passes the eight-way predicate of :726-733 against
 *                              current_position (float, promoted) -/+ length * resolution / 2 (double; the previous capture's
 *                              resolution) with float compares of position_shift's signs.  In iteration order, each is written to
 *                              points and upserted under ((float) x, (float) y): a present key is removed and inserted again, so it
 *                              moves to the end of the order.  out_replaced = the reference's `count`: selected cells whose key was
 *                              present, an earlier cell of the same call included (far from the origin distinct cells can round to
 *                              one key: the later one wins).  Keys compare as float pairs, so -0 equals +0.  The caller keeps the
 *                              gate, verbatim:  if (std::abs(dx) >= res || (std::abs(dy) >= res && initFlag == 0 && JumpFlag == 0)).
 *   gem_local_export           localHashtoPointCloud (EMg.cpp:1124-1140), in last-write order (a dict with del d[k]; d[k] = v); with
 *                              clear != 0 the local map is emptied afterwards (localMap_.swap(tmp)).  points may be NULL: only the
 *                              count is returned.
 *   gem_local_size             entries of the local map.
 * Records are PointXYZRGBICT (32 bytes): x, y the float positions, z elevation, pad = 1.0f, b g r from the colour layers through int,
 * a = 0, covariance = variance, intensity, travers = traver.  The reference leaves pad and a uninitialised and its
 * localHashtoPointCloud never sets intensity: the device writes the stored intensity there.  points arrays: L * L records (spill,
 * grid_cloud) or max_points (export); they may be NULL.  GEM_ERR_INVALID: not enabled, spill / keep_previous before any capture,
 * spill before any keep_previous, a handle with a communicator, max_points below the entry count.  Positions are assumed finite. */
int  gem_local_enable(gem_handle* h, long long capacity);
int  gem_local_capture(gem_handle* h, double map_length, double resolution, const double position[2]);
int  gem_local_keep_previous(gem_handle* h);
int  gem_local_grid_cloud(gem_handle* h, void* points, int* out_count);
int  gem_local_spill(gem_handle* h, const float current_position[2], const float position_shift[2],
                     void* points, int* out_count, int* out_replaced);
int  gem_local_export(gem_handle* h, void* points, long long max_points, long long* out_count, int clear);
int  gem_local_size(gem_handle* h, long long* out_count);

/* ---- composingGlobalMap without the host filter (EMg.cpp:482-514; pointCloudtoOctomap, :1146-1170) ------------------------------
 *   gem_local_compose            what pointCloudtoOctomap does to gridMaptoPointCloud(prevMap_) before the octree insertion, on the
 *                                PREVIOUS capture (gem_local_keep_previous): pcl::StatisticalOutlierRemoval<Anypoint> with
 *                                setMeanK(mean_k), setStddevMulThresh(stddev_mul), then the split of the survivors by travers.
 *   gem_local_compose_distances  the filter's per-point mean neighbour distances of the same cloud, in grid-cloud order.
 * PCL is not part of this library; the filter is RESTATED here from PCL >= 1.10 filters/impl/statistical_outlier_removal.hpp and
 * FLANN's L2_Simple<float> (tests/compose_ref.py is the same statement in numpy):
 *   input      the n records of the previous capture in its order (= gem_local_grid_cloud of that capture); the coordinates are the
 *              records' float x, y, z.  Elevation is assumed finite.
 *   d2         for point i and every point j, i included: d2 = ((dx*dx) + (dy*dy)) + (dz*dz), every operation rounded in float, no FMA.
 *   distance   point i's d2 values sorted ascending, the first mean_k + 1 taken (entry 0 is the query or a coincident point: 0 either
 *              way).  double dist_sum = 0; for k = 1 .. mean_k in that order dist_sum += s(d2[k]); distance[i] = (float)(dist_sum /
 *              mean_k).  Equal values give the same sum whichever point supplied them, so no tie rule is needed and the result does
 *              not depend on a search structure's traversal order.
 *   s()        flags = 0: (double)sqrtf(d2), the float overload;  GEM_COMPOSE_SQRT_DOUBLE: sqrt((double)d2).  Both correctly rounded.
 *   threshold  double sum = 0, sq_sum = 0; for i = 0 .. n-1 IN ORDER: sum += distance[i]; sq_sum += distance[i] * distance[i], the
 *              product a FLOAT product, widened when it is added.  mean = sum / n; variance = (sq_sum - sum * sum / n) / (n - 1);
 *              threshold = mean + stddev_mul * sqrt(variance), all in double.
 *   filter     point i survives iff (double)distance[i] <= threshold; survivors keep their order.
 *   split      a survivor with (double)travers > travers_threshold goes to road; otherwise one with (double)travers <=
 *              travers_threshold (so: travers not NaN) goes to obstacle.  Both lists in survivor order, the records copied unchanged.
 *              A capture holds no NaN travers, so road + obstacle + removed = n.
 *   n <= mean_k  the reference reads past the end of its search result (undefined).  Here nothing is removed, every distance and the
 *              threshold are +inf; n = 0 gives three zero counts.  A deliberate difference, like pad / a in the records.
 * NOT verified against PCL (there is none here; tools/ros_selfcheck.cpp's `sor` row settles them in a ROS workspace): (1) which
 * overload PCL's unqualified sqrt(nn_dists[k]) resolves to -- hence the flag; (2) that the product in sq_sum is a float product;
 * (3) a NaN threshold (a variance rounded below zero: every distance equal) removes every point under the `<=` statement above.
 * road, obstacle: L * L records each, host memory, either may be NULL (counted only).  out_counts[3]: road points, obstacle points,
 * points the filter removed.  out_threshold may be NULL.  distances: L * L floats, may be NULL.  The octree insertion itself
 * (updateNode / integrateNodeColor) and the flags preMapAvail and globalMap_.size() >= 1 stay with the caller.  The calls take the
 * handle's lock like every other entry: the composing thread may call them while the callback thread runs the frame loop.
 * GEM_ERR_INVALID, nothing changed: the local map is not enabled, no gem_local_keep_previous yet, a handle with a communicator, p
 * NULL, mean_k outside 1 .. 32, stddev_mul not finite. */
#define GEM_COMPOSE_SQRT_DOUBLE 1
typedef struct gem_compose_params {
    int    mean_k;            /* setMeanK; the node uses 20.  1 <= mean_k <= 32 */
    double stddev_mul;        /* setStddevMulThresh; the node uses 1.0 */
    double travers_threshold; /* traversThre (a double parameter of the node, default 0.0) */
    int    flags;             /* GEM_COMPOSE_SQRT_DOUBLE or 0 */
} gem_compose_params;
int  gem_local_compose(gem_handle* h, const gem_compose_params* p, void* road, void* obstacle, int out_counts[3], double* out_threshold);
int  gem_local_compose_distances(gem_handle* h, const gem_compose_params* p, float* distances, int* out_count);

/* ---- the submap stack (globalMap_: the new-keyframe branch of updateLocalMap, EMg.cpp:630-687; updateGlobalMap, :773-905) -------
 *   gem_global_enable          capacity > 0: switch the stack on, empty, with room for `capacity` records (it grows on demand); on an
 *                              enabled handle it starts over.  0: switch it off and free its memory.
 *   gem_global_push_local      globalMap_.push_back(*out_pc + *grid_pc) on the device: the local map's export (gem_local_export's
 *                              records, last-write order) followed by the last capture's grid cloud (gem_local_grid_cloud), as one new
 *                              submap; with clear_local != 0 the local map is emptied afterwards (localMap_.swap(tmp)).
 *   gem_global_push            a caller's PointXYZRGBICT cloud (host memory) as one new submap (the denseSubmap branch: the node's
 *                              own pointcloudinterpolation output).
 *   gem_global_loop_closure    the body of updateGlobalMap after the flag, restated:
 *     1. n = min(n_opt, submaps) (optKeyframeNum clamped, :784-786); submaps >= n are untouched.
 *     2. transforms: n_opt 4x4 float matrices, each column-major as Eigen::Matrix4f::data() -- the node's
 *        (optGlobalMapLoc_[i] * trajectory_[i].inverse()).matrix().  Entry 0 is ignored.
 *     3. for i in [1, n) every record of submap i, a non-finite one included, becomes x' = x*m00 + (y*m01 + (z*m02 + m03)), y', z' and
 *        pad likewise from rows 1, 2, 3, each product and sum rounded in float (no FMA); the other fields are copied.  This restates
 *        the SSE2 form of pcl::detail::Transformer<float>::se3 (PCL >= 1.10, x86-64).
 *     4. the neighbours of submap i, i in [0, n): the j in [0, n) whose centre (centres: n_opt float pairs, localMapLoc_, not moved by
 *        the transforms) has d2 = dx*dx + dy*dy (float; neighbour minus i) < (float)(radius * radius) (the square in double), in
 *        ascending d2, ties by ascending j.  This restates KdTreeFLANN::radiusSearch with sorted results and FLANN's strict test.
 *     5. a list of more than two entries (:844) runs the pair steps (i, k = list[p]) for p = 1, 2, ... in order; position 0 is skipped
 *        even when it is not i (a coincident centre of lower index comes first, and then k == i).  A step hashes old = submap i and
 *        new = submap k, both as they are before the step: each record gets the key ((float)(ceil((double)x / res) * res - res / 2.0),
 *        the same for y), res = resolution (a double; <= 0: the map's resolution), and the first record of a key keeps it (keys compare
 *        as float pairs; every record with a NaN key is kept and never matched).  For every key of new also in old whose old variance
 *        ov satisfies 0 < ov < 1 (float compares), in double with nv, ne new's variance and elevation and oe old's elevation:
 *          nv2 = nv*nv, ov2 = ov*ov, elevation = (float)(((nv2*oe) + ((ov2*ne) / ov2)) + nv2), variance = (float)(((ov2*nv2) / ov2) + nv2)
 *        -- :862-863 as C++ precedence parses them -- with new's r, g, b, intensity and travers, into both maps; *out_fused counts these
 *        keys over all steps.  Then submap k := export(new) and after it submap i := export(old), so for k == i old wins.  An export
 *        writes per key x, y = the key, z = elevation, pad = 1, b g r, a = 0, covariance, intensity (the reference leaves it unset:
 *        the stored one is written), travers, in the order of the key's first record in the cloud the map was built from (the
 *        reference's order is std::unordered_map's; after one hash the keys are unique, so no value depends on it).
 *   gem_global_export          submap `index` (-1: all, in stack order) into points (host); points NULL: only *out_count.
 *   gem_global_count           the number of submaps.
 * Records are PointXYZRGBICT (32 bytes) as in gem_local_*.  The pose bookkeeping (trajectory_, localMapLoc_, the flags) stays with the
 * caller.  GEM_ERR_INVALID, the stack left as it was: not enabled, a handle with a communicator, push_local without an enabled local
 * map or a capture, n_opt < 0, transforms or centres NULL with n_opt > 1, radius not finite or negative, an index out of range,
 * max_points below the record count. */
int  gem_global_enable(gem_handle* h, long long capacity);
int  gem_global_push_local(gem_handle* h, int clear_local, int* out_index);
int  gem_global_push(gem_handle* h, const void* points, long long n, int* out_index);
int  gem_global_loop_closure(gem_handle* h, int n_opt, const float* transforms, const float* centres, float radius,
                             double resolution, long long* out_fused);
int  gem_global_export(gem_handle* h, int index, void* points, long long max_points, long long* out_count);
int  gem_global_count(gem_handle* h, int* out_submaps);

/* ---- the costmap layers (layers/: PointMapLayer, pointMap_layer.cpp:45-100; ElevationMapLayer, elevationMap_layer.cpp:42-87) -----
 * A costmap is a device-resident byte grid bound to the handle; a handle holds up to eight (a local one, a global one, a master).
 * costmap_2d is not part of this library and not part of the reference tree: its pieces are RESTATED here from ROS noetic
 * costmap_2d/src/costmap_2d.cpp and costmap_layer.cpp (tests/costmap_ref.py is the same statement in numpy).  The restatement is NOT
 * verified against the library (there is none here; tools/ros_selfcheck.cpp's `cost` row settles it in a ROS workspace).  All
 * arithmetic is in double unless marked.
 *   constants    FREE_SPACE 0, LETHAL_OBSTACLE 254, NO_INFORMATION 255.
 *   geometry     size_x, size_y (cells), resolution, origin_x, origin_y; index = my * size_x + mx;
 *                sizeInMetersX = (size_x - 1 + 0.5) * resolution, Y likewise.
 *   worldToMap   fails if wx < origin_x || wy < origin_y; else mx = (int)((wx - origin_x) / resolution), my likewise, and it succeeds
 *                iff mx < size_x && my < size_y.  A deliberate difference: a non-finite wx or wy, or a quotient that does not fit an
 *                int, fails (the reference's cast is undefined there).
 *   gem_costmap_mark_points        PointMapLayer::updateBounds:55-81 over n PointXYZRGBICT records (host; _device: device memory,
 *                untouched until gem_synchronize as for gem_add_device): for i = 0 .. n-1 IN ORDER px = (double)x, py = (double)y; a
 *                record worldToMap refuses is skipped; else costmap[index] = ((double)travers > travers_thresh) ? FREE_SPACE :
 *                LETHAL_OBSTACLE (a NaN travers is lethal), then touch(px, py): min_x = std::min(px, min_x), ... max_y = std::max(py,
 *                max_y).  The result is that of this sequential loop: the LAST record of a cell decides.
 *   gem_costmap_mark_grid_cloud    the same over the last capture's records (= gem_local_grid_cloud: grid_pc) where they lie.
 *   gem_costmap_mark_global        the same over submap `index` of the stack, or with -1 over all of them in stack order, as one
 *                input (= gem_global_export's records).
 *   gem_costmap_mark_visual        ElevationMapLayer::updateBounds:58-81 with the last capture (gem_local_capture) standing for
 *                visualMap_ as show() leaves it (EM.cpp:89-111): every one of the L * L cells is visited in grid_map's iteration order;
 *                its position is getPositionFromIndex in double from the capture's geometry; a kept cell carries its traver, every
 *                other cell NaN; is_obstacle = ((double)traver < travers_thresh), so a NaN cell is FREE_SPACE; worldToMap, the write
 *                and touch as for points.  The test is `<` here and `>` in the point layer: at traver == travers_thresh the two layers
 *                disagree, as the reference's do.
 *   gem_costmap_update_origin      Costmap2D::updateOrigin: cell_ox = (int)((new_origin_x - origin_x) / resolution), truncating toward
 *                zero, cell_oy likewise; both zero: nothing changes.  The new origin is origin + cell_o * resolution.  The overlap of
 *                the old and the new window keeps its cells at their new places (lower_left = min(max(cell_o, 0), size), upper_right =
 *                min(max(cell_o + size, 0), size)); every other cell becomes default_value.
 *   gem_costmap_roll_to            the rolling_window_ line of both updateBounds (:48-49 / :45-46):
 *                update_origin(robot_x - sizeInMetersX / 2, robot_y - sizeInMetersY / 2).
 *   gem_costmap_reset              resetMaps: every cell becomes default_value.  default_value is a creation parameter: ObstacleLayer
 *                (ElevationMapLayer's base) sets it to NO_INFORMATION or FREE_SPACE by track_unknown_space; PointMapLayer::onInitialize
 *                never sets it.
 *   gem_costmap_merge              onto master_id inside [min_i, max_i) x [min_j, max_j).  mode 0, PointMapLayer::updateCosts:86-100 =
 *                CostmapLayer::updateWithOverwrite: a layer cell that is not NO_INFORMATION replaces the master cell.  mode 1,
 *                updateWithMax: it replaces the master cell if that is NO_INFORMATION or smaller.  Equal sizes.
 *   gem_costmap_read               the window's bytes, row j at out + (j - min_j) * row_stride (row_stride >= max_i - min_i).
 *   gem_costmap_write              the reverse: the window's cells from the caller's bytes (setCost over a window): what other
 *                layers of the caller's left in a master (a static map, say) before a merge onto it.  Inflation costs and the
 *                footprint need no such round trip: gem_costmap_inflate (gem_hip_inflate.h), gem_costmap_clear_footprint.
 *   gem_costmap_geometry           the configuration with the origin after rolling.
 * bounds = {min_x, min_y, max_x, max_y}, in / out, merged as touch() does; they compare as values, not bits (with std::min a tie
 * between -0 and +0 depends on the order).  With bounds NULL a mark only enqueues on the handle's stream and nothing waits.
 * Left with the caller: useExtraBounds, enabled_, the subscriptions and the layered costmap itself (master_grid.setCost from
 * gem_costmap_read); updateFootprint / setConvexPolygonCost is gem_costmap_clear_footprint (gem_hip_footprint.h).  Every entry takes
 * the handle's lock.
 * GEM_ERR_INVALID, nothing changed: a bad id; a zero size (or more than 2^30 cells), a resolution not finite and positive, a
 * non-finite origin or threshold; n < 0 or n above 2^31 - 2 (mark_global: the records of the call together); a window outside the
 * map; mark_grid_cloud or mark_visual without a capture; mark_global without an enabled stack or with an index out of range; an
 * origin step whose cell count does not fit an int; a merge mode other than 0 or 1; a handle with a communicator. */
typedef struct gem_costmap_config {
    unsigned int  size_x, size_y;
    double        resolution, origin_x, origin_y;
    unsigned char default_value;       /* 255 or 0 */
} gem_costmap_config;
int  gem_costmap_create(gem_handle* h, const gem_costmap_config* cfg, int* out_id);
int  gem_costmap_destroy(gem_handle* h, int id);
int  gem_costmap_geometry(gem_handle* h, int id, gem_costmap_config* out);
int  gem_costmap_reset(gem_handle* h, int id);
int  gem_costmap_update_origin(gem_handle* h, int id, double new_origin_x, double new_origin_y);
int  gem_costmap_roll_to(gem_handle* h, int id, double robot_x, double robot_y);
int  gem_costmap_mark_points(gem_handle* h, int id, const void* points, long long n, double travers_thresh, double bounds[4]);
int  gem_costmap_mark_points_device(gem_handle* h, int id, const void* d_points, long long n, double travers_thresh, double bounds[4]);
int  gem_costmap_mark_grid_cloud(gem_handle* h, int id, double travers_thresh, double bounds[4]);
int  gem_costmap_mark_global(gem_handle* h, int id, int index, double travers_thresh, double bounds[4]);
int  gem_costmap_mark_visual(gem_handle* h, int id, double travers_thresh, double bounds[4]);
int  gem_costmap_merge(gem_handle* h, int id, int master_id, int min_i, int min_j, int max_i, int max_j, int mode);
int  gem_costmap_read(gem_handle* h, int id, int min_i, int min_j, int max_i, int max_j, unsigned char* out, size_t row_stride);
int  gem_costmap_write(gem_handle* h, int id, int min_i, int min_j, int max_i, int max_j, const unsigned char* in, size_t row_stride);

/* ---- pointCloudtoOctomap's insertion loop (EMg.cpp:1158-1173) and fullMapToMsg on the device ---------------------------------------
 *   gem_octree_build           a host PointXYZRGBICT cloud -> the byte stream octomap_msgs::fullMapToMsg would put into msg.data for
 *                              a cleared octomap::ColorOcTree after, per record IN ORDER, updateNode(point3d(x, y, z), true) and
 *                              integrateNodeColor(x, y, z, r, g, b), then updateInnerOccupancy().  The stream stays on the device.
 *   gem_octree_build_device    the same for a cloud in device memory (untouched until gem_synchronize, as for gem_add_device).
 *   gem_local_compose_octrees  gem_local_compose with the road and obstacle lists kept on the device and built into slots
 *                              GEM_OCTREE_ROAD and GEM_OCTREE_OBSTACLE: same counts and threshold, bit for bit, same preconditions.
 *   gem_octree_read            the stream of a slot.  data NULL: only *out_bytes.  capacity below the size: GEM_ERR_INVALID with
 *                              *out_bytes filled in.
 * octomap is not part of this library; the contract is RESTATED here from octomap 1.8 / 1.9 (OcTreeBaseImpl.hxx, OccupancyOcTreeBase.hxx,
 * ColorOcTree.cpp; tests/octree_ref.py is the same statement in Python, as a literal pointer tree and in the array form of the device):
 *   constants  tree_depth 16 (a root-to-leaf path has 17 nodes), tree_max_val 32768, rf = 1.0 / resolution in double.
 *              hit = (float)log(0.7 / 0.3); clamps cmax = (float)log(0.971 / 0.029), cmin = (float)log(0.1192 / 0.8808); a non-zero
 *              probability P of the parameters gives (float)log(P / (1 - P)) instead.  A new node has value 0.0f and colour
 *              (255, 255, 255), which means "not set": isColorSet is "any channel != 255".
 *   key        per axis k = (int)floor(rf * (double)coord) + 32768, valid iff 0 <= k < 65536; a point with an invalid key on any axis
 *              is skipped by both calls.  DELIBERATE DIFFERENCE: a non-finite coordinate is skipped (the library's cast is undefined).
 *              The child index at bit d of the keys is xbit + 2 ybit + 4 zbit.
 *   updateNode if search(key) finds a node whose value is >= cmax: nothing (search returns a childless node above depth 16: a pruned
 *              leaf).  Otherwise descend from the root: a missing child of a node that has no children and was not created in this
 *              call means the node is pruned, and it is expanded first (eight children, each copying its value and colour); otherwise
 *              the missing child is created.  At depth 16 value = value + hit in float, clamped to [cmin, cmax].  On the way back up,
 *              at every ancestor: pruneNode succeeds iff all eight children exist, none has children and all eight VALUES are equal
 *              (colour is ignored); the node then takes child 0's value and colour, and if that colour is set its colour becomes
 *              getAverageChildColor(); the children are deleted.  Otherwise value = max(children).
 *   integrateNodeColor   n = search(key).  Colour not set: n takes (r, g, b).  Otherwise p = 1. - 1. / (1. + exp((double)value)) and each
 *              channel becomes (uint8_t)((double)prev * p + (double)c * (0.99 - p)), in double, no FMA.
 *   updateInnerOccupancy bottom-up over every node that has children: value = max over the existing children; colour = per-channel
 *              integer mean (int sums, /= count) over the children whose colour is set, (255, 255, 255) if none is.  Nothing is pruned
 *              here or in the writer.
 *   stream     pre-order from the root; each node 8 bytes: value (float, little-endian), r, g, b, one byte with bit i set iff child i
 *              exists; children in index order.  DELIBERATE DIFFERENCE: an empty tree (no valid point) gives zero bytes.  The message's
 *              id "ColorOcTree", binary = false and resolution stay with the caller.
 * NOT verified against octomap (there is none here; tools/ros_selfcheck.cpp's `octo` row settles them in a ROS workspace): (1) that the
 * installed version prunes on value only and recolours a pruned node as above (1.8 and 1.9 should; 1.6 differs); (2) the host libm's
 * exp for the handful of values that occur; (3) that the colour blend is compiled without contraction; (4) the (uint8_t) cast of the
 * blend, which is always < 253 here; (5) the empty-tree case.
 * How it is built (gem_octree.hip): a leaf's value depends only on its number of hits, so the device carries saturating counts and two
 * host-built tables (value and p per count, at most 64 entries).  Colour depends on the prune / expand history, which is local to a
 * leaf's largest aligned block of 8^k leaves that are all hit (k*): the records are sorted stably by Morton key and every block is
 * walked in input order -- k* = 0 one lane per leaf, k* = 1 eight lanes per block, k* = 2 one wave per block; k* >= 3 (512 leaves
 * jointly) is finished by an exact sequential routine on the host, its records counted in fallback_points.
 * stats may be NULL.  GEM_ERR_INVALID, nothing changed: a slot outside 0 .. 3, params NULL, a resolution not finite and positive,
 * prob_hit <= 0.5 (when not 0), values not strictly increasing up to the clamp within 64 steps, n < 0 or above 2^31 - 2, points NULL
 * with n > 0, a handle with a communicator; gem_local_compose_octrees: gem_local_compose's cases too.  Every entry takes the handle's
 * lock. */
#define GEM_OCTREE_ROAD     0
#define GEM_OCTREE_OBSTACLE 1
#define GEM_OCTREE_USER0    2
#define GEM_OCTREE_USER1    3
typedef struct gem_octree_params {
    double resolution;        /* the tree's; the node uses 0.2 (road) and 0.1 (obstacle) */
    double prob_hit;          /* 0: octomap's 0.7 */
    double clamp_min;         /* 0: octomap's 0.1192 */
    double clamp_max;         /* 0: octomap's 0.971 */
    int    flags;             /* 0 */
} gem_octree_params;
typedef struct gem_octree_stats {
    long long points_in;          /* records of the call */
    long long points_keyed;       /* ... with a valid key */
    long long leaves_depth16;     /* childless nodes at depth 16 */
    long long pruned_leaves;      /* childless nodes above it */
    long long nodes;
    long long bytes;              /* 8 * nodes */
    long long coupled_blocks[3];  /* full aligned blocks walked jointly: k* = 1, 2, >= 3 */
    long long fallback_points;    /* records of the k* >= 3 blocks (host routine) */
} gem_octree_stats;
int  gem_octree_build(gem_handle* h, int slot, const gem_octree_params* params, const void* points, long long n, gem_octree_stats* stats);
int  gem_octree_build_device(gem_handle* h, int slot, const gem_octree_params* params, const void* d_points, long long n, gem_octree_stats* stats);
int  gem_local_compose_octrees(gem_handle* h, const gem_compose_params* p, const gem_octree_params* road_params,
                               const gem_octree_params* obstacle_params, int out_counts[3], double* out_threshold, gem_octree_stats stats[2]);
int  gem_octree_read(gem_handle* h, int slot, void* data, size_t capacity, size_t* out_bytes);

/* ---- the history cloud (visualCloud_): gem_history_*, gem_costmap_mark_history ------------------------------------------------ */
#include "gem_hip_history.h"

/* ---- footprints on the costmap: gem_costmap_clear_footprint, gem_costmap_footprint_cost*, gem_costmap_score_trajectories* ------- */
#include "gem_hip_footprint.h"

/* ---- inflation on the costmap: gem_inflation_table, gem_costmap_inflate, gem_costmap_reset_window ------------------------------- */
#include "gem_hip_inflate.h"

/* ---- path and goal distance grids on the costmap: gem_mapgrid_adjust_plan, gem_costmap_mapgrid_prepare / _read / _score* -------- */
#include "gem_hip_mapgrid.h"

/* ---- the best trajectory: gem_costmap_mapgrid_prepare_front / _read_front, gem_costmap_best_trajectory*, gem_critics_select ----- */
#include "gem_hip_critics.h"

/* ---- the distance grids on a costmap of any size: gem_costmap_mapgrid_prepare_tiled / _prepare_front_tiled ------------------------ */
#include "gem_hip_mapgrid_tiled.h"

/* ---- DWA's sampled trajectories: gem_trajgen_plan / _generate / _velocity / _generate_device, gem_costmap_dwa_best* -------------- */
#include "gem_hip_trajgen.h"

/* ---- trajectory rollout (TrajectoryPlanner::createTrajectories): gem_rollout_plan / _host / _pick, gem_costmap_rollout_best* ------ */
#include "gem_hip_rollout.h"

/* ---- the global plan: gem_navplan_weights, gem_navplan_host, gem_costmap_navplan / _status / _read -------------------------------- */
#include "gem_hip_navplan.h"

/* ---- frontier search: gem_frontiers_host, gem_costmap_frontiers / _read, gem_costmap_navplan_goal --------------------------------- */
#include "gem_hip_frontier.h"

/* ---- ObstacleLayer: gem_costmap_observe / _observe_device, gem_obstacle_host ------------------------------------------------------- */
#include "gem_hip_obstacle.h"

/* ---- VoxelLayer: gem_costmap_voxels_*, gem_costmap_voxel_observe / _observe_device, gem_voxlayer_host ------------------------------ */
#include "gem_hip_voxlayer.h"

/* ---- paths on the last plan's potential, grid or gradient, a batch of goals: gem_navpath_host, gem_costmap_navplan_paths / _device -- */
#include "gem_hip_navpath.h"

/* ---- the quadratic potential, order-free and exact: gem_navquad_host, gem_costmap_navplan_quadratic -------------------------------- */
#include "gem_hip_navquad.h"

#ifdef __cplusplus
}
#endif
#endif
