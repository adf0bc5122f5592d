/* gem_hip_obstacle.h -- ObstacleLayer on the device costmap: the part of the C ABI of libgem_hip.so that runs the standard
 * costmap_2d::ObstacleLayer::updateBounds over a set of observations -- rays from the sensor through every return clear the cells they
 * cross, then the returns mark.  ElevationMapLayer derives from ObstacleLayer and calls ObstacleLayer::onInitialize()
 * (layers/src/elevationMap_layer.cpp:16), so a configuration with observation_sources expects it.  Included by gem_hip.h, not on its
 * own.  Symbols only added: GEM_ABI_VERSION is unchanged.
 *
 * Both device entries take the handle's lock and run on the handle's stream: whatever was enqueued before them (bounds NULL included)
 * is visible to them without a host wait, and with bounds NULL they only enqueue themselves.
 *
 * The contract is RESTATED from ROS noetic costmap_2d/plugins/obstacle_layer.cpp (updateBounds, raytraceFreespace,
 * updateRaytraceBounds), costmap_2d/src/observation_buffer.cpp (the height window of bufferCloud) and
 * costmap_2d/include/costmap_2d/costmap_2d.h (raytraceLine, bresenham2D, cellDistance); tests/obstacle_ref.py is the same statement in
 * numpy.  It is NOT verified against the library (there is none here; tools/ros_selfcheck.cpp's `obs` row settles it in a ROS
 * workspace).  All arithmetic is in double, every operation rounded on its own (no contraction); cells are ints.  std::min(a, b) is
 * (b < a) ? b : a and std::max(a, b) is (a < b) ? b : a wherever they occur below, so a NaN second argument leaves the first.
 *
 *   the result       is a SET FUNCTION of the call: a cell is 254 if an accepted marking record lies in it, else 0 if a ray of a
 *                    clearing observation crosses it, else unchanged.  (updateBounds runs every clearing observation first and every
 *                    marking one after them; every write of the first kind stores FREE_SPACE, every one of the second
 *                    LETHAL_OBSTACLE: no visiting order is left to decide anything.)
 *   record i         of an observation lies at points + i * point_step: float x, y, z at byte offsets 0, 4, 8, in the global frame;
 *                    wx = (double)x and so on.
 *   buffer filter    (ObservationBuffer::bufferCloud) a record belongs to its observation iff min_obstacle_height <= (double)z and
 *                    (double)z <= max_obstacle_height; a NaN z drops it.  This applies to both uses of the observation.
 *   worldToMap       as in gem_hip.h, its deliberate failure on non-finite input included.
 *   cellDistance(d)  c = std::max(0.0, ceil(d / resolution)), then (unsigned)c; here a c of 4294967295 or more gives 4294967295 (the
 *                    library's cast is undefined there).
 *   line(x0, y0, x1, y1)   as in gem_hip_footprint.h.  raytraceLine / bresenham2D with max_length walks a PREFIX of it: with dx = x1 - x0,
 *                    dy = y1 - y0, da = max(|dx|, |dy|): dist = sqrt((double)(dx * dx + dy * dy)) (the sum in 64-bit integers),
 *                    scale = (dist == 0.0) ? 1.0 : std::min(1.0, (double)max_length / dist), end = std::min((unsigned)(scale * da), da);
 *                    the cells k = 0 .. end of line() are visited.  (bresenham2D's own loop -- error_b starts at da / 2, error_b +=
 *                    db, a minor step and error_b -= da when (unsigned)error_b >= da -- puts its k-th cell at minor offset
 *                    (da / 2 + k * db) / da, the closed form; tests/test_obstacle_cpu.py compares the two.)
 *   clearing         (raytraceFreespace) for every observation with GEM_OBS_CLEARING, in order, before any marking, with (ox, oy) =
 *                    origin[0], origin[1]:  worldToMap(ox, oy) fails: the observation clears nothing and touches nothing.  Otherwise
 *                    (x0, y0) is the origin's cell and touch(ox, oy).  map_end_x = origin_x + size_x * resolution, map_end_y likewise.
 *                    Per record of the observation: a = wx - ox, b = wy - oy, then four clips in this order, each an `if`, the later
 *                    ones seeing the earlier ones' result:
 *                      wx < origin_x:  t = (origin_x - ox) / a;  wx = origin_x;          wy = oy + b * t
 *                      wy < origin_y:  t = (origin_y - oy) / b;  wx = ox + a * t;        wy = origin_y
 *                      wx > map_end_x: t = (map_end_x - ox) / a; wx = map_end_x - .001;  wy = oy + b * t
 *                      wy > map_end_y: t = (map_end_y - oy) / b; wx = ox + a * t;        wy = map_end_y - .001
 *                    worldToMap(wx, wy) fails: the record is skipped (non-finite fails, which absorbs a == 0 or b == 0 with an infinite
 *                    t).  Otherwise (x1, y1) is its cell, the cells of raytraceLine(x0, y0, x1, y1, cellDistance(raytrace_range))
 *                    become 0, and updateRaytraceBounds: ddx = wx - ox, ddy = wy - oy over the clipped point, full = sqrt(ddx * ddx +
 *                    ddy * ddy), s = std::min(1.0, raytrace_range / full), touch(ox + ddx * s, oy + ddy * s).
 *   marking          (updateBounds) for every observation with GEM_OBS_MARKING, per record of it with (px, py, pz) = (wx, wy, wz):
 *                    pz > layer_max_obstacle_height: skipped.  sq = (px - ox) * (px - ox) + (py - oy) * (py - oy) + (pz - oz) * (pz -
 *                    oz), summed left to right; sq >= obstacle_range * obstacle_range: skipped.  worldToMap(px, py) fails: skipped.
 *                    Otherwise the cell becomes 254 and touch(px, py).
 *   touch(x, y)      min_x = std::min(x, min_x), min_y = std::min(y, min_y), max_x = std::max(x, max_x), max_y = std::max(y, max_y).
 *                    bounds is in / out as in gem_costmap_mark_points and is compared as values (a -0.0 may come back as 0.0).  With
 *                    bounds NULL the device entries only enqueue.
 *   NAMED DEPARTURES both sqrt(x * x + y * y) above stand where the library calls hypot(); the integer one is exact up to the rounding
 *                    of the square root, the double one may differ from hypot in the last place.
 *   NOT PROVIDED     obstacle_min_range / raytrace_min_range (later releases), the buffers' time-keeping (observation_keep_time,
 *                    expected_update_rate) and TF -- the caller hands over the observations that are current, in the global frame --,
 *                    footprint clearing (gem_costmap_clear_footprint is that).  VoxelLayer is gem_hip_voxlayer.h.
 *
 * gem_costmap_observe takes `points` in host memory, gem_costmap_observe_device in device memory, untouched until gem_synchronize as
 * for gem_add_device.  gem_obstacle_host is the host twin: the same statement in plain C++ on a caller's grid (row-major, size_y rows
 * of size_x bytes), no handle, no device.  An observe call counts as a change of the grid: plans, searches and distance grids made
 * before it are refused as stale until they are made again.  The scratch buffers come from the handle's arenas; their capacity only
 * grows, so a loop that has reached its sizes allocates nothing.
 *
 * GEM_ERR_INVALID, nothing changed: a bad id, or a handle with a communicator (device entries); a NULL grid or geometry, a size of
 * zero or above 2^30 cells, a resolution not finite and positive or a non-finite origin (host twin); n_obs outside [0, GEM_OBS_MAX], or
 * obs NULL with n_obs > 0; n < 0, or more than 2^31 - 2 records in the call; a point_step below 12 or no multiple of 4; flags empty
 * or with unknown bits; a non-finite origin; a negative or NaN range (+inf is a range); a NaN height, or min_obstacle_height >
 * max_obstacle_height; a NaN layer_max_obstacle_height; NULL points with n > 0. */
typedef struct gem_observation {
    const void* points;        /* record i at points + i * point_step: float x, y, z at byte offsets 0, 4, 8; global frame */
    long long   n;
    unsigned    point_step;    /* >= 12, a multiple of 4: 12 packed, 16 = the xyzi of gem_add_device, 32 = PointXYZRGBICT */
    unsigned    flags;         /* GEM_OBS_MARKING | GEM_OBS_CLEARING, at least one */
    double      origin[3];
    double      obstacle_range, raytrace_range;
    double      min_obstacle_height, max_obstacle_height;   /* the ObservationBuffer's window */
} gem_observation;             /* 80 bytes */
#define GEM_OBS_MARKING  1
#define GEM_OBS_CLEARING 2
#define GEM_OBS_MAX 8
int  gem_costmap_observe(gem_handle* h, int id, const gem_observation* obs, int n_obs, double layer_max_obstacle_height, double bounds[4]);
int  gem_costmap_observe_device(gem_handle* h, int id, const gem_observation* obs, int n_obs, double layer_max_obstacle_height,
                                double bounds[4]);
int  gem_obstacle_host(unsigned char* grid, const gem_costmap_config* geom, const gem_observation* obs, int n_obs,
                       double layer_max_obstacle_height, double bounds[4]);
