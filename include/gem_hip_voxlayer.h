/* gem_hip_voxlayer.h -- VoxelLayer on the device costmap: the part of the C ABI of libgem_hip.so that runs the standard
 * costmap_2d::VoxelLayer::updateBounds over a set of observations on a costmap with a voxel grid attached -- 3-D rays from the sensor
 * through every return clear the voxels they cross, then the returns mark voxels, and a cell turns free, unknown or lethal by the bit
 * counts of its column.  It is the plugin for a 3-D sensor: a ray that passes under an overhang or over a low obstacle does not wipe
 * it, as the 2-D ObstacleLayer (gem_hip_obstacle.h) does.  Included by gem_hip.h, not on its own.  Symbols only added:
 * GEM_ABI_VERSION is unchanged.  gem_observation, its flags and GEM_OBS_MAX are gem_hip_obstacle.h's, unchanged.
 *
 * Both device entries take the handle's lock and run on the handle's stream: whatever was enqueued before them (bounds NULL included)
 * is visible to them without a host wait, and with bounds NULL they only enqueue themselves.
 *
 * The contract is RESTATED FROM MEMORY of ROS noetic costmap_2d/plugins/voxel_layer.cpp (updateBounds, raytraceFreespace, resetMaps,
 * updateOrigin) and voxel_grid/include/voxel_grid/voxel_grid.h (markVoxelInMap, clearVoxelLineInMap, raytraceLine, bresenham3D,
 * bitsBelowThreshold); tests/voxlayer_ref.py is the same statement in numpy, twice.  It is UNVERIFIED AGAINST THE LIBRARY (there is
 * none here; tools/ros_selfcheck.cpp's `voxel` row names what would settle it in a ROS workspace); the OPEN POINTS are listed below.
 * All arithmetic is in double, every operation rounded on its own (no contraction); voxel indices are ints.  std::min(a, b) is
 * (b < a) ? b : a and std::max(a, b) is (a < b) ? b : a wherever they occur below, so a NaN second argument leaves the first.
 * cellDistance, the buffer's height window, record i of an observation, touch() and updateRaytraceBounds are gem_hip_obstacle.h's.
 *
 *   voxel grid       one uint32_t COLUMN per cell, size_z in 1 .. 16 voxels of z_resolution from origin_z upwards.  Bit z (the low
 *                    half) is "not known free", bit 16 + z is "marked": a voxel is UNKNOWN when only the low bit is set, MARKED when
 *                    both are, FREE when neither is.  Reset makes every column 0x0000FFFF.  below(n, thr) = popcount(n) <= thr,
 *                    marked(col) = col >> 16, unknown(col) = (uint16_t)(col >> 16) ^ (uint16_t)col.
 *   worldToMap3DFloat(wx, wy, wz)   fails if wx < origin_x || wy < origin_y || wz < origin_z; otherwise fx = (wx - origin_x) /
 *                    resolution, fy likewise, fz = (wz - origin_z) / z_resolution, and it succeeds iff fx < size_x && fy < size_y &&
 *                    fz < size_z.  Non-finite input fails, as elsewhere in this family.
 *   worldToMap3D     the same pre-test, then each quotient truncated to int and the same < tests on the integers (a quotient of 2^31
 *                    or more fails).
 *   raytraceLine(x0, y0, z0, x1, y1, z1, max_length)   on double voxel coordinates: dx = (int)x1 - (int)x0, dy, dz likewise; dist =
 *                    sqrt((x0 - x1) * (x0 - x1) + (y0 - y1) * (y0 - y1) + (z0 - z1) * (z0 - z1)) on the doubles, summed left to
 *                    right; scale = std::min(1.0, (double)max_length / dist) (a zero dist gives +inf or NaN, both leave 1.0).  The
 *                    dominant axis is x if |dx| >= max(|dy|, |dz|), else y if |dy| >= |dz|, else z; da is its absolute delta; end =
 *                    min((unsigned)(scale * da), da).  The voxels k = 0 .. end are visited: voxel k lies k steps along the dominant
 *                    axis and (da / 2 + k * db) / da (integer division) steps along each of the other two -- the closed form of
 *                    bresenham3D, whose two errors start at da / 2, grow by db per step and take a minor step with error -= da when
 *                    (unsigned)error >= da; tests/test_voxlayer_cpu.py compares the two.  The z step shifts the mask
 *                    ((1 << 16) | 1) << z by one.
 *   clearing         (raytraceFreespace) for every observation with GEM_OBS_CLEARING, in order, before any marking, with (ox, oy, oz)
 *                    = origin.  An observation with no record in its height window does nothing.  worldToMap3DFloat(ox, oy, oz)
 *                    gives the sensor's voxel coordinates; if it fails the observation clears nothing and touches nothing.  There is
 *                    NO touch(ox, oy).  map_end_x = origin_x + (size_x - 1 + 0.5) * resolution, map_end_y likewise
 *                    (getSizeInMetersX).  Per record of the observation:
 *                      d = sqrt((wx - ox)^2 + (wy - oy)^2 + (wz - oz)^2);  f = std::max(std::min(1.0, (d - 2 * resolution) / d), 0.0);
 *                      wx = f * (wx - ox) + ox, wy, wz likewise;  a = wx - ox, b = wy - oy, c = wz - oz, t = 1.0;
 *                      if wz > layer_max_obstacle_height: t = std::max(0.0, std::min(t, (layer_max_obstacle_height - 0.01 - oz) / c))
 *                      else if wz < origin_z:             t = std::min(t, (origin_z - oz) / c)
 *                      then four ifs, each t = std::min(t, ...):  wx < origin_x: (origin_x - ox) / a;  wy < origin_y: (origin_y - oy) / b;
 *                      wx > map_end_x: (map_end_x - ox) / a;  wy > map_end_y: (map_end_y - oy) / b;
 *                      wx = ox + a * t, wy, wz likewise.
 *                    worldToMap3DFloat(wx, wy, wz) fails: the record is skipped.  Otherwise every voxel of raytraceLine(sensor, point,
 *                    cellDistance(raytrace_range)) has both of its bits cleared in its column and its cell is TOUCHED, and
 *                    updateRaytraceBounds(ox, oy, wx, wy, raytrace_range) runs exactly as in gem_hip_obstacle.h.
 *   marking          for every observation with GEM_OBS_MARKING, per record (px, py, pz) of it: pz > layer_max_obstacle_height:
 *                    skipped.  sq = (px - ox)^2 + (py - oy)^2 + (pz - oz)^2 summed left to right; sq >= obstacle_range *
 *                    obstacle_range: skipped.  worldToMap3D(px, py, pz < origin_z ? origin_z : pz) fails: skipped.  Otherwise both
 *                    bits of voxel z are set in the column and the record is ACCEPTED.
 *   the result       is a SET FUNCTION of the call.  The library writes a cell's byte as it goes: a cleared voxel's cell becomes,
 *                    if below(marked(col), mark_threshold), 0 or 255 by below(unknown(col), unknown_threshold); a marked voxel's cell
 *                    becomes 254 if !below(marked(col), mark_threshold).  Clearing only removes bits, marking only adds them, and all
 *                    clears precede all marks, so both threshold tests are monotone within their phase: once the clearing test on
 *                    marked() holds it keeps holding, and once the marking test holds it keeps holding.  The last clear of a cell and
 *                    the last mark of a cell therefore see the column's final state of their phase, and the last write wins.  With
 *                    col_c the column after every clear and col_f = col_c with the accepted marks OR-ed in, the cell's byte is
 *                      254 if the cell has an accepted record and !below(marked(col_f), mark_threshold);
 *                      otherwise, if the cell was touched and below(marked(col_c), mark_threshold):
 *                          below(unknown(col_c), unknown_threshold) ? 0 : 255;
 *                      otherwise unchanged.
 *                    The stored column is col_f.
 *   bounds           in / out and may be NULL, as for gem_costmap_observe.  Clearing touches through updateRaytraceBounds.  THE ONE
 *                    NAMED DEPARTURE: the library calls touch(px, py) only for a record whose own markVoxelInMap returned true,
 *                    which with mark_threshold > 0 depends on the order of the records in a column.  Here EVERY accepted record of a
 *                    cell that ends 254 by the first line of the rule touches.  With mark_threshold == 0 the two are identical;
 *                    above 0 the bounds here are a superset -- they are an update-region hint.
 *   OPEN POINTS      (each is this restatement's reading, not checked against the library) the popcount <= thr reading of
 *                    bitsBelowThreshold; no touch of the sensor in raytraceFreespace; getSizeInMetersX for map_end; the 2 * resolution
 *                    shortening of every ray; sqrt where the library may call hypot.
 *   NOT PROVIDED     clearNonLethal, the clearing-endpoints and voxel-grid publishers, footprint_clearing (gem_costmap_clear_footprint
 *                    is that), the buffers' time-keeping, and obstacle_min_range / raytrace_min_range.
 *
 * gem_costmap_voxels_create attaches a voxel grid to a costmap, every column unknown; gem_costmap_voxels_destroy detaches it;
 * gem_costmap_voxels_read / _write move a window's columns (row-major, row_stride_words >= the window's width) as gem_costmap_read /
 * _write move the bytes.  A costmap with voxels attached: gem_costmap_reset also resets the columns (VoxelLayer::resetMaps);
 * gem_costmap_update_origin and _roll_to also move the columns by the same overlap rule, everything outside the overlap unknown
 * (VoxelLayer::updateOrigin); gem_costmap_destroy frees them; gem_costmap_reset_window leaves them alone (the library's windowed
 * resetMap is Costmap2D's).  A costmap without voxels takes exactly the paths it took before.
 *
 * gem_costmap_voxel_observe takes `points` in host memory, gem_costmap_voxel_observe_device in device memory, untouched until
 * gem_synchronize.  gem_voxlayer_host is the host twin: the same statement in plain C++ on a caller's grid and columns (row-major,
 * size_y rows of size_x), no handle, no device.  Both observe calls count as a change of the grid: plans, searches and distance grids
 * made before are refused as stale.  The scratch comes from the handle's arenas; its capacity only grows.
 *
 * GEM_ERR_INVALID, nothing changed: everything gem_costmap_observe refuses (gem_obstacle_host for the host twin); size_z outside
 * 1 .. 16; a z_resolution not finite and positive; a non-finite origin_z; a threshold above 16; a NULL configuration; voxels attached
 * twice; destroy, observe, read or write on a costmap without voxels; a window outside the map, or a NULL array or a row stride below
 * the width with a window that is not empty; a NULL `columns` in the host twin. */
typedef struct gem_voxel_config {
    unsigned size_z;               /* 1 .. 16 */
    double   z_resolution, origin_z;
    unsigned unknown_threshold;    /* a cleared column with more unknown voxels than this is NO_INFORMATION, else FREE_SPACE */
    unsigned mark_threshold;       /* a column with more marked voxels than this is LETHAL_OBSTACLE */
} gem_voxel_config;
int  gem_costmap_voxels_create(gem_handle* h, int id, const gem_voxel_config* cfg);
int  gem_costmap_voxels_destroy(gem_handle* h, int id);
int  gem_costmap_voxels_read(gem_handle* h, int id, int min_i, int min_j, int max_i, int max_j, unsigned* out, size_t row_stride_words);
int  gem_costmap_voxels_write(gem_handle* h, int id, int min_i, int min_j, int max_i, int max_j, const unsigned* in, size_t row_stride_words);
int  gem_costmap_voxel_observe(gem_handle* h, int id, const gem_observation* obs, int n_obs, double layer_max_obstacle_height,
                               double bounds[4]);
int  gem_costmap_voxel_observe_device(gem_handle* h, int id, const gem_observation* obs, int n_obs, double layer_max_obstacle_height,
                                      double bounds[4]);
int  gem_voxlayer_host(unsigned char* grid, unsigned* columns, const gem_costmap_config* geom, const gem_voxel_config* voxels,
                       const gem_observation* obs, int n_obs, double layer_max_obstacle_height, double bounds[4]);
