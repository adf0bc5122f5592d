/* gem_hip_footprint.h -- footprints on the device costmap: the part of the C ABI of libgem_hip.so that clears the robot's footprint out
 * of a layer (ObstacleLayer::updateFootprint + the setConvexPolygonCost line of ObstacleLayer::updateCosts, which ElevationMapLayer
 * inherits: layers/src/elevationMap_layer.cpp:86) and answers base_local_planner's footprintCost for batches of poses and whole
 * trajectories from the grid where it lies.  Included by gem_hip.h, not on its own.  Symbols only added: GEM_ABI_VERSION is unchanged.
 *
 * Every entry takes the handle's lock and runs on the handle's stream: marks enqueued before it (bounds NULL included) are visible to
 * it without a host wait.
 *
 * The contract is RESTATED from ROS noetic costmap_2d/src/footprint.cpp, costmap_2d.cpp, obstacle_layer.cpp,
 * costmap_2d/include/costmap_2d/line_iterator.h and base_local_planner/src/costmap_model.cpp (tests/footprint_ref.py is the same
 * statement in numpy).  It is NOT verified against the libraries (there are none here; tools/ros_selfcheck.cpp's `foot` row settles it
 * in a ROS workspace).  All arithmetic is in double, every operation rounded on its own (no contraction); cells are ints.
 *   pose             {x, y, cos_th, sin_th}: the caller supplies the cosine and the sine (the kernels hold no transcendental, so a result
 *                    does not depend on whose cos it was; the facades use the host's std::cos / std::sin).
 *   transformFootprint   vertex i of spec (sx_i, sy_i) becomes (x + (sx_i * cos_th - sy_i * sin_th), y + (sx_i * sin_th + sy_i * cos_th)).
 *   worldToMap       as in gem_hip.h, its deliberate failure on non-finite input included.
 *   line(x0, y0, x1, y1)   LineIterator: the cells of raytraceLine / bresenham2D without a length limit.  dx = |x1 - x0|, dy = |y1 - y0|,
 *                    xi = (x1 >= x0) ? 1 : -1, yi likewise.  dx >= dy: the cells are (x0 + xi * k, y0 + yi * m_k) for k = 0 .. dx with
 *                    m_k = (dx / 2 + k * dy) / dx in integer division (0 when dx == 0).  Otherwise the roles are swapped: k = 0 .. dy,
 *                    (x0 + xi * m_k, y0 + yi * k), m_k = (dy / 2 + k * dx) / dy.  (This closed form equals the iterator's own loop
 *                    num += numadd; if (num >= den) { num -= den; minor step }; tests/test_footprint_cpu.py compares the two.)
 *   pointCost(cell)  255 -> -2; 254 -> -1; 253 -> -1 iff GEM_FOOTPRINT_INSCRIBED_LETHAL; otherwise the byte.
 *   footprintCost(pose, spec[n])   worldToMap(x, y) fails: -3.  n < 3: the centre cell alone, 255 -> -2, 254 or 253 -> -1 (whatever the
 *                    flag), otherwise the byte.  Otherwise for i = 0 .. n-1 IN ORDER, j = (i + 1) % n: if worldToMap of vertex i or of
 *                    vertex j fails the answer is -3; else line(cell_i, cell_j) is walked in order and the first negative pointCost is
 *                    the answer.  If nothing is negative the answer is the maximum pointCost over all edges (0 at least).  The answer is
 *                    that of this sequential loop: the FIRST negative event in walk order decides between -1, -2 and -3.  With n >= 3
 *                    the centre cell is tested for being on the map but not read.  Results are int: -3, -2, -1 or 0 .. 253.
 *   trajectories     trajectory t owns poses [t * T, (t + 1) * T), T = poses_per_traj.  Its score is the first negative pose result in
 *                    pose order; without one the maximum of the pose results, or with GEM_FOOTPRINT_SUM their sum (an int; T <= 2^20
 *                    keeps it from overflowing): the loop of ObstacleCostFunction::scoreTrajectory.
 *   gem_costmap_clear_footprint    updateFootprint and the footprint line of ObstacleLayer::updateCosts in one call: the spec is
 *                    transformed; every vertex IN ORDER is touch()ed into bounds (min_x = std::min(px, min_x), ...), on the map or not;
 *                    then setConvexPolygonCost(FREE_SPACE): n < 3 writes nothing, ok = 1; a vertex worldToMap refuses writes nothing,
 *                    ok = 0; otherwise with O the cells of line(cell_i, cell_(i+1)%n) for all i, every cell (x, y) of a column x that
 *                    occurs in O with min{y : (x, y) in O} <= y <= max{...} becomes 0, ok = 1 (polygonOutlineCells + convexFillCells as
 *                    a set).  bounds and *out_ok are computed on the host, which knows the geometry after rolling: the call only
 *                    enqueues.
 *   gem_costmap_footprint_cost     footprintCost of n poses (host arrays; the call waits).  _device: poses and results in device memory;
 *                    the call only enqueues and the buffers are untouched until gem_synchronize, as for gem_add_device.
 *   gem_costmap_score_trajectories n_traj trajectories of poses_per_traj poses each -> out_traj_cost[n_traj], and with out_pose_cost
 *                    not NULL also every pose's footprintCost.  _device as above.
 * spec_xy is always host memory: n_vertices pairs, 0 <= n_vertices <= GEM_FOOTPRINT_MAX_VERTICES.  The scratch buffers of the host-array
 * forms come from the handle's arenas; their capacity only grows, so a loop that has reached its sizes allocates nothing.
 *
 * GEM_ERR_INVALID, nothing written and the grid untouched: a bad id; a handle with a communicator; n < 0, n_traj < 0 or n_traj *
 * poses_per_traj above 2^31 - 2; poses_per_traj outside [1, 2^20]; n_vertices out of range; a non-finite spec coordinate; unknown flag
 * bits; a NULL array with a non-zero count; in gem_costmap_clear_footprint a NULL or non-finite pose.  In the scoring calls a
 * non-finite pose simply answers -3. */
typedef struct gem_footprint_pose { double x, y, cos_th, sin_th; } gem_footprint_pose;   /* 32 bytes */
#define GEM_FOOTPRINT_MAX_VERTICES 32
#define GEM_FOOTPRINT_INSCRIBED_LETHAL 1   /* 253 on an edge cell also answers -1 */
#define GEM_FOOTPRINT_SUM              2   /* trajectories: sum instead of max */
int  gem_costmap_clear_footprint(gem_handle* h, int id, const gem_footprint_pose* pose, const double* spec_xy, int n_vertices,
                                 double bounds[4], int* out_ok);
int  gem_costmap_footprint_cost(gem_handle* h, int id, const gem_footprint_pose* poses, long long n, const double* spec_xy,
                                int n_vertices, int flags, int* out_cost);
int  gem_costmap_footprint_cost_device(gem_handle* h, int id, const gem_footprint_pose* d_poses, long long n, const double* spec_xy,
                                       int n_vertices, int flags, int* d_out_cost);
int  gem_costmap_score_trajectories(gem_handle* h, int id, const gem_footprint_pose* poses, long long n_traj, int poses_per_traj,
                                    const double* spec_xy, int n_vertices, int flags, int* out_pose_cost, int* out_traj_cost);
int  gem_costmap_score_trajectories_device(gem_handle* h, int id, const gem_footprint_pose* d_poses, long long n_traj, int poses_per_traj,
                                           const double* spec_xy, int n_vertices, int flags, int* d_out_pose_cost, int* d_out_traj_cost);
