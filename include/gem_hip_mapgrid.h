/* gem_hip_mapgrid.h -- path and goal distance grids on the device costmap: the part of the C ABI of libgem_hip.so that computes
 * base_local_planner's MapGrid (path_dist / goal_dist) through the free cells of a costmap where it lies and answers
 * MapGridCostFunction::scoreTrajectory for batches of trajectories.  Included by gem_hip.h, not on its own.  Symbols only added:
 * GEM_ABI_VERSION is unchanged.
 *
 * Every device entry takes the handle's lock and runs on the handle's stream: marks, merges and inflation enqueued before a
 * prepare are visible to it without a host wait, and a scoring call behind it sees its grids.  A cycle is
 *     reset_window(master) -> mark -> clear_footprint -> merge -> inflate -> mapgrid_prepare -> score_trajectories + mapgrid_score,
 * and the first host wait is the one for the scores.  With gem_costmap_mapgrid_prepare_tiled in the prepare's place (a map above
 * GEM_MAPGRID_MAX_WORDS, a large local map) the first host wait of a cycle is the PREPARE, not the scores: that call waits, its round
 * count depends on the data.
 *
 * The contract is RESTATED from ROS noetic base_local_planner: src/map_grid.cpp (computeTargetDistance, updatePathCell,
 * adjustPlanResolution, setTargetCells, setLocalGoal), include/base_local_planner/map_cell.h and src/map_grid_cost_function.cpp
 * (tests/mapgrid_ref.py is the same statement in numpy / plain Python).  It is NOT verified against the library (there is none
 * here; tools/ros_selfcheck.cpp's `mapgrid` row settles it in a ROS workspace).  The costmap is size_x x size_y bytes, grid[y][x];
 * worldToMap is the one of gem_hip.h, its deliberate refusal of non-finite input included.
 *   constants    OB = size_x * size_y (obstacleCosts()), UN = OB + 1 (unreachableCellCosts()).  A cell is BLOCKED iff its byte is
 *                253, 254 or 255.  within_robot is never set on this path and is not modelled.
 *   adjustPlanResolution(plan, resolution)   on the host, in double, every operation rounded on its own.  An empty plan stays empty.
 *                Out starts with point 0, last = plan[0].  For i = 1 ..: sq = (x_i - last_x)^2 + (y_i - last_y)^2; if
 *                sq > resolution^2: steps = (int)ceil(sqrt(sq) / resolution), dx = (x_i - last_x) / steps, dy likewise, and
 *                (last_x + j * dx, last_y + j * dy) is appended for j = 1 .. steps - 1.  Then point i is appended, last = plan[i].
 *   the run      point i of the adjusted plan is ACCEPTED iff worldToMap succeeds and the cell's byte, when the call runs on the
 *                stream, is not 255.  a is the first accepted index, b the first index above a that is not accepted (n without one).
 *                No accepted point: started = 0 and both grids are UN everywhere (the library returns after resetPathDist).  The
 *                path grid's sources are the cells of points a .. b-1 (setTargetCells; duplicates are harmless), the goal grid's
 *                single source is the cell of point b-1 (setLocalGoal).  A source may be a 253 or 254 cell.
 *   computeTargetDistance   the library's FIFO queue, stated as a set (tests/test_mapgrid_cpu.py compares the two on random
 *                grids).  Sources get 0.  A non-blocked, non-source cell gets the length of the shortest 4-connected path from any
 *                source whose cells after the source are all non-blocked; UN without such a path.  With E the sources together
 *                with the reached non-blocked cells, a blocked non-source cell gets OB if it has a 4-neighbour in E, else UN.
 *                Distances are int32, size_y rows of size_x.
 *   MapGridCostFunction::scoreTrajectory   the pose is gem_footprint_pose {x, y, cos_th, sin_th}.  xshift != 0: px = x + xshift *
 *                cos_th, py = y + xshift * sin_th in double, each product rounded before the sum; otherwise px = x, py = y.
 *                (yshift is NOT provided: the library takes cos(pth + M_PI_2), the kernels hold no transcendental, and DWA leaves
 *                it 0.)  Walking a trajectory's poses in order: worldToMap(px, py) fails -> the answer is -4.  Otherwise d =
 *                dist[cell]; with GEM_MAPGRID_STOP_ON_FAILURE d == OB answers -3 and d == UN answers -2.  Otherwise the aggregate:
 *                Last (the default) cost = d; GEM_MAPGRID_SUM cost += d in 64 bits.  The answer is that of the sequential loop:
 *                the FIRST negative event in pose order decides, otherwise the aggregate.  (Product is NOT provided: it leaves the
 *                exact integers after a few poses.)  Results are long long.  Trajectory t owns poses [t * T, (t + 1) * T),
 *                T = poses_per_traj, as in gem_costmap_score_trajectories.
 * Combining the critics (obstacle, path_dist, goal_dist, goal_front, alignment) into one cost and picking the winner is
 * gem_costmap_best_trajectory of gem_hip_critics.h, which also keeps goal_front's own grid (FRONT); these calls know PATH and GOAL.
 *
 *   gem_mapgrid_adjust_plan   host only, no handle and no device: *out_n = the adjusted plan's point count, and with out_xy not
 *                NULL its points (cap = the pairs out_xy holds; fewer than *out_n: GEM_ERR_INVALID, *out_n still set).
 *   gem_costmap_mapgrid_prepare   `which` is a mask of GEM_MAPGRID_PATH | GEM_MAPGRID_GOAL.  On the host, under the handle's lock,
 *                the plan (host memory, n pairs) is adjusted to the costmap's resolution and worldToMap applied with the geometry
 *                after rolling; the cells (or "off the map") go to the device through pinned staging.  The call only ENQUEUES: the
 *                reset of the requested grids to UN, the run test against the grid's bytes and the distance search (one workgroup
 *                per grid, PATH | GOAL one launch of two).  The grids live with the costmap in arenas that only grow: a second
 *                identical call allocates nothing.  An empty plan is valid: started = 0.
 *   gem_costmap_mapgrid_read   waits.  which_one is GEM_MAPGRID_PATH or GEM_MAPGRID_GOAL.  out (may be NULL): the size_y x size_x
 *                distances; *out_started; out_goal_cell = the (x, y) of point b-1, (-1, -1) without one.
 *   gem_costmap_mapgrid_score   n_traj trajectories of poses_per_traj poses each (host arrays; the call waits) -> out_traj[n_traj].
 *                _device: poses and results in device memory; the call only enqueues and the buffers are untouched until
 *                gem_synchronize, as for gem_costmap_score_trajectories_device.  A non-finite pose simply answers -4.
 * gem_costmap_mapgrid_prepare keeps the whole search in one workgroup's LDS, so ceil(size_x / 64) * size_y must not exceed
 * GEM_MAPGRID_MAX_WORDS there (512 x 512 is the largest square; 513 x 66 and 70 x 520 fit, 1 x 4100 does not).
 *   gem_costmap_mapgrid_prepare_tiled   the same grids on a costmap of ANY size: the sections `constants`, `the run` and
 *                `computeTargetDistance` above apply unchanged, to the byte.  The distances live in global memory and are relaxed tile
 *                by tile of 64 x 64 cells, one launch per round over every tile, a tile that no neighbour changed leaving at once
 *                (the protocol of gem_costmap_navplan's potential; computeTargetDistance is its unit-weight, multi-source case).
 *                The grids land in the same slots with the same status words and generation, so gem_costmap_mapgrid_read, _score,
 *                _score_device, gem_costmap_best_trajectory, _dwa_best and _rollout_best work behind it without a change.  The call
 *                WAITS: the round count depends on the data, as in gem_costmap_navplan; rounds are enqueued in chunks of tiles_x +
 *                tiles_y, each closed by a read of a converged word in pinned host memory.  The requested grids count as never
 *                prepared from before the first launch until convergence: a failure in between leaves no half-relaxed grid to read.
 *                Not converged within size_x * size_y + 2 rounds (it cannot happen): GEM_ERR_HIP.  *st (may be NULL): started and
 *                goal_cell as gem_costmap_mapgrid_read answers them; rounds = launches that found an active tile (it depends on
 *                timing, the grids do not); chunks = host round trips.  A second identical call allocates nothing.  Its error cases
 *                are gem_costmap_mapgrid_prepare's without the cap.  (gem_costmap_mapgrid_prepare_front_tiled is
 *                the same for the FRONT grid; both are declared in gem_hip_mapgrid_tiled.h.)  gem_costmap_mapgrid_prepare itself still only enqueues and still refuses a map above
 *                the cap: nothing dispatches from it to the tiled form.
 *
 * GEM_ERR_INVALID, nothing enqueued and nothing changed: a bad id; a handle with a communicator; a NULL array with a non-zero
 * count; n < 0, n_traj < 0, n_traj * poses_per_traj above 2^31 - 2, poses_per_traj outside [1, 2^20]; a non-finite plan coordinate
 * or xshift; a resolution not finite and positive (gem_mapgrid_adjust_plan); an adjusted plan above GEM_MAPGRID_MAX_POINTS; `which`
 * empty or with unknown bits, which_one not exactly one grid, unknown flag bits; a map above GEM_MAPGRID_MAX_WORDS (the capped prepare alone); scoring or reading
 * a grid that was never prepared, or was prepared before the costmap last rolled (gem_costmap_update_origin / _roll_to moved it), was
 * observed (gem_costmap_observe* or gem_costmap_voxel_observe* with at least one observation: gem_hip_obstacle.h, gem_hip_voxlayer.h) or
 * was created anew: the host keeps a generation number per costmap (the library recomputes the grids every cycle for the same
 * reason).  A refusal of the capped prepare leaves grids that gem_costmap_mapgrid_prepare_tiled made readable as they were. */
#define GEM_MAPGRID_PATH 1
#define GEM_MAPGRID_GOAL 2
#define GEM_MAPGRID_STOP_ON_FAILURE 1   /* d == OB answers -3, d == UN answers -2 */
#define GEM_MAPGRID_SUM             2   /* the sum of the poses' distances instead of the last pose's */
#define GEM_MAPGRID_MAX_POINTS (1 << 20)
#define GEM_MAPGRID_MAX_WORDS  4096
int  gem_mapgrid_adjust_plan(const double* plan_xy, long long n, double resolution, double* out_xy, long long cap, long long* out_n);
int  gem_costmap_mapgrid_prepare(gem_handle* h, int id, const double* plan_xy, long long n, int which);
int  gem_costmap_mapgrid_read(gem_handle* h, int id, int which_one, int* out, int* out_started, int out_goal_cell[2]);
int  gem_costmap_mapgrid_score(gem_handle* h, int id, int which_one, const gem_footprint_pose* poses, long long n_traj, int poses_per_traj,
                               double xshift, int flags, long long* out_traj);
int  gem_costmap_mapgrid_score_device(gem_handle* h, int id, int which_one, const gem_footprint_pose* d_poses, long long n_traj,
                                      int poses_per_traj, double xshift, int flags, long long* d_out_traj);
