/* gem_hip_critics.h -- the best trajectory on the device costmap: the part of the C ABI of libgem_hip.so that scores a batch of
 * trajectories against an ordered list of critics, combines the scores as base_local_planner's SimpleScoredSamplingPlanner does and
 * leaves the winner on the device; and the third distance grid (FRONT) that DWA's goal_front critic reads.  Included by gem_hip.h, not
 * on its own.  Symbols only added: GEM_ABI_VERSION is unchanged.
 *
 * Every device entry takes the handle's lock and runs on the handle's stream.  A cycle is
 *     reset_window(master) -> mark -> clear_footprint -> merge -> inflate -> mapgrid_prepare (+ _prepare_front) -> best_trajectory,
 * and the first host wait is the one for the 32-byte answer.
 *
 * The contract is RESTATED from ROS noetic base_local_planner: src/simple_scored_sampling_planner.cpp (scoreTrajectory,
 * findBestTrajectory), src/obstacle_cost_function.cpp (scoreTrajectory, footprintCost), src/map_grid_cost_function.cpp
 * (scoreTrajectory) and the critic order dwa_local_planner's DWAPlanner builds (tests/critics_ref.py is the same statement in numpy /
 * plain Python).  UNVERIFIED: it is NOT verified against the library (there is none here; tools/ros_selfcheck.cpp's `critics` row
 * settles the combination and the winner in a ROS workspace).
 *   the FRONT grid   DWA's goal_front_costs_ reads the goal-mode grid of front_global_plan, the plan with its last point pushed
 *                forward.  gem_costmap_mapgrid_prepare_front is exactly gem_costmap_mapgrid_prepare(..., GEM_MAPGRID_GOAL) on the plan
 *                it is given, written into a third slot of the costmap: adjusted plan, run, single source, fill, one workgroup,
 *                generation number and error cases are the same, and the PATH and GOAL grids are not touched.  Moving the last
 *                point (x += forward_point_distance * cos(atan2(dy, dx)), y likewise) stays with the caller: it needs atan2 and is
 *                three lines of host code.  gem_costmap_mapgrid_read_front waits, as gem_costmap_mapgrid_read does.  The existing
 *                calls still know two grids: their which / which_one = 4 stays GEM_ERR_INVALID.
 *                gem_costmap_mapgrid_prepare_front_tiled (gem_hip_mapgrid_tiled.h) is to it what gem_costmap_mapgrid_prepare_tiled is to
 *                gem_costmap_mapgrid_prepare: the same grid in the same slot on a costmap of any size, and the call WAITS.
 *   a critic     {kind, grid, flags, column, scale, xshift}.  Its score for trajectory t is an exact integer converted to double,
 *                or the caller's double:
 *       GEM_CRITIC_OBSTACLE   the trajectory cost of gem_costmap_score_trajectories with the same spec and the flags
 *                GEM_FOOTPRINT_INSCRIBED_LETHAL | GEM_FOOTPRINT_SUM: the first negative pose result in pose order, else the maximum,
 *                or the sum.  With GEM_CRITIC_CENTRE_COST a non-negative pose result r becomes max(r, the byte of the centre's
 *                cell) first: the occ_cost of ObstacleCostFunction::footprintCost.  The library answers -6 / -7 where this gives
 *                -1 / -2 / -3: only the SIGN is the library's.  The footprint scaling factor is not modelled (noetic computes it
 *                and does not use it).  At most one OBSTACLE critic in a list: there is one spec.
 *       GEM_CRITIC_MAPGRID    exactly gem_costmap_mapgrid_score on the grid GEM_CRITIC_GRID_PATH / _GOAL / _FRONT with this xshift and
 *                the flags GEM_MAPGRID_STOP_ON_FAILURE | GEM_MAPGRID_SUM.  yshift and Product stay unprovided, as there.
 *       GEM_CRITIC_EXTERNAL   ext[column * n_traj + t]: the caller's raw score.  This is how the critics that read velocities only
 *                enter at their place in the order (oscillation first, twirling last, prefer-forward).  A negative value rejects.
 *                (gem_hip_trajgen.h generates the trajectories and these two columns on the device: gem_costmap_dwa_best.)
 *                Fields a kind does not read (grid, column, xshift) are ignored; its flags are checked.
 *   combination  for trajectory t, every operation in double and rounded on its own:
 *                    total = 0.0
 *                    for k in order:
 *                        if scale_k == 0: continue
 *                        s = score_k(t)
 *                        if s < 0: total = s; stop
 *                        if s != 0: s = s * scale_k
 *                        total = total + s
 *                t is VALID iff total >= 0; a NaN from an external column is never valid.  A scale that is negative or not finite
 *                is refused.  The library's early exit against the best cost so far (`if (best_traj_cost > 0 && traj_cost >
 *                best_traj_cost) break`) is NOT modelled and need not be: with scales >= 0 every term is >= 0, so the partial sums
 *                never decrease; a trajectory the exit cuts short already costs more than the best so far and could not have won
 *                with its full sum either, and a rejection found behind the cut only makes it lose in another way.
 *                (tests/test_critics_cpu.py runs both forms.)  out_total of a trajectory the library would have cut short is the
 *                full sum.
 *   lengths      traj_len (may be NULL: every trajectory has poses_per_traj poses) holds one int per trajectory, host or device like
 *                the poses.  Trajectory t owns the slots [t * T, (t + 1) * T), T = poses_per_traj, and uses the first traj_len[t] of
 *                them (DWA's num_steps differs per sample); "last" is pose traj_len[t] - 1.  A length outside [1, T] cannot be
 *                refused in device memory: it rejects the trajectory with total = -5.0 before any critic runs.  The host form
 *                refuses it as GEM_ERR_INVALID.
 *   the winner   the smallest total among the valid trajectories, ties to the SMALLEST INDEX (findBestTrajectory's strict < in
 *                generation order).  gem_best_trajectory {index, n_valid, cost, reserved = 0}: index = -1 and cost = -1.0 without a
 *                valid trajectory; n_valid is always set.  n_traj = 0 is valid input and answers the same.
 *
 *   gem_costmap_best_trajectory   critics, spec_xy: host memory.  poses [n_traj * poses_per_traj], traj_len [n_traj] or NULL,
 *                ext [n_ext_columns * n_traj] or NULL with n_ext_columns = 0, out_total [n_traj] or NULL, out_best: host arrays; the
 *                call waits.  _device: these five in device memory; the call only ENQUEUES two launches (the critics of every
 *                trajectory with one candidate per workgroup, then one workgroup that picks) and the buffers are untouched until
 *                gem_synchronize, as for gem_costmap_score_trajectories_device.  spec_xy is read by an OBSTACLE critic only.
 *                Scratch comes from the handle's arenas, which only grow: a second identical call allocates nothing.
 *   gem_critics_select   host only, no handle and no device: the combination and the winner over scores the caller already holds,
 *                scores[k * n_traj + t] = score_k(t); kind, grid, flags and column are not read.  out_total may be NULL.
 *
 * GEM_ERR_INVALID, nothing enqueued and nothing written: a bad id; a handle with a communicator; a NULL critics or out_best; a NULL
 * array with a non-zero count; n_traj < 0, n_traj * poses_per_traj above 2^31 - 2, poses_per_traj outside [1, 2^20]; n_critics outside
 * [1, GEM_CRITIC_MAX]; an unknown kind; a scale negative or not finite; unknown flag bits for the kind; more than one OBSTACLE critic;
 * with an OBSTACLE critic n_vertices out of range or a non-finite spec coordinate; a MAPGRID critic whose grid is not exactly one of
 * the three, whose xshift is not finite, or whose grid was never prepared or was prepared before the costmap last rolled or was observed (a critic with
 * scale 0 is checked like any other); n_ext_columns < 0 or an EXTERNAL column outside [0, n_ext_columns); in the host form a length
 * outside [1, poses_per_traj].  For the FRONT entries: the cases of gem_costmap_mapgrid_prepare / _read. */
#define GEM_CRITIC_OBSTACLE 1   /* flags: GEM_FOOTPRINT_INSCRIBED_LETHAL | GEM_FOOTPRINT_SUM | GEM_CRITIC_CENTRE_COST */
#define GEM_CRITIC_MAPGRID  2   /* grid: GEM_CRITIC_GRID_PATH | _GOAL | _FRONT; xshift; flags: GEM_MAPGRID_STOP_ON_FAILURE | GEM_MAPGRID_SUM */
#define GEM_CRITIC_EXTERNAL 3   /* column `column` of the caller's ext array */
#define GEM_CRITIC_MAX 8
#define GEM_CRITIC_GRID_PATH  1   /* = GEM_MAPGRID_PATH */
#define GEM_CRITIC_GRID_GOAL  2   /* = GEM_MAPGRID_GOAL */
#define GEM_CRITIC_GRID_FRONT 4
#define GEM_CRITIC_CENTRE_COST 4  /* OBSTACLE: a pose's cost is at least the byte of its centre cell */
typedef struct gem_critic { int kind, grid, flags, column; double scale, xshift; } gem_critic;              /* 32 bytes */
typedef struct gem_best_trajectory { long long index, n_valid; double cost; long long reserved; } gem_best_trajectory;  /* 32 bytes */
int  gem_costmap_mapgrid_prepare_front(gem_handle* h, int id, const double* plan_xy, long long n);
int  gem_costmap_mapgrid_read_front(gem_handle* h, int id, int* out, int* out_started, int out_goal_cell[2]);
int  gem_costmap_best_trajectory(gem_handle* h, int id, const gem_critic* critics, int n_critics, const gem_footprint_pose* poses,
                                 const int* traj_len, long long n_traj, int poses_per_traj, const double* spec_xy, int n_vertices,
                                 const double* ext, int n_ext_columns, double* out_total, gem_best_trajectory* out_best);
int  gem_costmap_best_trajectory_device(gem_handle* h, int id, const gem_critic* critics, int n_critics, const gem_footprint_pose* d_poses,
                                        const int* d_traj_len, long long n_traj, int poses_per_traj, const double* spec_xy, int n_vertices,
                                        const double* d_ext, int n_ext_columns, double* d_out_total, gem_best_trajectory* d_out_best);
int  gem_critics_select(const gem_critic* critics, int n_critics, const double* scores, long long n_traj, double* out_total,
                        gem_best_trajectory* out_best);
