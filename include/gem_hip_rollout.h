/* gem_hip_rollout.h -- trajectory rollout on the device costmap: the part of the C ABI of libgem_hip.so that restates
 * base_local_planner's TrajectoryPlanner::createTrajectories + generateTrajectory, the local planner move_base runs when no planner
 * is named (TrajectoryPlannerROS; the reference's layers/launch/create_globalmap.launch names none), so that a control cycle of that
 * configuration reads back 64 bytes instead of the local costmap and both distance grids.  Included by gem_hip.h, not on its own.
 * Symbols only added: GEM_ABI_VERSION is unchanged.
 *
 * A cycle is  ... -> inflate -> mapgrid_prepare(PATH | GOAL) -> rollout_best, and the first host wait is the one for the 64-byte answer.
 * Nothing in the costmap is written.
 *
 * The contract is RESTATED FROM MEMORY of ROS noetic base_local_planner/src/trajectory_planner.cpp and
 * include/base_local_planner/trajectory_inc.h (tests/rollout_ref.py is the same statement in plain Python, twice: the literal
 * createTrajectories with its two swapped trajectories and early returns, and evaluate-all-then-pick).  UNVERIFIED against the library:
 * there is none here; tools/ros_selfcheck.cpp's `rollout` row settles it in a ROS workspace.  The open points of that row:
 *   - the pairing of a negative vth_samp with stuck_left (and a positive one with stuck_right) in phase B;
 *   - `<=` in phases B / C against the strict `<` of phase A;
 *   - hypot in the window (below: this contract's definition is the sqrt form);
 *   - whether int(... + 0.5) of num_steps sees the double or a float.
 * All arithmetic is double, every operation rounded on its own (-ffp-contract=off); cells are ints.  min(a, b) is b < a ? b : a and
 * max(a, b) is a < b ? b : a, as std::min / std::max.
 *
 *   configuration   gem_rollout_config.  meter_scoring is the CALLER's multiplication of pdist_scale and gdist_scale by the costmap's
 *                resolution: the library does it once in its constructor, this contract takes the scales as they are used.  The
 *                state flags come from the caller as a mask (GEM_ROLLOUT_ESCAPING, _STUCK_LEFT, _STUCK_RIGHT, _STUCK_LEFT_STRAFE,
 *                _STUCK_RIGHT_STRAFE); UPDATING them from the answer stays with the caller, as the oscillation flags do for DWA: the
 *                rotating / strafing bookkeeping, prev_x_ / prev_y_, the escape pose and the two reset distances.
 *   the window   mx = max_vel_x; with final_goal_valid  mx = min(mx, sqrt(dx * dx + dy * dy) / sim_time) over (final_goal - pos).
 *                DEVIATION: the library calls hypot there; the double sqrt(dx * dx + dy * dy) is this contract's definition, as in
 *                gem_hip_trajgen.h.  T = dwa ? sim_period : sim_time;
 *                    max_x  = max(min(mx, vel0 + acc_lim_x * T), min_vel_x)      min_x  = max(min_vel_x, vel0 - acc_lim_x * T)
 *                    max_th = min(max_vel_th, vel2 + acc_lim_theta * T)          min_th = max(min_vel_th, vel2 - acc_lim_theta * T)
 *                    dvx = (max_x - min_x) / (vx_samples - 1)                    dvth = (max_th - min_th) / (vtheta_samples - 1)
 *                vx_samples < 2 or vtheta_samples < 2 is refused: the library divides by zero there.
 *   the candidates  in the library's call order, their values formed by its running additions (vx_samp += dvx), not by min + i * d:
 *                A (absent with ESCAPING)  vx_samp from min_x: for each of the vx_samples values first (vx_samp, 0, 0), then with
 *                  vth_samp restarted at min_th the vtheta_samples - 1 candidates (vx_samp, 0, vth_samp), vth_samp += dvth after
 *                  each; then vx_samp += dvx.  With holonomic_robot then (0.1, 0.1, 0) and (0.1, -0.1, 0).
 *                B  vtheta_samples in-place candidates, vth_samp from min_th by += dvth: the simulated value is
 *                  lim = vth_samp > 0 ? max(vth_samp, min_in_place_vel_th) : min(vth_samp, -min_in_place_vel_th), the candidate
 *                  (0, 0, lim).  It is ELIGIBLE iff vth_samp > dvth || vth_samp < -dvth, on the unlimited value, and its SIDE is the
 *                  sign of the unlimited value.
 *                C  with holonomic_robot: (0, y_vels[i], 0) for i < n_y_vels.
 *                D  (backup_vel, 0, 0).
 *                Candidate c of phase A is (i, j) = (c / vtheta_samples, c % vtheta_samples): j = 0 is the straight one, j >= 1 has
 *                vth list value j - 1.  The phases follow each other: gem_rollout_plan.off_b, off_c, off_d, n_cand = off_d + 1.
 *   a trajectory (generateTrajectory) for the candidate (sx, sy, sth) from pos, vel:
 *                vmag = sqrt(sx * sx + sy * sy);  num_steps = (int)(max(vmag * sim_time / sim_granularity, fabs(sth) /
 *                angular_sim_granularity) + 0.5) -- the angular term has no sim_time: that is the library's -- and 0 becomes 1;
 *                dt = sim_time / num_steps;  occ = path = goal = 0.  For each step i < num_steps, in this order:
 *                  1. worldToMap(x, y) fails: cost -1, stop.
 *                  2. f = footprintCost({x, y, cos th, sin th}, spec, flags) exactly as gem_hip_footprint.h states it, with the
 *                     caller's GEM_FOOTPRINT_INSCRIBED_LETHAL bit; f < 0: cost -1, stop.
 *                  3. occ = max(max(occ, f), the byte of the centre cell).
 *                  4. path = PATH[cell], goal = GOAL[cell]; with OB = size_x * size_y: OB <= goal || OB <= path: cost -2, stop.
 *                  5. the pose is recorded; the last one recorded is the END POSE.
 *                  6. v_k = (s_k - v_k >= 0) ? min(s_k, v_k + acc_k * dt) : max(s_k, v_k - acc_k * dt)  for x, y, theta.
 *                  7. with the NEW velocities and the OLD theta:  x += (vx * cos th + vy * cos(M_PI_2 + th)) * dt,
 *                     y += (vx * sin th + vy * sin(M_PI_2 + th)) * dt, then th += vth * dt.
 *                After all steps  cost = (pdist_scale * path + goal * gdist_scale) + occdist_scale * occ.  A scale that is negative
 *                (-0.0 included) or not finite is refused, so a legal cost is >= +0.0 and its bit pattern orders as an integer.
 *                Sine and cosine are the contract's of gem_hip_trajgen.h (gem_amd/csrc/gem_sincos.hpp), under the same bound, checked
 *                on the host: |pos[2]| + sim_time * (the largest |theta velocity| of the candidates and of vel) <= 64 pi - 2.
 *                `ahead` of a candidate with cost >= 0 and the end pose (xe, ye, the): worldToMap(xe + heading_lookahead * cos the,
 *                ye + heading_lookahead * sin the) gives a cell and ahead = GOAL[cell]; when it fails ahead is "none", written -1.
 *                A candidate with cost < 0 has ahead -1 too.
 *   the pick     the sequential loop it is.  best = none with cost -1; heading_dist unbounded.
 *                A  in order: take c iff cost_c >= 0 && (cost_c < best.cost || best.cost < 0).
 *                B  in order: consider c iff cost_c >= 0 && (cost_c <= best.cost || best.cost < 0 || best.yv != 0.0) and c is
 *                   eligible; then iff ahead_c exists and ahead_c < heading_dist: side negative and not STUCK_LEFT: take c and set
 *                   heading_dist = ahead_c; else side positive and not STUCK_RIGHT: the same.  best.cost moves inside the loop.
 *                   If best.cost >= 0 here: stage 1, done.
 *                C  in order: consider c iff cost_c >= 0 && (cost_c <= best.cost || best.cost < 0); the same ahead test against the
 *                   same heading_dist; vy > 0 and not STUCK_LEFT_STRAFE, else vy < 0 and not STUCK_RIGHT_STRAFE.  If best.cost >= 0:
 *                   stage 2.
 *                D  the backward candidate wins whatever its cost: stage 3.  raw_cost is its cost as generated (the caller's escape
 *                   rule needs raw_cost > -2); cost = 1.0 when raw_cost is exactly -1.0, else raw_cost.
 *                In stages 1 and 2 raw_cost == cost.  (xv, yv, thetav) is the winner's simulated sample (lim in phase B).
 *   NOT PROVIDED  heading_scoring (it needs atan2 and lineCost per step: a call with it set cannot be made, the config has no such
 *                field); simple_attractor; the flag bookkeeping above; checkTrajectory / scoreTrajectory of a single command;
 *                TrajectoryPlannerROS's stop-and-rotate controller.  navfn's potential is not offered either.
 *
 *   gem_rollout_plan   host only, no handle: the window, the two lists the candidates are decoded from (vx at 0, vth at n_vx),
 *                n_cand, the phase offsets and max_steps, the largest num_steps of any candidate.  The plan is POD and travels in the
 *                kernel arguments: vx_samples + vtheta_samples <= GEM_ROLLOUT_MAX_LIST.  It is made FOR a state and a mask (it keeps
 *                the mask: state_flags): every call makes it again from its own arguments and refuses a plan that differs in a byte.
 *   gem_rollout_host   host only: the twin of the kernels over caller-held arrays -- the bytes and the PATH and GOAL grids, row-major
 *                [size_y * size_x].  out_cost [n_cand], out_ahead [n_cand], out_steps [n_cand] = the poses RECORDED (num_steps of a
 *                candidate that ran to its end, the failing step's index otherwise), out_poses [n_cand * max_steps] or NULL (slots
 *                past out_steps are left untouched), out_best.  The state flags are the plan's.  It shares its arithmetic with the
 *                kernel (gem_amd/csrc/gem_rollout.hpp).
 *   gem_rollout_pick   host only: the pick alone over cost [n_cand] and ahead [n_cand].  Its ESCAPING bit must be the plan's (it decides
 *                the candidates); the four stuck bits are the argument's, so one set of costs answers every stuck state.
 *   gem_costmap_rollout_best   the candidates and the pick on the device costmap `id`, two launches.  out_cost and out_ahead (either
 *                may be NULL) and out_best are host memory and the call waits.  _device: device memory, and it only ENQUEUES.  Scratch
 *                comes from arenas of the handle that only grow: a second identical call allocates nothing.
 *
 * GEM_ERR_INVALID, nothing enqueued and nothing written: a NULL argument other than those that may be; a parameter, pos or vel that
 * is not finite; sim_time, sim_granularity, angular_sim_granularity, or with dwa sim_period, <= 0; vx_samples < 2 or
 * vtheta_samples < 2; a list sum above GEM_ROLLOUT_MAX_LIST; a negative (or -0.0) or non-finite scale; n_y_vels outside
 * 0 .. GEM_ROLLOUT_MAX_Y_VELS, or a zero among the y_vels in use; unknown state or footprint flag bits (only
 * GEM_FOOTPRINT_INSCRIBED_LETHAL is known here); a plan gem_rollout_plan did not make for these pos, vel and flags; max_steps above
 * GEM_ROLLOUT_MAX_STEPS; the 64 pi bound; n_vertices out of range or a non-finite spec coordinate; a handle with a communicator, or a
 * bad id; a PATH or GOAL grid never prepared, or prepared before the costmap last rolled or was observed. */
#define GEM_ROLLOUT_MAX_Y_VELS 8
#define GEM_ROLLOUT_MAX_LIST   256
#define GEM_ROLLOUT_MAX_STEPS  4096
#define GEM_ROLLOUT_ESCAPING           1
#define GEM_ROLLOUT_STUCK_LEFT         2
#define GEM_ROLLOUT_STUCK_RIGHT        4
#define GEM_ROLLOUT_STUCK_LEFT_STRAFE  8
#define GEM_ROLLOUT_STUCK_RIGHT_STRAFE 16
typedef struct gem_rollout_config {           /* 240 bytes */
    double sim_time, sim_granularity, angular_sim_granularity, sim_period, pdist_scale, gdist_scale, occdist_scale, heading_lookahead;
    double max_vel_x, min_vel_x, max_vel_th, min_vel_th, min_in_place_vel_th, backup_vel, acc_lim_x, acc_lim_y, acc_lim_theta;
    double final_goal_x, final_goal_y;
    int vx_samples, vtheta_samples, dwa, holonomic_robot, final_goal_valid, n_y_vels;
    double y_vels[GEM_ROLLOUT_MAX_Y_VELS];
} gem_rollout_config;
/* The plan shares its name with the call that makes it, so it has a tag and no typedef: write `struct gem_rollout_plan` (C keeps tags
 * apart from functions; in C++ the function hides the class name and the elaborated form still names the class). */
struct gem_rollout_plan {                     /* 2368 bytes */
    gem_rollout_config config;
    double max_x, min_x, max_th, min_th, dvx, dvth;
    int n_vx, n_vth, state_flags, max_steps;
    int off_b, off_c, off_d, n_cand;
    double lists[GEM_ROLLOUT_MAX_LIST];
};
typedef struct gem_rollout_best {             /* 64 bytes */
    long long index;                          /* the winner's candidate index */
    int stage, reserved;                      /* 1 | 2 | 3 */
    double cost, raw_cost, xv, yv, thetav;
    long long reserved1;                      /* 0: the fields above are 56 bytes, the record is 64 */
} gem_rollout_best;
int  gem_rollout_plan(const gem_rollout_config* config, const double pos[3], const double vel[3], int state_flags, struct gem_rollout_plan* out);
int  gem_rollout_host(const struct gem_rollout_plan* plan, const double pos[3], const double vel[3], const gem_costmap_config* geometry,
                      const unsigned char* bytes, const int* path, const int* goal, const double* spec_xy, int n_vertices, int flags,
                      double* out_cost, int* out_ahead, int* out_steps, gem_footprint_pose* out_poses, gem_rollout_best* out_best);
int  gem_rollout_pick(const struct gem_rollout_plan* plan, int state_flags, const double* cost, const int* ahead, gem_rollout_best* out_best);
int  gem_costmap_rollout_best(gem_handle* h, int id, const struct gem_rollout_plan* plan, const double pos[3], const double vel[3], int state_flags,
                              const double* spec_xy, int n_vertices, int flags, double* out_cost, int* out_ahead, gem_rollout_best* out_best);
int  gem_costmap_rollout_best_device(gem_handle* h, int id, const struct gem_rollout_plan* plan, const double pos[3], const double vel[3],
                                     int state_flags, const double* spec_xy, int n_vertices, int flags, double* d_out_cost, int* d_out_ahead,
                                     gem_rollout_best* d_out_best);
