/* gem_hip_trajgen.h -- DWA's sampled trajectories on the device: the part of the C ABI of libgem_hip.so that restates
 * base_local_planner's SimpleTrajectoryGenerator and its two velocity-only critics, so that a local-planner cycle uploads a few hundred
 * bytes of velocity lists instead of the poses, and everything between the sensor data and the chosen velocity command stays on the
 * GPU.  Included by gem_hip.h, not on its own.  Symbols only added: GEM_ABI_VERSION is unchanged.
 *
 * A cycle is  reset_window(master) -> mark -> clear_footprint -> merge -> inflate -> mapgrid_prepare (+ _prepare_front) -> dwa_best,
 * and the first host wait is the one for the 32-byte answer; gem_trajgen_velocity turns its index into the command on the host.
 *
 * The contract is RESTATED from ROS noetic base_local_planner: src/simple_trajectory_generator.cpp, include/.../velocity_iterator.h,
 * src/oscillation_cost_function.cpp, src/twirling_cost_function.cpp (tests/trajgen_ref.py is the same statement in numpy / plain
 * Python).  UNVERIFIED: it is NOT verified against the library (there is none here; tools/ros_selfcheck.cpp's `trajgen` row settles it
 * in a ROS workspace -- first of all which cos overload the library's unqualified cos(pos[2]) picks for a float: this contract
 * promotes to double).
 *   state        the library keeps pos, vel, the samples and the acceleration limits in Eigen::Vector3f: state is float32.  An
 *                expression that mixes in a double parameter is evaluated in double and rounded to float32 on assignment, every
 *                operation rounded on its own.  acc_lim_* are rounded to float32 on entry (they enter a Vector3f).
 *   the window   (initialise) shown for x; y and theta alike with max_vel_th = max_vel_theta, min_vel_th = -max_vel_theta.  With
 *                use_dwa:  max_vel[0] = (float)min(max_vel_x, vel[0] + acc[0] * sim_period),
 *                          min_vel[0] = (float)max(min_vel_x, vel[0] - acc[0] * sim_period).
 *                Without:  dist = sqrt(dx * dx + dy * dy) in double over the float differences goal - pos; max_vel_x =
 *                max(min(max_vel_x, dist / sim_time), min_vel_x), the same for y; then the two formulas with sim_time in place of
 *                sim_period.  DEVIATION: the library calls hypot here and for vmag below; the double sqrt(x * x + y * y) is this
 *                contract's definition.  vsamples[0] * vsamples[1] * vsamples[2] <= 0: no samples (n_traj = 0, a valid plan).
 *   the lists    VelocityIterator(min, max, n) in double: min == max gives the single value min; otherwise n = max(2, n),
 *                step = (max - min) / (double)max(1, n - 1), next = min; for j < n - 1: current = next, next += step, push current,
 *                and if current < 0 && next > 0 also push 0.0; finally push max.  A value becomes float32 when it enters a sample.
 *                The samples are the product, x outermost and theta innermost: sample t = (ix * n_y + iy) * n_th + ith.
 *   a trajectory (generateTrajectory) for the sample s: vmag = sqrt(s0 * s0 + s1 * s1), eps = 1e-4.  NOT GENERATED when
 *                (min_vel_trans >= 0 && vmag + eps < min_vel_trans) && (min_vel_theta >= 0 && fabs(s2) + eps < min_vel_theta), or when
 *                max_vel_trans >= 0 && vmag - eps > max_vel_trans.  num_steps = ceil(sim_time / sim_granularity) with
 *                discretize_by_time, else ceil(max(vmag * sim_time / sim_granularity, fabs(s2) * sim_time / angular_sim_granularity));
 *                zero steps: not generated.  dt = sim_time / num_steps.  With continued_acceleration (the library sets it to
 *                !use_dwa; here it is the caller's flag) loop_vel = computeNewVelocities(s, vel, acc, dt) and that is the
 *                trajectory's (xv, yv, thetav); otherwise loop_vel = s.  For i < num_steps: record the pose (pos0, pos1, pos2); with
 *                continued acceleration loop_vel = computeNewVelocities(s, loop_vel, acc, dt); then, all three right-hand sides
 *                read from the old pos,
 *                    pos0 = (float)(pos0 + (v0 * cos(pos2) + v1 * cos(M_PI_2 + pos2)) * dt)
 *                    pos1 = (float)(pos1 + (v0 * sin(pos2) + v1 * sin(M_PI_2 + pos2)) * dt)
 *                    pos2 = (float)(pos2 + v2 * dt).
 *                computeNewVelocities per component: vel_i < target_i ? (float)min((double)target_i, vel_i + acc_i * dt)
 *                                                                     : (float)max((double)target_i, vel_i - acc_i * dt).
 *                (xv, yv, thetav) of a sample that is not generated is the sample itself.
 *   sin and cos  are part of the contract (the kernels of this library hold no transcendental, so that a result does not depend on
 *                whose cos it was): plain double + - * in the form of gem_amd/csrc/gem_sincos.hpp, k = (t * INV + 1.5 * 2^52) -
 *                1.5 * 2^52, r = ((t - k * P1) - k * P2) - k * P3, Taylor polynomials of degree 17 / 16 by Horner, the quadrant
 *                (long long)k & 3.  Within 2^-53 of libm on the angles tried up to 64 pi.  |pos2| <= 64 pi is required throughout a
 *                trajectory: the host checks |pos[2]| + sim_time * (the largest |theta velocity| of the lists and of vel) <= 64 pi - 2.
 *   a pose       {(double)pos0, (double)pos1, cos((double)pos2), sin((double)pos2)}: a gem_footprint_pose.
 *   the critics  oscillation: -5.0 if a bit of config.oscillation_flags fires against (xv, yv, thetav), else 0.0 --
 *                FORWARD_POS_ONLY & xv < 0, FORWARD_NEG_ONLY & xv > 0, STRAFE_POS_ONLY & yv < 0, STRAFE_NEG_ONLY & yv > 0,
 *                ROT_POS_ONLY & thetav < 0, ROT_NEG_ONLY & thetav > 0.  Updating the flags from the chosen command stays with the
 *                caller.  twirling: fabs(thetav).  They are the external columns 0 and 1.
 *
 *   gem_trajgen_plan     host only, no handle: the window and the three lists (samples: x at 0, y at n_x, theta at n_x + n_y), n_traj =
 *                n_x * n_y * n_th, and max_steps, the largest num_steps any sample can take (ceil and the maxima are monotone: the
 *                lists' extremes decide it).  The plan carries the limits and the configuration: it is all the other calls need.
 *   gem_trajgen_generate host only, the twin of the kernel: poses [n_traj * poses_per_traj], traj_len [n_traj], ext [2 * n_traj],
 *                out_vel [3 * n_traj] or NULL.  Slot t is the sample index.  A sample that is not generated gets traj_len[t] = 0, its
 *                pose slots and the slots past traj_len[t] are left untouched, its two external scores and velocity are still written.
 *   gem_trajgen_velocity host only: (xv, yv, thetav) of sample `index`: the winner's command, so that a cycle reads back 32 bytes.
 *   gem_trajgen_sincos   host only: the contract's sine and cosine of n angles, as the kernel and the twin evaluate them.
 *   gem_trajgen_generate_device   the same into device memory; it only ENQUEUES one launch on the handle's stream.  pos, vel and the
 *                plan are host memory and travel in the kernel arguments.  gem_costmap_best_trajectory_device turns length 0 into the
 *                total -5.0 before any critic, so the library's "skip what was not generated" and "ties to the first generated"
 *                come out unchanged.
 *   gem_costmap_dwa_best / _device   generation into arenas of the handle that only grow, then the critics and the pick of
 *                gem_costmap_best_trajectory_device on them: one call, three launches, 32 bytes back.  An EXTERNAL critic's column
 *                0 / 1 is the generated oscillation / twirling column.  out_total [n_traj] (may be NULL) and out_best are host memory
 *                and the call waits; _device: device memory, only enqueued.  A second identical call allocates nothing.  A
 *                MAPGRID critic's grid passes gem_costmap_best_trajectory's test (gem_hip_critics.h): never prepared, or prepared
 *                before the costmap last rolled or was observed, is refused.
 *
 * GEM_ERR_INVALID, nothing enqueued and nothing written: a NULL argument other than those that may be; a parameter, pos, vel or goal
 * that is not finite; sim_time, sim_period, sim_granularity or (without discretize_by_time) angular_sim_granularity <= 0; unknown
 * oscillation bits; a list count above GEM_TRAJGEN_MAX_LIST in sum (the lists travel in the kernel arguments); a plan that
 * gem_trajgen_plan did not make; poses_per_traj outside [1, 2^20] or below the plan's max_steps; more than 2^31 - 2 pose slots; the
 * 64 pi bound; an index outside [0, n_traj); a handle with a communicator; for dwa_best the cases of gem_costmap_best_trajectory
 * with n_ext_columns = 2. */
#define GEM_TRAJGEN_MAX_LIST 256
#define GEM_OSC_FORWARD_POS_ONLY 1
#define GEM_OSC_FORWARD_NEG_ONLY 2
#define GEM_OSC_STRAFE_POS_ONLY  4
#define GEM_OSC_STRAFE_NEG_ONLY  8
#define GEM_OSC_ROT_POS_ONLY     16
#define GEM_OSC_ROT_NEG_ONLY     32
typedef struct gem_trajgen_limits {           /* 88 bytes */
    double max_vel_x, min_vel_x, max_vel_y, min_vel_y, max_vel_theta, min_vel_theta, max_vel_trans, min_vel_trans;
    double acc_lim_x, acc_lim_y, acc_lim_theta;
} gem_trajgen_limits;
typedef struct gem_trajgen_config {           /* 64 bytes */
    double sim_time, sim_granularity, angular_sim_granularity, sim_period;
    int use_dwa, discretize_by_time, continued_acceleration, oscillation_flags;
    int vsamples[3], reserved;
} gem_trajgen_config;
typedef struct gem_dwa_plan {                 /* 1200 bytes */
    gem_trajgen_limits limits;
    gem_trajgen_config config;
    int n_x, n_y, n_th, max_steps;
    long long n_traj;
    float samples[GEM_TRAJGEN_MAX_LIST];
} gem_dwa_plan;
int  gem_trajgen_plan(const gem_trajgen_limits* limits, const gem_trajgen_config* config, const float pos[3], const float vel[3],
                      const float goal[2], gem_dwa_plan* out);
int  gem_trajgen_generate(const gem_dwa_plan* plan, const float pos[3], const float vel[3], gem_footprint_pose* poses, int* traj_len,
                          double* ext, float* out_vel, int poses_per_traj);
int  gem_trajgen_velocity(const gem_dwa_plan* plan, const float vel[3], long long index, float out_vel[3]);
int  gem_trajgen_sincos(const double* angles, long long n, double* out_sin, double* out_cos);
int  gem_trajgen_generate_device(gem_handle* h, const gem_dwa_plan* plan, const float pos[3], const float vel[3],
                                 gem_footprint_pose* d_poses, int* d_traj_len, double* d_ext, float* d_vel, int poses_per_traj);
int  gem_costmap_dwa_best(gem_handle* h, int id, const gem_critic* critics, int n_critics, const gem_dwa_plan* plan, const float pos[3],
                          const float vel[3], int poses_per_traj, const double* spec_xy, int n_vertices, double* out_total,
                          gem_best_trajectory* out_best);
int  gem_costmap_dwa_best_device(gem_handle* h, int id, const gem_critic* critics, int n_critics, const gem_dwa_plan* plan,
                                 const float pos[3], const float vel[3], int poses_per_traj, const double* spec_xy, int n_vertices,
                                 double* d_out_total, gem_best_trajectory* d_out_best);
