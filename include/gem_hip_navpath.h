/* gem_hip_navpath.h -- paths on the last plan's potential, for a batch of goals: the part of the C ABI of libgem_hip.so that walks from up
 * to 1024 goals back to the start of the costmap's last gem_costmap_navplan in ONE launch, one wave per goal, either as the grid path of
 * gem_hip_navplan.h (GEM_NAVPATH_GRID) or as global_planner's default, the gradient path (GEM_NAVPATH_GRADIENT): sub-cell points half a
 * cell apart along the interpolated gradient of the potential.  Included by gem_hip.h, not on its own.  Symbols only added:
 * GEM_ABI_VERSION is unchanged.
 *
 * The calls READ the potential.  They leave it, the costmap's last path and status (gem_costmap_navplan_status / _read) and the
 * frontier search (gem_costmap_frontiers_read) untouched.
 *
 * The gradient walk is RESTATED FROM MEMORY from global_planner/src/gradient_path.cpp (ROS noetic: GradientPath::getPath, gradCell) and
 * is NOT VERIFIED against the library (there is none here).  tests/navpath_ref.py is the same statement in numpy scalar operations,
 * twice: once literally, with the library's linear index and its gradx_ / grady_ cache arrays, once as the pure function below; they
 * agree on every case, so the cache is inert (a cell's gradient is recomputed to the same value whenever it is asked for).  The walk
 * is a pure function of the potential, which is why it can be stated although the quadratic calculator cannot (gem_hip_navplan.h).
 * float is binary32, double is binary64, EVERY operation is rounded on its own (no fused multiply-add), sqrtf is correctly rounded.
 *
 *   inputs       pot: int32 potentials, size_y rows of size_x.  The plan's start cell (sx0, sy0).  A goal cell (gx, gy).  max_points.
 *                P(x, y) is pot on the map and GEM_NAV_UNREACHED off it.  "High" means == GEM_NAV_UNREACHED.
 *   G(x, y)      the gradient of a cell with cv = P(x, y) not high: gx_ = gy_ = 0.f; if P(x-1, y) is not high gx_ += (float)(P(x-1, y) -
 *                cv); if P(x+1, y) is not high gx_ += (float)(cv - P(x+1, y)); the same in y with y-1 and y+1.  n = sqrtf(gx_*gx_ +
 *                gy_*gy_); if n > 0: r = (float)(1.0 / (double)n) and G = (r*gx_, r*gy_), else G = (0, 0).
 *   L(t, a, b)   (float)((1.0 - (double)t) * (double)a + (double)(t * b)): the product t * b is a float product, everything else is in
 *                double -- what the C++ expression (1.0 - dx) * a + dx * b over floats evaluates to.
 *   the walk     c = (gx, gy), dx = dy = 0.f, the point list empty.  A goal off the map: GEM_NAVPATH_OFF_MAP.  A high P(goal):
 *                GEM_NAVPATH_UNREACHED.  Then loop:
 *                1. the list holds max_points: stop, GEM_NAVPATH_CAP.
 *                2. nx = (float)cx + dx, ny = (float)cy + dy (float adds).  If fabs((double)nx - sx0) < 0.5 and fabs((double)ny - sy0)
 *                   < 0.5: append ((float)sx0, (float)sy0) and stop, GEM_NAVPATH_FOUND.
 *                3. append (nx, ny).  osc: the list has more than 2 points and its last equals its third from last (float == on both).
 *                4. if any of the nine P(cx+i, cy+j), i, j in {-1, 0, 1}, is high, or osc: the fallback.  best = c, bp = P(c); scan
 *                   (i, j) in the order (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1) -- row-major, NOT the grid path's order --
 *                   and strict < on P moves best.  c = best, dx = dy = 0.f.  If P(c) is high: stop, GEM_NAVPATH_HIGH.
 *                5. otherwise the gradient step.  g00 = G(cx, cy), g10 = G(cx+1, cy), g01 = G(cx, cy+1), g11 = G(cx+1, cy+1);
 *                   x = L(dy, L(dx, g00.x, g10.x), L(dx, g01.x, g11.x)), y likewise (the inner L are floats).  x == 0 and y == 0:
 *                   stop, GEM_NAVPATH_ZERO_GRADIENT.  ss = 0.5f / sqrtf(x*x + y*y); dx += x*ss; dy += y*ss.  Then four independent
 *                   tests in this order: dx > 1: cx++, dx -= 1; dx < -1: cx--, dx += 1; dy > 1: cy++, dy -= 1; dy < -1: cy--, dy += 1.
 *   the cap      is the walk's termination (the library's is 4 * size_x * size_y iterations and an empty plan).  It is not decoration:
 *                the walk above has genuine cycles that the oscillation test does not catch (a period of three points was met on a
 *                40 x 40 map with noisy weights).  Every status other than FOUND leaves the points walked so far in place and n_points
 *                set.
 *   GRID form    the walk of gem_hip_navplan.h's grid path (nav_grid_path: its scan order, strict <), the visited cells written as
 *                ((float)x, (float)y); GEM_NAVPATH_CAP when the path is longer than max_points.  A cell without a neighbour on the map
 *                that is not the start (a 1 x 1 map) ends in GEM_NAVPATH_HIGH.  The loop is nav_grid_path's restated, not called: its
 *                bound is max_points where nav_grid_path's is the cell count, and it has the HIGH exit.  On a converged potential the
 *                two visit the same cells (the potential strictly falls); on a hand-made one they need not: an island goal steps onto
 *                unreached cells, as nav_grid_path would, and wanders until GEM_NAVPATH_CAP.
 *   order, units points are in WALK ORDER, goal first and start last, in CELL coordinates.  The facades reverse them and convert on the
 *                host in double: origin + ((double)p + 0.5) * resolution, the cell-centre convention of the grid path.
 *
 * Departures from the library and open points, named:
 *   - P is GEM_NAV_UNREACHED off the map.  The library has no column check and a row guard on the linear index only: it
 *     relies on the outline.
 *   - differences of potentials are taken in int32 and then converted; the library subtracts float potentials.  The two agree while
 *     potentials stay below 2^24.
 *   - open point 1: hypot(x, y) is sqrtf(x*x + y*y) here, as in gem_hip_trajgen.h.
 *   - the library's gradient of a HIGH cell (+- lethal_cost) is not built: it is dead in this walk, because every cell whose gradient
 *     is taken lies in a 3 x 3 block just tested to be free of high cells.
 *   - GEM_NAVPATH_HIGH cannot arise in the GRADIENT form as stated: the fallback starts from best = c and strict < never moves it to a
 *     high cell, so P(c) is not high behind it (the library's test is dead in the same way).  A reached goal whose every neighbour is
 *     high repeats its own point until the cap.  The status is kept for the test the library has and for the GRID form's use of it.
 *   - the slots of out_pts behind a goal's n_points are not defined (the waiting form copies its scratch; the device form leaves them).
 *   - convert_offset_ stays unmodelled, as in gem_hip_navplan.h; the orientation filter, default_tolerance, A*, the quadratic potential
 *     and navfn are not restated (gem_hip_navplan.h gives the reason for the last two).
 *
 *   gem_navpath_host   the host twin of one goal, no handle and no device.  start_cell and goal_cell are (x, y), on the map or not.
 *                out_pts (may be NULL) takes max_points pairs.
 *   gem_costmap_navplan_paths   n_goals world points (goals_xy, pairs) mapped by the worldToMap of gem_hip.h; a goal off the map is
 *                not a refusal, it is that goal's GEM_NAVPATH_OFF_MAP with goal_cell (-1, -1).  One launch on the handle's stream
 *                behind whatever was enqueued, one wave per goal.  out_pts (may be NULL) takes n_goals slots of max_points pairs, out
 *                n_goals results.  The call WAITS.  Scratch for the goal cells, the points and the results lives with the costmap in
 *                arenas that only grow: a second identical call allocates nothing.
 *   gem_costmap_navplan_paths_device   the same with d_out_pts (may be NULL) and d_out in device memory.  The call does not wait for
 *                the walk it enqueues, but it is NOT free of waits: the goal cells (8 bytes a goal) are uploaded on the handle's stream
 *                and the call returns when that copy has run, that is, behind everything enqueued on the stream before it -- an
 *                earlier _device walk included.  A stream of _device calls therefore serialises with the host.
 *
 * GEM_ERR_INVALID, nothing enqueued and nothing changed: a bad id; a handle with a communicator; NULL goals or results; non-finite goal
 * coordinates; n_goals outside 1 .. 1024; max_points outside 2 .. 2^20; n_goals * max_points above 2^24; an unknown form; size_x or
 * size_y of 2^24 or more; no plan, or a stale one, by the generation test of gem_costmap_navplan_read.  Host twin: a NULL pot, start,
 * goal or result, sizes below 1 or of 2^24 or more, max_points outside 2 .. 2^20, an unknown form. */
#define GEM_NAVPATH_GRID     0
#define GEM_NAVPATH_GRADIENT 1
enum { GEM_NAVPATH_FOUND = 1, GEM_NAVPATH_OFF_MAP, GEM_NAVPATH_UNREACHED, GEM_NAVPATH_HIGH, GEM_NAVPATH_ZERO_GRADIENT, GEM_NAVPATH_CAP };
typedef struct gem_navpath_result {    /* 32 bytes */
    int status;             /* GEM_NAVPATH_FOUND .. GEM_NAVPATH_CAP */
    int n_points;           /* points written for this goal (0: off the map or unreached) */
    int goal_cell[2];       /* (x, y); (-1, -1) off the map */
    int goal_potential;     /* GEM_NAV_UNREACHED off the map */
    int reserved[3];        /* 0 */
} gem_navpath_result;
int  gem_navpath_host(const int* pot, int size_x, int size_y, const int start_cell[2], const int goal_cell[2], int form, int max_points,
                      float* out_pts, gem_navpath_result* out);
int  gem_costmap_navplan_paths(gem_handle* h, int id, const double* goals_xy, int n_goals, int form, int max_points, float* out_pts,
                               gem_navpath_result* out);
int  gem_costmap_navplan_paths_device(gem_handle* h, int id, const double* goals_xy, int n_goals, int form, int max_points, float* d_out_pts,
                                      gem_navpath_result* d_out);
