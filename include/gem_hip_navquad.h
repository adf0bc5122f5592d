/* gem_hip_navquad.h -- the QUADRATIC potential on the device costmap: the part of the C ABI of libgem_hip.so that computes a
 * two-axis (Eikonal-like) potential where gem_hip_navplan.h computes the Manhattan-like min4 + w.  Included by gem_hip.h, not on its
 * own.  Symbols only added: GEM_ABI_VERSION is unchanged.
 *
 * Why.  The gradient walk of gem_hip_navpath.h (global_planner's default path) cycles on the linear potential of rough maps; the
 * quadratic update is global_planner's default (use_quadratic) and what navfn computes.  gem_hip_navplan.h left it out because the
 * library's float result depends on the visiting order of its priority buffers and its polynomial is not monotone.  Stated in exact
 * integers and clamped at hf the update IS monotone, and the potential below is order-free.  It is THE PROJECT'S OWN CONTRACT, not a
 * bit-copy of any library; tests/navquad_ref.py is the same statement in numpy / plain Python, twice.
 *
 *   inputs       weights w[256] by cost byte (0 = impassable), cells, GEM_NAV_OUTLINE, the source rule (the start cell has potential 0
 *                whatever its byte and wherever it lies), the overflow refusal and GEM_NAV_UNREACHED are exactly those of
 *                gem_hip_navplan.h.  In addition max(w) > 462 is refused (GEM_ERR_INVALID): 10046 * 462^2 < 2^31, so the numerator
 *                below fits 31 bits and no 64-bit arithmetic is needed.  gem_navplan_weights' defaults are <= 252.
 *   minima       for a traversable non-source cell n with hf = w[byte[n]]: h = the minimum of the left and right neighbours'
 *                potentials, v = that of the up and down neighbours'; a neighbour off the map, impassable or unreached counts as
 *                UNREACHED.  ta = min(h, v), tc = max(h, v).  ta UNREACHED: the cell is unreached.  Otherwise dc = hf if tc is
 *                UNREACHED, else dc = min(tc - ta, hf).
 *   increment    inc(hf, dc) = hf                                                                              if dc >= hf
 *                            = max(1, min(hf, floor((-2301 dc^2 + 5307 dc hf + 7040 hf^2) / (10000 hf))))      otherwise
 *                with mathematical integer floor division; the numerator is never negative (dc < hf).
 *   potential    T(n) = ta + inc.  The potential is the GREATEST fixed point of pot[n] = T(n) with pot[start] = 0; every impassable
 *                or unreachable cell is GEM_NAV_UNREACHED.  int32 in the units of w, like the linear one, and nowhere above it, with
 *                the same reached set (inc <= hf).
 *   path, status, world points: GridPath::getPath on that potential and the status of gem_hip_navplan.h, unchanged.
 *
 * Why the fixed point is unique and order-free.  Write f(dc) = inc(hf, dc).  f is non-decreasing with f(dc + 1) - f(dc) <= 1
 * (the polynomial's slope in dc is (5307 hf - 4602 dc) / (10000 hf) in (0.07, 0.54) on [0, hf), the floor of a function of slope
 * below 1 steps by at most 1, the clamp to 1 .. hf keeps both, and the last step, to f(hf) = hf, is from the polynomial's 1.0046 hf
 * floored and clamped: 0 or 1; tests/test_navquad_cpu.py checks every step of every hf in 1 .. 462).  So T = ta + f(min(tc - ta,
 * hf)) is non-decreasing in tc, and in ta too: raising ta by 1 lowers dc by at most 1 and f by at most 1.  T is therefore MONOTONE in each neighbour, and by Knaster-Tarski the fixed points above form a lattice with a greatest
 * element P*.  An iteration that starts from the top (UNREACHED everywhere, 0 at the start) and only ever replaces a cell by
 * min(old, T(current neighbours)) stays at or above P* (induction: T(values >= P*) >= T(P*) = P*), and it can only stop -- nothing
 * left to lower -- at a fixed point, which is at or below P* by definition: it stops AT P*, whatever order the cells were visited in,
 * however stale the neighbours a cell was computed from.  It does stop: the values are non-negative integers that only fall.  The
 * tests check it: Jacobi sweeps, three Gauss-Seidel orders, the host twin's heap and the device's tiles agree byte for byte.
 *
 * NAMED DEPARTURES from the library (global_planner's QuadraticCalculator, navfn's updateCell):
 *   - the coefficients -0.2301, 0.5307, 0.7040 are QuadraticCalculator's / navfn's, RECALLED FROM MEMORY and NOT VERIFIED against
 *     either (tools/ros_selfcheck.cpp's `navquad` row settles it in a ROS workspace);
 *   - min(hf, .) removes the library's jump for dc / hf in (0.9448, 1), where its polynomial exceeds hf by at most 0.46 % of hf and
 *     then drops to hf at dc = hf;
 *   - the floor loses under one unit per cell (the library's potential is a float);
 *   - max(1, .) keeps a cell strictly above its lowest 4-neighbour when w < 2: GridPath and gem_costmap_navplan_goal need a
 *     potential that strictly falls to terminate;
 *   - the result is converged EVERYWHERE.  The library stops pushing a neighbour that is not higher by INVSQRT2 * cost and exits at
 *     the goal: its float result depends on the visiting order, and no parallel form can equal it (gem_hip_navplan.h says so too).
 * On rough maps the gradient walk arrives more often on this potential than on the linear one, but NOT always: GEM_NAVPATH_CAP stays
 * possible (DESIGN.md section 7w has the counts).
 *
 *   gem_navquad_host   the host twin, no handle and no device: arguments, checks and status of gem_navplan_host, plus the weight
 *                limit.  Its potential is relaxed in an order unlike the kernel's (a binary heap keyed by potential, a lowered cell
 *                pushed again until nothing lowers), so their agreement is evidence of the order-free claim.
 *   gem_costmap_navplan_quadratic   arguments, waits, arenas, generation rule, error list and status of gem_costmap_navplan, plus
 *                the weight limit.  It leaves potential, path and status in the SAME slots as the linear plan: whichever plan ran last
 *                is the costmap's plan, and gem_costmap_navplan_read / _status / _navplan_goal, gem_costmap_navplan_paths* and
 *                gem_costmap_frontiers* work on it unchanged.  flags is 0 or GEM_NAV_OUTLINE.  The potential is relaxed tile by tile as
 *                the linear one is; a tile is allowed a fixed number of in-tile passes per round and goes on a round later when it
 *                needs more, so status.rounds is usually above the linear plan's. */
int  gem_navquad_host(const unsigned char* grid, int size_x, int size_y, const int* w, int flags, const int start_cell[2], const int goal_cell[2],
                      int* pot, int* path_cells, long long cap, gem_navplan_status* status);
int  gem_costmap_navplan_quadratic(gem_handle* h, int id, const double start_xy[2], const double goal_xy[2], const int* w, int flags, double* out_xy,
                                   long long cap, gem_navplan_status* st);
