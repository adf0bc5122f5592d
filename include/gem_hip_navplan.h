/* gem_hip_navplan.h -- the global plan on the device costmap: the part of the C ABI of libgem_hip.so that computes global_planner's
 * weighted potential over the cells of a costmap where it lies and walks the grid path from the goal back to the start.  Included
 * by gem_hip.h, not on its own.  Symbols only added: GEM_ABI_VERSION is unchanged.
 *
 * gem_costmap_navplan takes the handle's lock and runs on the handle's stream: marks, merges and inflation enqueued before it are
 * visible to it without a host wait.  It is the first costmap call that does not fit one workgroup (a global costmap is 1000 x 1000
 * cells): the potential is relaxed tile by tile in global memory, a launch per round, and the host waits for the plan.
 *
 * The contract is RESTATED FROM MEMORY from the navigation stack's global_planner package (GlobalPlanner::makePlan,
 * DijkstraExpansion, PotentialCalculator, GridPath, Expander::getCost) and is NOT VERIFIED against the library (there is none here;
 * tools/ros_selfcheck.cpp's `navplan` row settles it in a ROS workspace).  tests/navplan_ref.py is the same statement in numpy /
 * plain Python, twice.  Only ONE configuration is restated, the one whose answer does not depend on the order cells are visited in:
 *     use_dijkstra = true, use_quadratic = false (PotentialCalculator: min of the four neighbours + cost), use_grid_path = true.
 * Deliberately NOT restated:
 *   - navfn and the quadratic calculator AS THE LIBRARY COMPUTES THEM: their potential is a float whose value depends on the visiting
 *     order of the priority buffers, and the quadratic update jumps from 1.0046 * hf to hf at dc = hf, so it is not even monotone.
 *     No parallel form can be bit-equal to it.  The quadratic update stated in exact integers and clamped at hf IS monotone and
 *     order-free: that contract, the project's own, is gem_hip_navquad.h (gem_costmap_navplan_quadratic), beside this one.
 *   - the gradient path, A*, default_tolerance, the orientation filter, publishing the potential.
 *     (The gradient path is a pure function of the potential and is stated on its own, for a batch of goals: gem_hip_navpath.h.)
 *   - the library's early exit at the goal: the potential here is the converged one EVERYWHERE.
 *   - convert_offset_: the library's half-cell shift of start and goal is not modelled; both are world points mapped by the
 *     worldToMap of gem_hip.h (its refusal of non-finite input is turned into GEM_ERR_INVALID here).
 * Where the contract IS exact: everything is an integer.
 *   weights      the device sees w[256] of int32 indexed by the cost byte: 0 = impassable, > 0 = traversable.  gem_navplan_weights
 *                makes the table as Expander::getCost is recalled: for byte c, if c < lethal_cost - 1, or allow_unknown and c == 255,
 *                v = (float)c * cost_factor + neutral_cost in float32, each operation rounded on its own; v >= lethal_cost becomes
 *                lethal_cost - 1; every other byte is impassable.  Defaults 50, 3.0, 253, 1 (byte 252 is impassable under them).  A
 *                traversable v that is not a whole number, or not positive: GEM_ERR_INVALID -- the integer contract is the point; a
 *                caller with another cost model passes a table of its own, so the device contract does not rest on this recollection.
 *   cells        those of the costmap where it lies, geometry after rolling, size_y rows of size_x; the bytes are read when the call
 *                runs on the stream.  With GEM_NAV_OUTLINE (outline_map, the library's default) the outermost ring of cells counts as
 *                impassable; the costmap is NOT written (the library writes 254 into it).
 *   potential    the start cell is a source with potential 0 whatever its byte and wherever it lies (clearRobotCell without the
 *                write).  Every other cell n with w[byte[n]] > 0 gets the minimum, over 4-connected paths from the start whose cells
 *                after the start are all traversable, of the sum of w over those cells: the unique fixed point of
 *                pot[n] = min4(pot) + w[n].  Everything else is GEM_NAV_UNREACHED.  int32.  size_x * size_y * max(w) >= 2^31 - 1 is
 *                refused.
 *   grid path    GridPath::getPath: c starts at the goal cell; while c is not the start cell the eight neighbours are scanned in the
 *                library's order (xd = -1, 0, 1 outer, yd = -1, 0, 1 inner, (0, 0) skipped), the smallest potential wins and strict <
 *                keeps the first; c steps there.  Cells off the map are skipped (the library has no such check and relies on the
 *                outline).  The path is the visited cells reversed: start to goal, both ends included; start = goal gives one cell.
 *                found = 0 and an empty path when the start or the goal is off the map or the goal's potential is GEM_NAV_UNREACHED
 *                (an impassable goal is unreached).  The walk ends because the potential strictly falls: a traversable non-start
 *                cell has a 4-neighbour smaller by its w.  World points are cell centres, origin + (m + 0.5) * resolution, computed
 *                on the host in double.
 *
 *   gem_navplan_weights   host only.
 *   gem_navplan_host      the host twin, no handle and no device: a binary-heap Dijkstra and the same getPath.  start_cell and
 *                goal_cell are (x, y); pot (may be NULL) takes size_x * size_y ints, path_cells (may be NULL) the path's linear cells
 *                y * size_x + x.  rounds and chunks are 0.  With path_cells not NULL, cap below n_path: GEM_ERR_INVALID, status filled.
 *   gem_costmap_navplan   flags is 0 or GEM_NAV_OUTLINE.  out_xy (may be NULL) takes the path's world points, cap = the pairs it
 *                holds; cap below n_path: GEM_ERR_INVALID with the first cap points written and *st filled, like
 *                gem_mapgrid_adjust_plan.  The call WAITS.  The potential, the tiles' active maps, the path and the status live with
 *                the costmap in arenas that only grow: a second identical call allocates nothing.  status.rounds is the number of
 *                launches that found an active tile (it depends on timing: a tile may or may not see a neighbour's new edge in the
 *                round that writes it), status.chunks the number of host round trips.
 *   gem_costmap_navplan_status   the status of the last plan, as gem_costmap_navplan filled it: a caller that did not make the plan
 *                itself learns n_path here before it sizes the buffer of a read.  Host only: nothing is enqueued.
 *   gem_costmap_navplan_read   waits.  The last plan's potential (out_pot, may be NULL) and path cells (out_path_cells, may be NULL,
 *                cap ints; cap below the path's length: GEM_ERR_INVALID).
 *
 * GEM_ERR_INVALID, nothing enqueued and nothing changed: a bad id; a handle with a communicator; a NULL w, start, goal or status, a
 * negative weight; non-finite coordinates; unknown flag bits; the overflow condition; sizes below 1 (host twin); a read or a status
 * before any plan, or after the costmap rolled (gem_costmap_update_origin / _roll_to moved it), was observed (gem_costmap_observe* or
 * gem_costmap_voxel_observe* with at least one observation) or was created anew: the generation number of
 * gem_hip_mapgrid.h. */
#define GEM_NAV_OUTLINE   1
#define GEM_NAV_UNREACHED 0x7fffffff
typedef struct gem_navplan_status {
    int found;              /* 1: the path runs from the start to the goal */
    int n_path;             /* its cells, both ends included; 0 without one */
    int rounds, chunks;     /* launches that found an active tile | host round trips (both 0 from the host twin) */
    int goal_potential;     /* GEM_NAV_UNREACHED when there is none */
    int start_cell[2];      /* (x, y); (-1, -1) off the map */
    int goal_cell[2];
} gem_navplan_status;
int  gem_navplan_weights(int neutral_cost, double cost_factor, int lethal_cost, int allow_unknown, int out[256]);
int  gem_navplan_host(const unsigned char* grid, int size_x, int size_y, const int* w, int flags, const int start_cell[2], const int goal_cell[2],
                      int* pot, int* path_cells, long long cap, gem_navplan_status* status);
int  gem_costmap_navplan(gem_handle* h, int id, const double start_xy[2], const double goal_xy[2], const int* w, int flags, double* out_xy,
                         long long cap, gem_navplan_status* st);
int  gem_costmap_navplan_status(gem_handle* h, int id, gem_navplan_status* st);
int  gem_costmap_navplan_read(gem_handle* h, int id, int* out_pot, int* out_path_cells, long long cap);
