/* gem_hip_frontier.h -- frontier search on the device costmap: the part of the C ABI of libgem_hip.so that turns the edge of the mapped
 * space into the next goal of an exploration cycle, where the costmap lies.  Included by gem_hip.h, not on its own.  Symbols only
 * added: GEM_ABI_VERSION is unchanged.
 *
 * The cycle is ... -> inflate -> gem_costmap_navplan(start = goal = robot) -> gem_costmap_frontiers -> gem_costmap_navplan_goal(the
 * winner's access cell); the grid is never downloaded.  gem_costmap_navplan's potential is the converged one everywhere
 * (gem_hip_navplan.h), so it already says which known cells the robot reaches and at what cost; what is added here is the labelling of
 * the frontier cells into connected frontiers, their reduction to records, and the pick.
 *
 * The contract is written IN THE MANNER OF explore_lite's FrontierSearch (searchFrom, isNewFrontierCell, buildNewFrontier,
 * frontierCost), RECALLED FROM MEMORY and NOT VERIFIED against the library (there is none here).  tests/frontier_ref.py is the same
 * statement in numpy / plain Python, twice.  It DELIBERATELY DEPARTS from the library in four places:
 *   - reachability comes from the plan's potential, not from the library's BFS over non-increasing costs from the robot's cell;
 *   - the travel cost (the potential at the cheapest point of access) replaces the Euclidean min_distance;
 *   - exact integer coordinate sums replace the library's double sums in visiting order (the centroid is one division at the end);
 *   - the access cell (the cheapest door, below) replaces the library's `initial` and `middle` points.
 * Everything except the final cost is an integer; the cost is double operations each rounded on its own (no fused multiply-add).
 *
 *   inputs       the costmap's bytes as they are when the call runs on the stream (size_y rows of size_x), and the potential `pot` of
 *                the costmap's last plan.  Keeping the two consistent -- no mark, merge or inflation between the plan and the search --
 *                is the CALLER'S business: nothing checks it.  A costmap without a plan, or whose plan predates its last roll or observe call, is
 *                refused by the generation test of gem_costmap_navplan_read.
 *   known(n)     byte[n] != 255.          reached(n)   pot[n] != GEM_NAV_UNREACHED.
 *   doors of c   its 4-neighbours on the map that are known and reached.  The plan's start cell has potential 0 whatever its byte: it
 *                is a door only if it is known.
 *   frontier cell   byte[c] == 255 and c has at least one door.  Its access key is the lexicographic minimum of (pot[n], n) over its
 *                doors n, n the linear cell y * size_x + x.  Callers are advised to plan with allow_unknown = 0: with it on, a door may
 *                have been reached THROUGH unknown space.  That is not forbidden; the definitions hold either way.
 *   frontier     an 8-connected component of the set of frontier cells.  root: its smallest linear cell, its identity.  size: its cell
 *                count.  sum_x, sum_y: the sums of its cells' x and y, int64.  (access_potential, access_cell): the minimum access key
 *                over its cells.
 *   kept         iff (double)size * resolution >= min_frontier_size.
 *   cost         potential_scale * (double)access_potential - gain_scale * ((double)size * resolution), each operation rounded on its
 *                own.
 *   best         the kept frontier of least cost, compared with <; among equals the smaller root wins; -0.0 and +0.0 are equal.
 *   centroid     host only, in the facades: origin + ((double)sum / (double)size + 0.5) * resolution.
 *
 *   gem_frontiers_host     the host twin, no handle and no device: a flood fill in plain C++.  out_labels (may be NULL) takes size_x *
 *                size_y ints, the root of the cell's frontier or -1 for a cell that is no frontier cell; out (may be NULL) takes the
 *                KEPT frontiers in ascending root order, cap = the records it holds.  With out not NULL, cap below n_kept:
 *                GEM_ERR_INVALID with the status filled and nothing written to out.  rounds and chunks are 0.
 *   gem_costmap_frontiers  takes the handle's lock and runs on the handle's stream behind whatever was enqueued.  The call WAITS, as
 *                gem_costmap_navplan does: labels are relaxed tile by tile, a launch per round, and the host drives the rounds.  It
 *                fills *status, the winner included, so the answer needs no second call.  Its arenas live with the costmap and only
 *                grow: a second identical call allocates nothing.  status.rounds is the number of launches that found an active tile
 *                (it depends on timing, nothing else does), status.chunks the number of host round trips.
 *   gem_costmap_frontiers_read   waits.  The last search's kept list (out, may be NULL, cap records; cap below n_kept:
 *                GEM_ERR_INVALID) and label grid (out_labels, may be NULL).  Refused before any search, after a roll or an observe call, and after a new
 *                gem_costmap_navplan: a search carries the plan it was made from.  gem_costmap_navplan_goal leaves the potential
 *                alone and so keeps the search.
 *   gem_costmap_navplan_goal   the grid path from the last plan's start to ANOTHER goal on the last plan's potential, which it does not
 *                touch: one launch of the plan's path walk.  On a costmap whose bytes did not change, everything in *st except rounds
 *                and chunks, the world points, and what gem_costmap_navplan_read returns afterwards are exactly what
 *                gem_costmap_navplan with the same start, weights, flags and this goal would have produced.  st->rounds stays the
 *                plan's, st->chunks is 1.  It replaces the costmap's last path and status.  out_xy and cap as in gem_costmap_navplan.
 *                The call waits.
 *
 * GEM_ERR_INVALID, nothing enqueued and nothing changed: a bad id; a handle with a communicator; NULL params or status (a NULL goal or
 * status); a parameter that is not finite, is negative or is above 1e100 (so no product overflows and no NaN can arise); sizes below 1,
 * a NULL grid or pot, a resolution not finite and positive (host twin); non-finite goal coordinates; no plan, or a stale one; a read
 * before any search; cap below the list's length. */
typedef struct gem_frontier_params { double min_frontier_size, potential_scale, gain_scale; } gem_frontier_params;
typedef struct gem_frontier {          /* 40 bytes */
    int root, size;
    long long sum_x, sum_y;
    int access_potential, access_cell;
    double cost;
} gem_frontier;
typedef struct gem_frontier_status {
    int n_cells;        /* frontier cells */
    int n_frontiers;    /* components */
    int n_kept;
    int best;           /* index into the kept list (ascending root), -1 without one */
    int rounds, chunks; /* as in gem_navplan_status; rounds depends on timing, nothing else does */
    gem_frontier best_frontier;     /* all zero, root -1, without one */
} gem_frontier_status;
int  gem_frontiers_host(const unsigned char* grid, const int* pot, int size_x, int size_y, double resolution, const gem_frontier_params* params,
                        int* out_labels, gem_frontier* out, long long cap, gem_frontier_status* status);
int  gem_costmap_frontiers(gem_handle* h, int id, const gem_frontier_params* params, gem_frontier_status* status);
int  gem_costmap_frontiers_read(gem_handle* h, int id, gem_frontier* out, long long cap, int* out_labels);
int  gem_costmap_navplan_goal(gem_handle* h, int id, const double goal_xy[2], double* out_xy, long long cap, gem_navplan_status* st);
