/* gem_hip_inflate.h -- inflation on the device costmap: the part of the C ABI of libgem_hip.so that spreads InflationLayer's costs
 * around the lethal cells of a master where it lies, and Costmap2D::resetMap over a window.  Included by gem_hip.h, not on its own.
 * Symbols only added: GEM_ABI_VERSION is unchanged.
 *
 * Every device entry takes the handle's lock and only enqueues on the handle's stream: marks, clears and merges enqueued before it
 * are visible to it without a host wait, and a scoring call behind it sees its costs.  A cycle is
 *     reset_window(master) -> mark -> clear_footprint -> merge -> inflate -> score_trajectories.
 *
 * The contract is RESTATED from ROS noetic costmap_2d/src/inflation_layer.cpp (updateCosts, computeCaches, enqueue),
 * include/costmap_2d/inflation_layer.h (computeCost) and Costmap2D::cellDistance / resetMap(x0, y0, xn, yn) (tests/inflate_ref.py is
 * the same statement in numpy).  It is NOT verified against the library.
 *   parameters   {inflation_radius, inscribed_radius, cost_scaling_factor (the library's weight_), inflate_unknown}.
 *                R = (unsigned)max(0.0, ceil(inflation_radius / resolution)): cell_inflation_radius_ of cellDistance.
 *   cost table   made on the host, for d2 = 0 .. R * R with d = sqrt((double)d2):  d2 == 0 -> 254;  d * resolution <= inscribed_radius
 *                -> 253;  otherwise (unsigned char)((253 - 1) * exp(-1.0 * cost_scaling_factor * (d * resolution - inscribed_radius))).
 *                The library indexes its cache by (|dx|, |dy|) and takes d = hypot(dx, dy); the table here rests on
 *                hypot(i, j) == sqrt((double)(i * i + j * j)) for all i, j <= 128, which holds for a correctly rounded sqrt and glibc's
 *                hypot (tests/test_inflate_cpu.py repeats the check).  The table is the only place a float appears: the kernels are
 *                integer code.
 *   seeds        the window [min_i, max_i) x [min_j, max_j) is widened by R on every side and clamped to the map; the seeds are the
 *                cells equal to 254 inside the widened window when the call runs on the stream.
 *   every cell of the map (not only of the window, as in the library):  d2 = min over the seeds of dx * dx + dy * dy.  No seed with
 *                d2 <= R * R: unchanged.  Otherwise cost = table[d2], and with old the cell's byte: old == 255 and
 *                (inflate_unknown ? cost > 0 : cost >= 253) -> cost; otherwise max(old, cost).
 *   so           a 254 never appears or disappears (the seed predicate does not change under the call's own writes); every cell is
 *                written at most once, from its own old value; the call is idempotent; R == 0 changes nothing.
 * A DELIBERATE DIFFERENCE, next to worldToMap's non-finite input: the library propagates (cell, source obstacle) pairs through
 * 4-neighbours in bins of increasing distance, and that brushfire does not always reach a cell from its NEAREST obstacle (discrete
 * Voronoi regions are not 4-connected).  With lethal cells at (2, 2), (3, 0) and (0, 3) relative to p = (0, 0) the library gives p the
 * squared distance 9, the true one is 8.  This call uses the exact nearest lethal cell: where the brushfire over-estimates a
 * distance the library's cost is at or below the one here, elsewhere the two are equal (tests/test_inflate_cpu.py compares them:
 * no cell differs on structured inputs and sparse noise, a few in ten thousand on dense noise).
 *
 *   gem_inflation_table   host only, no handle and no device: *out_cells = R, and with out_table not NULL the R * R + 1 table bytes.
 *   gem_costmap_inflate   as above.  The table lives on the device per costmap, keyed by the parameters and the resolution: a
 *                second identical call uploads and allocates nothing (the call that makes a new table waits for its upload).
 *   gem_costmap_reset_window   Costmap2D::resetMap(x0, y0, xn, yn): the rows y0 <= y < yn become default_value for x0 <= x < xn.
 *                LayeredCostmap::updateMap does this to the master before the layers write; without it old inflation costs never
 *                leave a device master.
 * GEM_ERR_INVALID, nothing changed: a bad id; a handle with a communicator; NULL params; a non-finite or negative radius, inscribed
 * radius or scaling factor; a resolution not finite and positive (gem_inflation_table); R above GEM_INFLATE_MAX_CELLS; a window
 * outside the map (0 <= min <= max <= size).  An empty window is valid and changes nothing. */
typedef struct gem_inflation_params {
    double inflation_radius, inscribed_radius, cost_scaling_factor;
    int inflate_unknown;
} gem_inflation_params;
#define GEM_INFLATE_MAX_CELLS 127
int  gem_inflation_table(const gem_inflation_params* params, double resolution, unsigned char* out_table, int* out_cells);
int  gem_costmap_inflate(gem_handle* h, int id, const gem_inflation_params* params, int min_i, int min_j, int max_i, int max_j);
int  gem_costmap_reset_window(gem_handle* h, int id, int x0, int y0, int xn, int yn);
