/* gem_hip_mapgrid_tiled.h -- path, goal and front distance grids on a device costmap of ANY size: the declarations of the tiled
 * prepare calls.  Included by gem_hip.h, not on its own.  Symbols only added: GEM_ABI_VERSION is unchanged.
 *
 * The contract is gem_hip_mapgrid.h's, unchanged to the byte (its paragraph gem_costmap_mapgrid_prepare_tiled says what differs: any
 * size, and the calls WAIT); the FRONT grid is gem_hip_critics.h's.  The grids land in the slots of gem_costmap_mapgrid_prepare /
 * _prepare_front with the same status words and generation, so every reader -- gem_costmap_mapgrid_read, _read_front, _score,
 * _score_device, gem_costmap_best_trajectory, _dwa_best, _rollout_best -- works behind them without a change.
 *
 * GEM_ERR_INVALID, nothing enqueued and nothing changed: the list of gem_costmap_mapgrid_prepare without the cap.  GEM_ERR_HIP: not
 * converged within size_x * size_y + 2 rounds; the requested grids then count as never prepared. */
typedef struct gem_mapgrid_tiled_status {
    int started;        /* as gem_costmap_mapgrid_read's */
    int goal_cell[2];   /* (x, y) of point b-1, (-1, -1) without one */
    int rounds, chunks; /* launches that found an active tile (timing-dependent) | host round trips */
} gem_mapgrid_tiled_status;
int  gem_costmap_mapgrid_prepare_tiled(gem_handle* h, int id, const double* plan_xy, long long n, int which, gem_mapgrid_tiled_status* st /* may be NULL */);
int  gem_costmap_mapgrid_prepare_front_tiled(gem_handle* h, int id, const double* plan_xy, long long n, gem_mapgrid_tiled_status* st /* may be NULL */);
