/* gem_hip_history.h -- the history cloud on the device: the part of the C ABI of libgem_hip.so that keeps ElevationMapping's
 * visualCloud_ (the input of visualPointMap, savingMap and, with grid_pc, of PointMapLayer: /robot0/history_point).  Included by
 * gem_hip.h, not on its own.  Symbols only added: GEM_ABI_VERSION is unchanged.
 *
 * The history is one flat log of PointXYZRGBICT records (32 bytes, as everywhere in gem_hip.h) in history order, bound to the handle.
 * It only grows until it is cleared or rebuilt; its capacity only grows, by at least doubling, so a frame loop that has reached its
 * sizes allocates nothing.  Every entry takes the handle's lock and runs on the handle's stream.
 *
 *   gem_history_enable         capacity > 0: the history is switched on, empty, with room for `capacity` records (on an enabled handle it
 *                starts over); 0: switched off, its memory freed.
 *   gem_local_spill            (gem_hip.h) while the history is enabled also appends the records it selected: the same records it writes
 *                to `points`, in the same order, device to device inside the same call -- visualCloud_.push_back(pt) of
 *                ElevationMapping.cpp:750-760.  `points` may be NULL as before: then only the counts cross the link.  With the history
 *                disabled the call is what it was.
 *   gem_history_append         n records of the caller's (host) behind the history: a saved map loaded again, a node that keeps part of
 *                the bookkeeping.  _device: device memory; the call only enqueues and the buffer is untouched until gem_synchronize, as for
 *                gem_add_device.
 *   gem_history_reset_from_global   visualCloud_.clear() (:788) plus the "Visual step" (:894-897): the history becomes every submap of
 *                the stack in stack order -- gem_global_export(-1)'s records, device to device; like the reference all submaps, not only
 *                the first optKeyframeNum.
 *   gem_history_clear          empties the history.
 *   gem_history_size           *out = its record count.
 *   gem_history_export         the history, followed by the last capture's grid cloud when with_grid_cloud != 0 (visualPointMap, :524-526;
 *                without it savingMap's cloud), into points (host); points NULL: only *out_count.
 *   gem_costmap_mark_history   gem_costmap_mark_points over the history where it lies, as one input: record i carries stamp index i.  It
 *                resolves as every mark does; bounds NULL only enqueues.  gem_costmap_mark_grid_cloud after it is the reference's
 *                visualCloud_ + grid_pc input.  The history has a bounding box per block of 4096 consecutive records; a block whose box
 *                lies off the costmap (one cell of margin on the far sides) is skipped whole, which changes nothing: worldToMap refuses
 *                those records, and a refused record reaches neither the grid nor the bounds (gem_hip_debug.h: "history_cull",
 *                "history_blocks", "history_blocks_culled").
 *
 * GEM_ERR_INVALID, with nothing changed: the history not enabled; a handle with a communicator; n < 0; NULL points with n > 0; a length
 * that would pass 2^31 - 2 records, the stamp limit of a mark (checked before anything is read or allocated; gem_local_spill fails the
 * same way); gem_history_reset_from_global without an enabled submap stack; with_grid_cloud without a capture; max_points below the
 * count; a bad costmap id or a travers_thresh that is not finite. */
int  gem_history_enable(gem_handle* h, long long capacity);
int  gem_history_append(gem_handle* h, const void* points, long long n);
int  gem_history_append_device(gem_handle* h, const void* d_points, long long n);
int  gem_history_reset_from_global(gem_handle* h);
int  gem_history_clear(gem_handle* h);
int  gem_history_size(gem_handle* h, long long* out_count);
int  gem_history_export(gem_handle* h, int with_grid_cloud, void* points, long long max_points, long long* out_count);
int  gem_costmap_mark_history(gem_handle* h, int id, double travers_thresh, double bounds[4]);
