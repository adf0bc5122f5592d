// gem_capi_navplan.cpp -- the global-plan entry points of include/gem_hip_navplan.h: the weight table and the host twin (host only),
// gem_costmap_navplan and its read-back; and those of include/gem_hip_navquad.h, the quadratic potential: gem_navquad_host and
// gem_costmap_navplan_quadratic, which share everything here with the linear plan but the potential itself.  The kernels are in
// gem_navplan.hip and gem_navquad.hip, the path routine in gem_navpath.hpp, the quadratic cell update in gem_navquad.hpp.
//
// gem_costmap_navplan maps start and goal with worldToMap on the host (it knows the geometry after rolling), hands the weight table
// over in pinned host memory and enqueues: init, then CHUNKS of rounds, each chunk closed by k_nav_finish, which answers through the
// pinned status words: "a tile is still marked", or the walked path.  The host loop and its bound are run_tile_rounds' (gem_rounds.hpp);
// a chunk is tiles_x + tiles_y rounds (gem_debug_set "nav_chunk" sets another length).
// The potential, the active maps, the path and the status live with the costmap (Map::nav_*), the device table and the pinned block
// with the handle's costmaps; all come from ensure() and only grow, so a second identical call allocates nothing.
#include "gem_costmap_host.hpp"
#include "gem_navplan.hpp"
#include "gem_navquad.hpp"
#include "gem_rounds.hpp"

#include <algorithm>
#include <cmath>
#include <queue>
#include <utility>

namespace {

static_assert(kNavUnreached == GEM_NAV_UNREACHED, "the kernels' constant is the header's");
constexpr long long kNavLimit = 2147483647ll;                       // 2^31 - 1
constexpr size_t kNavPinBytes = (256 + kNavStatusWords) * sizeof(int);

// a table the contract admits for this many cells: no negative weight, cells * max(w) below 2^31 - 1
bool weights_ok(const int* w, long long cells)
{
    long long top = 0;
    for (int c = 0; c < 256; ++c) {
        if (w[c] < 0) return false;
        top = std::max<long long>(top, w[c]);
    }
    return cells >= 1 && cells < kNavLimit && cells * top < kNavLimit;
}

void empty_status(gem_navplan_status* st)
{
    *st = gem_navplan_status{};
    st->goal_potential = GEM_NAV_UNREACHED;
    st->start_cell[0] = st->start_cell[1] = st->goal_cell[0] = st->goal_cell[1] = -1;
}

// the contract's potential by a binary-heap Dijkstra: the minimum over 4-connected paths is what the heap settles, whatever the order
void host_potential(const unsigned char* grid, int sx, int sy, const int* w, bool outline, int start, int* pot)
{
    const long long cells = (long long)sx * sy;
    std::fill(pot, pot + cells, GEM_NAV_UNREACHED);
    if (start < 0) return;
    auto weight = [&](int x, int y) {
        if (outline && (x == 0 || y == 0 || x == sx - 1 || y == sy - 1)) return 0;
        return w[grid[(size_t)y * sx + x]];
    };
    using Item = std::pair<int, int>;                                   // potential, cell
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    pot[start] = 0;
    heap.push({0, start});
    const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, -1, 1};
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        if (it.first != pot[it.second]) continue;                       // an entry a smaller one overtook
        const int cx = it.second % sx, cy = it.second / sx;
        for (int k = 0; k < 4; ++k) {
            const int x = cx + dx[k], y = cy + dy[k];
            if (x < 0 || y < 0 || x >= sx || y >= sy) continue;
            const int n = y * sx + x, wn = n == start ? 0 : weight(x, y);
            if (wn <= 0) continue;
            const int cand = it.first + wn;                             // below 2^31 - 1: cells * max(w) is
            if (cand < pot[n]) { pot[n] = cand; heap.push({cand, n}); }
        }
    }
}

// the kernels' argument block bound to a costmap whose arenas and pinned block exist: sizes, tiles, grid, arenas, pin (its status
// words cleared); start, goal, outline and round are the caller's
NavArgs bind_args(gem_handle* h, CostMap& m)
{
    auto& cm = h->costmap;
    NavArgs a{};
    a.sx = (int)m.cfg.size_x; a.sy = (int)m.cfg.size_y; a.ntx = nav_tiles(a.sx); a.nty = nav_tiles(a.sy);
    a.grid = grid_of(m);
    a.w = static_cast<int*>(cm.nav_w.p);
    a.pot = static_cast<int*>(m.nav_pot.p); a.act = static_cast<int*>(m.nav_act.p);
    a.path = static_cast<int*>(m.nav_path.p); a.status = static_cast<int*>(m.nav_status.p);
    a.pin = static_cast<int*>(cm.nav_pin);
    volatile int* pin_status = a.pin + 256;
    for (int i = 0; i < kNavStatusWords; ++i) pin_status[i] = 0;
    return a;
}

// behind the wait for k_nav_finish: its answer out of the pinned words into *st (rounds and chunks are the caller's), the plan on
// record in generation `gen`, the path downloaded and its cells' centres in out_xy
int finish_plan(gem_handle* h, CostMap& m, const NavArgs& a, unsigned long long gen, const char* what, gem_navplan_status* st, double* out_xy,
                long long cap)
{
    auto& cm = h->costmap;
    const volatile int* pin_status = a.pin + 256;
    st->found = pin_status[kNavFound];
    st->n_path = pin_status[kNavNPath];
    st->goal_potential = pin_status[kNavGoalPot];
    m.nav_gen = gen;
    m.nav_n_path = st->n_path;
    m.nav_last = *st;
    const long long n = st->n_path, cells = (long long)a.sx * a.sy;
    cm.nav_cells.resize((size_t)n);
    if (n > 0) {
        HostXfer d{cm.nav_cells.data(), a.path + (cells - n), (size_t)n * sizeof(int)};
        if (const int rc = download_arrays(h, &d, 1, 0)) return rc;
    }
    if (!out_xy) return GEM_OK;
    const CostGeom g = geom_of(m);
    for (long long i = 0; i < std::min(n, cap); ++i) {
        const int c = cm.nav_cells[(size_t)i];
        out_xy[2 * i] = g.ox + ((double)(c % a.sx) + 0.5) * g.res;
        out_xy[2 * i + 1] = g.oy + ((double)(c / a.sx) + 0.5) * g.res;
    }
    return cap < n ? fail(h, GEM_ERR_INVALID, (std::string(what) + ": the path has more points than out_xy holds").c_str()) : GEM_OK;
}

// gem_costmap_navplan and gem_costmap_navplan_quadratic behind their preludes: the same checks, arenas, rounds and finish.  The
// quadratic plan differs in one more check (the weight limit), in its round launcher and in what the kernel makes of the table.
int plan_on_costmap(gem_handle* h, int id, const char* what, bool quadratic, const double start_xy[2], const double goal_xy[2], const int* w,
                    int flags, double* out_xy, long long cap, gem_navplan_status* st)
{
    const std::string name(what);
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, what, &m))) return rc;
    if (!start_xy || !goal_xy || !w || !st) return fail(h, GEM_ERR_INVALID, (name + ": a NULL start, goal, weight table or status").c_str());
    if (flags & ~GEM_NAV_OUTLINE) return fail(h, GEM_ERR_INVALID, (name + ": unknown flag bits").c_str());
    if (out_xy && cap < 0) return fail(h, GEM_ERR_INVALID, (name + ": a negative capacity").c_str());
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(start_xy[k]) || !std::isfinite(goal_xy[k])) return fail(h, GEM_ERR_INVALID, (name + ": a coordinate not finite").c_str());
    const CostGeom g = geom_of(*m);
    const long long cells = (long long)g.sx * g.sy;
    if (!weights_ok(w, cells)) return fail(h, GEM_ERR_INVALID, (name + ": a negative weight, or size_x * size_y * max(w) not below 2^31 - 1").c_str());
    if (quadratic && *std::max_element(w, w + 256) > kNavQuadMaxWeight) return fail(h, GEM_ERR_INVALID, (name + ": a weight above 462").c_str());

    auto& cm = h->costmap;
    const size_t nt = (size_t)nav_tiles((int)g.sx) * nav_tiles((int)g.sy);
    if ((rc = ensure(h, m->nav_pot, (size_t)cells * sizeof(int))) || (rc = ensure(h, m->nav_path, (size_t)cells * sizeof(int))) ||
        (rc = ensure(h, m->nav_act, 2 * nt * sizeof(int))) || (rc = ensure(h, m->nav_status, kNavStatusWords * sizeof(int))) ||
        (rc = ensure(h, cm.nav_w, 256 * sizeof(int)))) return rc;
    if (!cm.nav_pin) GEM_HIP(h, hipHostMalloc(&cm.nav_pin, kNavPinBytes, hipHostMallocDefault));
    NavArgs a = bind_args(h, *m);
    std::copy(w, w + 256, a.pin);

    empty_status(st);
    uint32_t cell = 0u;
    a.start = cost_cell(g, start_xy[0], start_xy[1], cell) ? (int)cell : -1;
    a.goal = cost_cell(g, goal_xy[0], goal_xy[1], cell) ? (int)cell : -1;
    if (a.start >= 0) { st->start_cell[0] = a.start % a.sx; st->start_cell[1] = a.start / a.sx; }
    if (a.goal >= 0) { st->goal_cell[0] = a.goal % a.sx; st->goal_cell[1] = a.goal / a.sx; }
    a.outline = (flags & GEM_NAV_OUTLINE) ? 1 : 0;
    a.passes = h->navquad_passes > 0 ? h->navquad_passes : kNavQuadPasses;

    m->nav_gen = 0;                                                     // (a failure below leaves no plan to read)
    m->nav_n_path = 0;
    m->fr_gen = 0;                                                      // (a frontier search carries the plan it was made from)
    GEM_HIP(h, launch_nav_init(h->stream, a));
    const volatile int* pin_status = a.pin + 256;
    RoundsResult rr;
    rc = run_tile_rounds(
        cells, h->nav_chunk > 0 ? h->nav_chunk : (long long)a.ntx + a.nty,
        [&](int round) -> int {
            a.round = round;
            GEM_HIP(h, quadratic ? launch_navquad_round(h->stream, a) : launch_nav_round(h->stream, a));
            return GEM_OK;
        },
        [&](int round, bool& converged) -> int {
            a.round = round;
            GEM_HIP(h, launch_nav_finish(h->stream, a));
            GEM_HIP(h, hipStreamSynchronize(h->stream));
            converged = pin_status[kNavConverged] != 0;
            return GEM_OK;
        },
        rr);
    if (rc) return rc;
    if (!rr.converged) return fail(h, GEM_ERR_HIP, (name + ": the potential did not converge within its bound").c_str());
    st->rounds = pin_status[kNavRounds];
    st->chunks = rr.chunks;
    return finish_plan(h, *m, a, m->gen, what, st, out_xy, cap);
}

// gem_navplan_host and gem_navquad_host: the same checks, status and path; the potential is the caller's
int plan_on_host(bool quadratic, const unsigned char* grid, int size_x, int size_y, const int* w, int flags, const int start_cell[2],
                 const int goal_cell[2], int* pot, int* path_cells, long long cap, gem_navplan_status* status)
{
    if (!grid || !w || !start_cell || !goal_cell || !status || size_x < 1 || size_y < 1 || (flags & ~GEM_NAV_OUTLINE) || (path_cells && cap < 0))
        return GEM_ERR_INVALID;
    const long long cells = (long long)size_x * size_y;
    if (!weights_ok(w, cells)) return GEM_ERR_INVALID;
    if (quadratic && *std::max_element(w, w + 256) > kNavQuadMaxWeight) return GEM_ERR_INVALID;
    auto cell_of = [&](const int c[2]) { return c[0] >= 0 && c[1] >= 0 && c[0] < size_x && c[1] < size_y ? c[1] * size_x + c[0] : -1; };
    const int start = cell_of(start_cell), goal = cell_of(goal_cell);
    empty_status(status);
    if (start >= 0) { status->start_cell[0] = start_cell[0]; status->start_cell[1] = start_cell[1]; }
    if (goal >= 0) { status->goal_cell[0] = goal_cell[0]; status->goal_cell[1] = goal_cell[1]; }
    std::vector<int> own;
    if (!pot) { own.resize((size_t)cells); pot = own.data(); }
    if (quadratic) navquad_potential_host(grid, size_x, size_y, w, (flags & GEM_NAV_OUTLINE) != 0, start, pot);
    else host_potential(grid, size_x, size_y, w, (flags & GEM_NAV_OUTLINE) != 0, start, pot);
    if (goal >= 0) status->goal_potential = pot[goal];
    if (start < 0 || goal < 0 || pot[goal] == GEM_NAV_UNREACHED) return GEM_OK;
    const long long n = nav_grid_path(pot, size_x, size_y, start, goal, nullptr, 0);
    status->found = 1;
    status->n_path = (int)n;
    if (!path_cells) return GEM_OK;
    if (cap < n) return GEM_ERR_INVALID;
    nav_grid_path(pot, size_x, size_y, start, goal, path_cells, n);
    std::reverse(path_cells, path_cells + n);
    return GEM_OK;
}

} // namespace

extern "C" {

int gem_navplan_weights(int neutral_cost, double cost_factor, int lethal_cost, int allow_unknown, int out[256])
{
    if (!out || !std::isfinite(cost_factor) || lethal_cost < 1 || lethal_cost > 256 || neutral_cost < 0 || neutral_cost > 255) return GEM_ERR_INVALID;
    const float factor = (float)cost_factor, neutral = (float)neutral_cost;
    int table[256];
    for (int c = 0; c < 256; ++c) {
        table[c] = 0;
        if (!(c < lethal_cost - 1 || (allow_unknown && c == 255))) continue;
        const float prod = (float)c * factor;
        const float v = prod + neutral;                                 // (two float32 operations, each rounded on its own)
        if (!(v == v)) return GEM_ERR_INVALID;
        if (v >= (float)lethal_cost) { table[c] = lethal_cost - 1; }
        else {
            if (!(v > 0.0f) || v != std::floor(v)) return GEM_ERR_INVALID;      // the integer contract
            table[c] = (int)v;
        }
        if (table[c] <= 0) return GEM_ERR_INVALID;
    }
    std::copy(table, table + 256, out);
    return GEM_OK;
}

int gem_navplan_host(const unsigned char* grid, int size_x, int size_y, const int* w, int flags, const int start_cell[2], const int goal_cell[2],
                     int* pot, int* path_cells, long long cap, gem_navplan_status* status)
{
    return plan_on_host(false, grid, size_x, size_y, w, flags, start_cell, goal_cell, pot, path_cells, cap, status);
}

int gem_navquad_host(const unsigned char* grid, int size_x, int size_y, const int* w, int flags, const int start_cell[2], const int goal_cell[2],
                     int* pot, int* path_cells, long long cap, gem_navplan_status* status)
{
    return plan_on_host(true, grid, size_x, size_y, w, flags, start_cell, goal_cell, pot, path_cells, cap, status);
}

int gem_costmap_navplan(gem_handle* h, int id, const double start_xy[2], const double goal_xy[2], const int* w, int flags, double* out_xy,
                        long long cap, gem_navplan_status* st)
{
    GEM_ENTRY("gem_costmap_navplan");
    return plan_on_costmap(h, id, "gem_costmap_navplan", false, start_xy, goal_xy, w, flags, out_xy, cap, st);
}

int gem_costmap_navplan_quadratic(gem_handle* h, int id, const double start_xy[2], const double goal_xy[2], const int* w, int flags, double* out_xy,
                                  long long cap, gem_navplan_status* st)
{
    GEM_ENTRY("gem_costmap_navplan_quadratic");
    return plan_on_costmap(h, id, "gem_costmap_navplan_quadratic", true, start_xy, goal_xy, w, flags, out_xy, cap, st);
}

// Another goal on the last plan's potential (include/gem_hip_frontier.h): one launch of k_nav_finish.  After convergence both active
// maps are clear, so the kernel reports "converged" and walks; the potential is read, never written.
int gem_costmap_navplan_goal(gem_handle* h, int id, const double goal_xy[2], double* out_xy, long long cap, gem_navplan_status* st)
{
    GEM_ENTRY("gem_costmap_navplan_goal");
    const char* what = "gem_costmap_navplan_goal";
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, what, &m))) return rc;
    if (!goal_xy || !st) return fail(h, GEM_ERR_INVALID, "gem_costmap_navplan_goal: a NULL goal or status");
    if (out_xy && cap < 0) return fail(h, GEM_ERR_INVALID, "gem_costmap_navplan_goal: a negative capacity");
    if (!std::isfinite(goal_xy[0]) || !std::isfinite(goal_xy[1])) return fail(h, GEM_ERR_INVALID, "gem_costmap_navplan_goal: a coordinate not finite");
    if ((rc = costmap_plan_fresh(h, *m, what))) return rc;
    NavArgs a = bind_args(h, *m);                                       // (a plan was made on this handle: the arenas and the block exist)
    *st = m->nav_last;                                                  // (rounds are the plan's)
    uint32_t cell = 0u;
    a.start = st->start_cell[0] >= 0 ? st->start_cell[1] * a.sx + st->start_cell[0] : -1;
    a.goal = cost_cell(geom_of(*m), goal_xy[0], goal_xy[1], cell) ? (int)cell : -1;
    st->goal_cell[0] = a.goal >= 0 ? a.goal % a.sx : -1;
    st->goal_cell[1] = a.goal >= 0 ? a.goal / a.sx : -1;
    a.round = 0;                                                        // (either map: both are clear)
    const unsigned long long plan_gen = m->nav_gen;
    m->nav_gen = 0;                                                     // (a failure below leaves no path to read)
    m->nav_n_path = 0;
    GEM_HIP(h, launch_nav_finish(h->stream, a));
    GEM_HIP(h, hipStreamSynchronize(h->stream));
    const volatile int* pin_status = a.pin + 256;
    if (!pin_status[kNavConverged]) return fail(h, GEM_ERR_HIP, "gem_costmap_navplan_goal: a tile of the last plan is still marked");
    st->chunks = 1;
    return finish_plan(h, *m, a, plan_gen, what, st, out_xy, cap);
}

int gem_costmap_navplan_status(gem_handle* h, int id, gem_navplan_status* st)
{
    GEM_ENTRY("gem_costmap_navplan_status");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_navplan_status", &m))) return rc;
    if (!st) return fail(h, GEM_ERR_INVALID, "gem_costmap_navplan_status: a NULL status");
    if ((rc = costmap_plan_fresh(h, *m, "gem_costmap_navplan_status"))) return rc;
    *st = m->nav_last;
    return GEM_OK;
}

int gem_costmap_navplan_read(gem_handle* h, int id, int* out_pot, int* out_path_cells, long long cap)
{
    GEM_ENTRY("gem_costmap_navplan_read");
    const char* what = "gem_costmap_navplan_read";
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, what, &m))) return rc;
    if ((rc = costmap_plan_fresh(h, *m, what))) return rc;
    const long long n = m->nav_n_path, cells = (long long)m->cfg.size_x * m->cfg.size_y;
    if (out_path_cells && cap < n) return fail(h, GEM_ERR_INVALID, "gem_costmap_navplan_read: the path has more cells than out_path_cells holds");
    HostXfer d[2];
    int k = 0;
    if (out_pot) d[k++] = HostXfer{out_pot, m->nav_pot.p, (size_t)cells * sizeof(int)};
    if (out_path_cells && n > 0) d[k++] = HostXfer{out_path_cells, static_cast<int*>(m->nav_path.p) + (cells - n), (size_t)n * sizeof(int)};
    return k ? download_arrays(h, d, k, 0) : GEM_OK;
}

} // extern "C"
