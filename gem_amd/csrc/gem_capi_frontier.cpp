// gem_capi_frontier.cpp -- the frontier-search entry points of include/gem_hip_frontier.h: the host twin (host only),
// gem_costmap_frontiers and its read-back.  The kernels are in gem_frontier.hip; gem_costmap_navplan_goal is in gem_capi_navplan.cpp.
//
// gem_costmap_frontiers enqueues: the classification, then CHUNKS of label rounds, each chunk closed by k_front_check, which answers
// through pinned words: "a tile is still marked" or not.  The host loop and its bound are run_tile_rounds' (gem_rounds.hpp), as for the
// potential; a chunk is tiles_x + tiles_y rounds (gem_debug_set "front_chunk" sets another length).  Behind the last chunk the
// reduction is enqueued, and one more wait brings the status.
// The labels, the index scratch, the active maps, the records and the kept list live with the costmap (Map::fr_*), the compaction's
// block counts and the pinned block with the handle's costmaps; all come from ensure() and only grow.
#include "gem_costmap_host.hpp"
#include "gem_compact.hpp"
#include "gem_frontier.hpp"
#include "gem_rounds.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

// finite, not negative, at most 1e100: no product of the cost overflows and no NaN can arise
bool params_ok(const gem_frontier_params* p)
{
    for (double v : {p->min_frontier_size, p->potential_scale, p->gain_scale})
        if (!std::isfinite(v) || v < 0.0 || v > 1e100) return false;
    return true;
}

gem_frontier empty_frontier()
{
    gem_frontier f{};
    f.root = -1;
    return f;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

} // namespace

extern "C" {

int gem_frontiers_host(const unsigned char* grid, const int* pot, int size_x, int size_y, double resolution, const gem_frontier_params* params,
                       int* out_labels, gem_frontier* out, long long cap, gem_frontier_status* status)
{
    if (!grid || !pot || !params || !status || size_x < 1 || size_y < 1 || !std::isfinite(resolution) || !(resolution > 0.0) || !params_ok(params) ||
        (out && cap < 0))
        return GEM_ERR_INVALID;
    const long long cells = (long long)size_x * size_y;
    if (cells >= 2147483647ll) return GEM_ERR_INVALID;
    const int sx = size_x, sy = size_y;
    constexpr unsigned long long no_key = ~0ull;
    std::vector<unsigned long long> key((size_t)cells, no_key);         // a frontier cell's access key; no_key: no frontier cell
    int n_cells = 0;
    const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, -1, 1};
    for (int y = 0; y < sy; ++y)
        for (int x = 0; x < sx; ++x) {
            const size_t c = (size_t)y * sx + x;
            if (grid[c] != 255) continue;
            for (int k = 0; k < 4; ++k) {
                const int nx = x + dx[k], ny = y + dy[k];
                if (nx < 0 || ny < 0 || nx >= sx || ny >= sy) continue;
                const size_t n = (size_t)ny * sx + nx;
                if (grid[n] == 255 || pot[n] == GEM_NAV_UNREACHED) continue;
                key[c] = std::min(key[c], ((unsigned long long)(unsigned)pot[n] << 32) | (unsigned long long)n);
            }
            n_cells += key[c] != no_key;
        }
    // a flood fill over 8-neighbours from every unlabelled frontier cell in ascending order: the seed is its component's smallest cell
    std::vector<int> own;
    int* label = out_labels;
    if (!label) { own.resize((size_t)cells); label = own.data(); }
    std::fill(label, label + cells, -1);
    std::vector<gem_frontier> all;
    std::vector<int> stack;
    for (long long seed = 0; seed < cells; ++seed) {
        if (key[(size_t)seed] == no_key || label[seed] >= 0) continue;
        gem_frontier f{};
        f.root = (int)seed;
        unsigned long long best = no_key;
        label[seed] = (int)seed;
        stack.push_back((int)seed);
        while (!stack.empty()) {
            const int c = stack.back();
            stack.pop_back();
            const int cx = c % sx, cy = c / sx;
            ++f.size; f.sum_x += cx; f.sum_y += cy;
            best = std::min(best, key[(size_t)c]);
            for (int yd = -1; yd <= 1; ++yd)
                for (int xd = -1; xd <= 1; ++xd) {
                    const int x = cx + xd, y = cy + yd;
                    if (x < 0 || y < 0 || x >= sx || y >= sy) continue;
                    const int n = y * sx + x;
                    if (key[(size_t)n] == no_key || label[n] >= 0) continue;
                    label[n] = (int)seed;
                    stack.push_back(n);
                }
        }
        f.access_potential = (int)(best >> 32);
        f.access_cell = (int)(best & 0xffffffffull);
        all.push_back(f);
    }
    *status = gem_frontier_status{};
    status->n_cells = n_cells;
    status->n_frontiers = (int)all.size();
    status->best = -1;
    status->best_frontier = empty_frontier();
    std::vector<gem_frontier> kept;
    for (gem_frontier& f : all) {
        const double gain = (double)f.size * resolution;
        const double travel = params->potential_scale * (double)f.access_potential;
        const double gained = params->gain_scale * gain;
        f.cost = travel - gained;                                       // (each operation rounded on its own: -ffp-contract=off)
        if (!(gain >= params->min_frontier_size)) continue;
        if (status->best < 0 || f.cost < status->best_frontier.cost) {  // ascending roots and a strict <: the smaller root wins a tie
            status->best = (int)kept.size();
            status->best_frontier = f;
        }
        kept.push_back(f);
    }
    status->n_kept = (int)kept.size();
    if (!out) return GEM_OK;
    if (cap < (long long)kept.size()) return GEM_ERR_INVALID;
    std::copy(kept.begin(), kept.end(), out);
    return GEM_OK;
}

int gem_costmap_frontiers(gem_handle* h, int id, const gem_frontier_params* params, gem_frontier_status* status)
{
    GEM_ENTRY("gem_costmap_frontiers");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_frontiers", &m))) return rc;
    if (!params || !status) return fail(h, GEM_ERR_INVALID, "gem_costmap_frontiers: NULL params or status");
    if (!params_ok(params)) return fail(h, GEM_ERR_INVALID, "gem_costmap_frontiers: a parameter that is not finite, is negative or is above 1e100");
    if ((rc = costmap_plan_fresh(h, *m, "gem_costmap_frontiers"))) return rc;

    auto& cm = h->costmap;
    FrontArgs a{};
    a.sx = (int)m->cfg.size_x; a.sy = (int)m->cfg.size_y; a.ntx = nav_tiles(a.sx); a.nty = nav_tiles(a.sy);
    const long long cells = (long long)a.sx * a.sy;
    const size_t nt = (size_t)a.ntx * a.nty, n_rec = (size_t)front_max_records(a.sx, a.sy);
    // the records, field by field: root | size | sum_x | sum_y | key, each 256-byte aligned
    const size_t o_size = align256(n_rec * sizeof(int)), o_sx = o_size + align256(n_rec * sizeof(int)), o_sy = o_sx + align256(n_rec * 8),
                 o_key = o_sy + align256(n_rec * 8), rec_bytes = o_key + align256(n_rec * 8);
    const size_t nb = (size_t)compact_blocks(cells);
    if ((rc = ensure(h, m->fr_label, (size_t)cells * sizeof(int))) || (rc = ensure(h, m->fr_index, (size_t)cells * sizeof(int))) ||
        (rc = ensure(h, m->fr_act, 2 * nt * sizeof(int))) || (rc = ensure(h, m->fr_rec, rec_bytes)) ||
        (rc = ensure(h, m->fr_out, n_rec * sizeof(gem_frontier))) || (rc = ensure(h, m->fr_words, kFrontWords * sizeof(int))) ||
        (rc = ensure(h, cm.fr_blocks, (nb + 1) * sizeof(uint32_t)))) return rc;
    if (!cm.fr_pin) GEM_HIP(h, hipHostMalloc(&cm.fr_pin, sizeof(FrontPin), hipHostMallocDefault));
    volatile FrontPin* pin = static_cast<FrontPin*>(cm.fr_pin);
    pin->converged = 0; pin->rounds = 0;

    a.grid = grid_of(*m);
    a.pot = static_cast<int*>(m->nav_pot.p);
    a.label = static_cast<int*>(m->fr_label.p); a.index = static_cast<int*>(m->fr_index.p);
    a.act = static_cast<int*>(m->fr_act.p); a.words = static_cast<int*>(m->fr_words.p);
    unsigned char* rec = static_cast<unsigned char*>(m->fr_rec.p);
    a.rec.root = reinterpret_cast<int*>(rec); a.rec.size = reinterpret_cast<int*>(rec + o_size);
    a.rec.sum_x = reinterpret_cast<unsigned long long*>(rec + o_sx); a.rec.sum_y = reinterpret_cast<unsigned long long*>(rec + o_sy);
    a.rec.key = reinterpret_cast<unsigned long long*>(rec + o_key);
    a.out = static_cast<gem_frontier*>(m->fr_out.p);
    a.pin = static_cast<FrontPin*>(cm.fr_pin);
    a.resolution = m->cfg.resolution;
    a.params = *params;

    m->fr_gen = 0;                                                      // (a failure below leaves no search to read)
    m->fr_n_kept = 0;
    GEM_HIP(h, hipMemsetAsync(a.act, 0, 2 * nt * sizeof(int), h->stream));
    GEM_HIP(h, hipMemsetAsync(a.words, 0, kFrontWords * sizeof(int), h->stream));
    GEM_HIP(h, launch_front_classify(h->stream, a));
    RoundsResult rr;
    rc = run_tile_rounds(
        cells, h->front_chunk > 0 ? h->front_chunk : (long long)a.ntx + a.nty,
        [&](int round) -> int {
            a.round = round;
            GEM_HIP(h, launch_front_round(h->stream, a));
            return GEM_OK;
        },
        [&](int round, bool& converged) -> int {
            a.round = round;
            GEM_HIP(h, launch_front_check(h->stream, a));
            GEM_HIP(h, hipStreamSynchronize(h->stream));
            converged = pin->converged != 0;
            return GEM_OK;
        },
        rr);
    if (rc) return rc;
    if (!rr.converged) return fail(h, GEM_ERR_HIP, "gem_costmap_frontiers: the labels did not converge within their bound");
    GEM_HIP(h, launch_front_reduce(h->stream, a, static_cast<uint32_t*>(cm.fr_blocks.p)));
    GEM_HIP(h, hipStreamSynchronize(h->stream));
    *status = const_cast<const FrontPin*>(static_cast<FrontPin*>(cm.fr_pin))->status;
    status->chunks = rr.chunks;
    if (status->best < 0) status->best_frontier = empty_frontier();
    m->fr_gen = m->gen;
    m->fr_n_kept = status->n_kept;
    return GEM_OK;
}

int gem_costmap_frontiers_read(gem_handle* h, int id, gem_frontier* out, long long cap, int* out_labels)
{
    GEM_ENTRY("gem_costmap_frontiers_read");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_frontiers_read", &m))) return rc;
    if ((rc = costmap_search_fresh(h, *m, "gem_costmap_frontiers_read"))) return rc;
    const long long n = m->fr_n_kept, cells = (long long)m->cfg.size_x * m->cfg.size_y;
    if (out && cap < n) return fail(h, GEM_ERR_INVALID, "gem_costmap_frontiers_read: the list has more records than out holds");
    HostXfer d[2];
    int k = 0;
    if (out && n > 0) d[k++] = HostXfer{out, m->fr_out.p, (size_t)n * sizeof(gem_frontier)};
    if (out_labels) d[k++] = HostXfer{out_labels, m->fr_label.p, (size_t)cells * sizeof(int)};
    return k ? download_arrays(h, d, k, 0) : GEM_OK;
}

} // extern "C"
