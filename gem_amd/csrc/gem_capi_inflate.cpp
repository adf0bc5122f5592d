// gem_capi_inflate.cpp -- the inflation entry points of include/gem_hip_inflate.h: the cost table (host only), gem_costmap_inflate and
// Costmap2D::resetMap over a window.  The kernels are in gem_inflate.hip.
//
// The table is the only floating point of the feature and is made here, in double with every operation rounded on its own, for
// d2 = 0 .. R * R.  A costmap keeps its table on the device next to the key it was made for (the three doubles, compared as bits; the
// resolution is the costmap's own and never changes): a call with the same parameters uploads nothing.  The seed words and flags of a
// call live in Costmaps::infl_bits / infl_flags, which come from ensure() and only grow, so a loop that has reached its window
// allocates nothing (gem_debug_get("arena_allocations") counts).  gem_costmap_inflate enqueues two launches and waits for nothing,
// except in the call that uploads a new table.
#include "gem_costmap_host.hpp"
#include "gem_inflate.hpp"

#include <cmath>
#include <cstring>

namespace {

static_assert(kInflateMaxCells == GEM_INFLATE_MAX_CELLS, "the kernels' radius limit is the header's");

// cell_inflation_radius_ = cellDistance(inflation_radius_); false: the parameters or the resolution are not usable, or R is too large
bool inflation_cells(const gem_inflation_params* p, double res, unsigned* out_R)
{
    if (!p || !std::isfinite(res) || !(res > 0.0)) return false;
    for (double v : {p->inflation_radius, p->inscribed_radius, p->cost_scaling_factor})
        if (!std::isfinite(v) || v < 0.0) return false;
    const double cells = std::max(0.0, std::ceil(p->inflation_radius / res));
    if (!(cells <= (double)GEM_INFLATE_MAX_CELLS)) return false;
    *out_R = (unsigned)cells;
    return true;
}

// InflationLayer::computeCost at distance sqrt(d2) cells
unsigned char inflation_cost(const gem_inflation_params& p, double res, unsigned d2)
{
    if (d2 == 0u) return kCostLethal;
    const double distance = std::sqrt((double)d2);
    if (distance * res <= p.inscribed_radius) return kCostInscribed;
    const double euclidean_distance = distance * res;
    const double factor = std::exp(-1.0 * p.cost_scaling_factor * (euclidean_distance - p.inscribed_radius));
    return (unsigned char)((kCostInscribed - 1) * factor);
}

void fill_table(const gem_inflation_params& p, double res, unsigned R, unsigned char* out)
{
    for (unsigned d2 = 0; d2 <= R * R; ++d2) out[d2] = inflation_cost(p, res, d2);
}

bool same_key(const gem_inflation_params& a, const gem_inflation_params& b)
{
    return !memcmp(&a.inflation_radius, &b.inflation_radius, 8) && !memcmp(&a.inscribed_radius, &b.inscribed_radius, 8) &&
           !memcmp(&a.cost_scaling_factor, &b.cost_scaling_factor, 8);
}

} // namespace

extern "C" {

int gem_inflation_table(const gem_inflation_params* params, double resolution, unsigned char* out_table, int* out_cells)
{
    unsigned R;
    if (!inflation_cells(params, resolution, &R)) return GEM_ERR_INVALID;
    if (out_table) fill_table(*params, resolution, R, out_table);
    if (out_cells) *out_cells = (int)R;
    return GEM_OK;
}

int gem_costmap_inflate(gem_handle* h, int id, const gem_inflation_params* params, int min_i, int min_j, int max_i, int max_j)
{
    GEM_ENTRY("gem_costmap_inflate");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_inflate", &m))) return rc;
    unsigned R;
    if (!inflation_cells(params, m->cfg.resolution, &R))
        return fail(h, GEM_ERR_INVALID, "gem_costmap_inflate: NULL parameters, a radius or factor not finite or negative, or more than 127 cells");
    if (!window_ok(*m, min_i, min_j, max_i, max_j)) return fail(h, GEM_ERR_INVALID, "gem_costmap_inflate: window outside the map");
    if (R == 0u || min_i == max_i || min_j == max_j) return GEM_OK;     // a seed only confirms itself | no seeds
    if (!m->infl_valid || !same_key(m->infl_key, *params)) {
        std::vector<unsigned char> table((size_t)R * R + 1);
        fill_table(*params, m->cfg.resolution, R, table.data());
        m->infl_valid = false;
        if ((rc = ensure(h, m->infl_table, table.size()))) return rc;
        HostXfer up{table.data(), m->infl_table.p, table.size()};
        if ((rc = upload_arrays(h, &up, 1))) return rc;                 // (waits for the copy: `table` may go)
        m->infl_key = *params;
        m->infl_valid = true;
    }
    const InflateArgs a = inflate_args(m->cfg.size_x, m->cfg.size_y, min_i, min_j, max_i, max_j, R, params->inflate_unknown);
    auto& cm = h->costmap;
    if ((rc = ensure(h, cm.infl_bits, inflate_bits_bytes(a))) || (rc = ensure(h, cm.infl_flags, inflate_flags_bytes(a)))) return rc;
    unsigned long long* bits = static_cast<unsigned long long*>(cm.infl_bits.p);
    uint32_t* flags = static_cast<uint32_t*>(cm.infl_flags.p);
    GEM_HIP(h, launch_inflate_seeds(h->stream, grid_of(*m), a, bits, flags));
    GEM_HIP(h, launch_inflate(h->stream, grid_of(*m), a, bits, flags, static_cast<const unsigned char*>(m->infl_table.p)));
    return GEM_OK;
}

int gem_costmap_reset_window(gem_handle* h, int id, int x0, int y0, int xn, int yn)
{
    GEM_ENTRY("gem_costmap_reset_window");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_reset_window", &m))) return rc;
    if (!window_ok(*m, x0, y0, xn, yn)) return fail(h, GEM_ERR_INVALID, "gem_costmap_reset_window: window outside the map");
    GEM_HIP(h, launch_inflate_reset(h->stream, grid_of(*m), m->cfg.size_x, InflateBox{(uint32_t)x0, (uint32_t)y0, (uint32_t)xn, (uint32_t)yn},
                                    m->cfg.default_value));
    return GEM_OK;
}

} // extern "C"
