// The baseline of tools/bench_footprint.py: what a caller does today with the window on the host -- a single-thread restatement of
// ObstacleCostFunction::scoreTrajectory over CostmapModel::footprintCost (the contract of include/gem_hip_footprint.h, with the line
// iterator's own loop), compiled by the tool with -O2 -ffp-contract=off.
#include <cmath>
#include <cstdlib>

namespace {

struct Map { const unsigned char* grid; unsigned sx, sy; double res, ox, oy; };

bool world_to_map(const Map& m, double wx, double wy, int& mx, int& my)
{
    if (!std::isfinite(wx) || !std::isfinite(wy) || wx < m.ox || wy < m.oy) return false;
    const double qx = (wx - m.ox) / m.res, qy = (wy - m.oy) / m.res;
    if (!(qx < 2147483648.0 && qy < 2147483648.0)) return false;
    mx = (int)qx; my = (int)qy;
    return (unsigned)mx < m.sx && (unsigned)my < m.sy;
}

int point_cost(unsigned char c, int flags) { return c == 255 ? -2 : (c == 254 || (c == 253 && (flags & 1))) ? -1 : c; }

// the first negative pointCost on line(x0, y0, x1, y1), else the maximum folded into best
int line_cost(const Map& m, int x0, int y0, int x1, int y1, int flags, int& best)
{
    const int dx = std::abs(x1 - x0), dy = std::abs(y1 - y0);
    int xinc1 = x1 >= x0 ? 1 : -1, xinc2 = xinc1, yinc1 = y1 >= y0 ? 1 : -1, yinc2 = yinc1, den, num, numadd, numpixels;
    if (dx >= dy) { xinc1 = 0; yinc2 = 0; den = dx; num = dx / 2; numadd = dy; numpixels = dx; }
    else { xinc2 = 0; yinc1 = 0; den = dy; num = dy / 2; numadd = dx; numpixels = dy; }
    int x = x0, y = y0;
    for (int cur = 0; cur <= numpixels; ++cur) {
        const int pc = point_cost(m.grid[(size_t)y * m.sx + (size_t)x], flags);
        if (pc < 0) return pc;
        if (pc > best) best = pc;
        num += numadd;
        if (num >= den) { num -= den; x += xinc1; y += yinc1; }
        x += xinc2; y += yinc2;
    }
    return 0;
}

int footprint_cost(const Map& m, const double* p, const double* spec, int n, int flags)
{
    int cx, cy;
    if (!world_to_map(m, p[0], p[1], cx, cy)) return -3;
    if (n < 3) {
        const unsigned char c = m.grid[(size_t)cy * m.sx + (size_t)cx];
        return c == 255 ? -2 : c >= 253 ? -1 : c;
    }
    int vx[32], vy[32];
    bool ok[32];
    for (int i = 0; i < n; ++i) {
        const double wx = p[0] + (spec[2 * i] * p[2] - spec[2 * i + 1] * p[3]), wy = p[1] + (spec[2 * i] * p[3] + spec[2 * i + 1] * p[2]);
        ok[i] = world_to_map(m, wx, wy, vx[i], vy[i]);
    }
    int best = 0;
    for (int i = 0; i < n; ++i) {
        const int j = (i + 1) % n;
        if (!ok[i] || !ok[j]) return -3;
        const int r = line_cost(m, vx[i], vy[i], vx[j], vy[j], flags, best);
        if (r < 0) return r;
    }
    return best;
}

} // namespace

extern "C" void host_score_trajectories(const unsigned char* grid, unsigned sx, unsigned sy, double res, double ox, double oy, const double* poses,
                                        long long n_traj, int T, const double* spec, int n_vertices, int flags, int* out_traj)
{
    const Map m{grid, sx, sy, res, ox, oy};
    for (long long t = 0; t < n_traj; ++t) {
        int cost = 0;
        for (int k = 0; k < T; ++k) {
            const int f = footprint_cost(m, poses + 4 * (t * T + k), spec, n_vertices, flags);
            if (f < 0) { cost = f; break; }
            cost = (flags & 2) ? cost + f : (f > cost ? f : cost);
        }
        out_traj[t] = cost;
    }
}
