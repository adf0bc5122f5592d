// plan_cover.cpp -- gem_amd/csrc/gem_plan.hpp on its own (no GPU): whatever gem_reserve's bound passes are planned to allocate covers
// the plan of every pass drawn from inside the bounds, buffer by buffer, on either pipeline; and the sub-tables of a sort plan's s_misc neither
// overlap nor leave the buffer.  Comparisons are exact.  Built with `hipcc --offload-host-only -x hip` (the header includes
// gem_kernels.hpp for the kernels' constants).
#include "../../gem_amd/csrc/gem_plan.hpp"

#include <cstdio>

using namespace gem;

static bool fits_always(int) { return true; }       // (the sort kernels' LDS check lives with sort_shape in the library)
static long long failures = 0;

#define SORT_BUFFERS(X) X(hv) X(key) X(src) X(cnt1) X(cnt2) X(misc) X(blkcnt) X(ranges) X(shard) X(tables.total)
#define TILE_BUFFERS(X) X(rec) X(srt) X(seg) X(flag) X(gflag) X(bkt) X(bcnt) X(fctl) X(spill) X(tables.total)

struct Cover { SortPlan sort{}; TilePlan tile{}; bool declined = false; };

static Cover cover_of(const PlanEnv& e, long long P, int S, int ranks, bool colours)
{
    Cover c;
    BoundPlan plan[kMaxBoundPlans];
    const int n = bound_plans(e, P, S, ranks, colours, fits_always, plan);
    for (int i = 0; i < n; ++i) {
        const BoundPlan& p = plan[i];
        if (p.kind == 0) c.declined = true;
#define MAX_SORT(f) if (p.kind == 1) c.sort.f = std::max(c.sort.f, p.sort.f);
#define MAX_TILE(f) if (p.kind == 2) c.tile.f = std::max(c.tile.f, p.tile.f);
        SORT_BUFFERS(MAX_SORT) TILE_BUFFERS(MAX_TILE)
    }
    return c;
}

static void fail_line(const char* what, const PlanEnv& e, long long P, int S, long long n, int sweeps, size_t need, size_t have)
{
    if (++failures <= 20)
        std::printf("FAIL %s: L=%d form=%d passes=%d chunk=%d min=%lld bounds=(%lld, %d) pass n=%lld sweeps=%d needs %zu, reserved %zu\n",
                    what, e.L, e.sort_form, e.sort_passes, e.sort_chunk, e.sort_min_points, P, S, n, sweeps, need, have);
}

static void check_sort(const PlanEnv& e, const Cover& c, const SortGeometry& g, long long P, int S, long long n, int sweeps, const long long* off, bool colours, bool shard)
{
    const size_t chunk = (size_t)sort_chunk_for(n, e.sort_chunk);
    size_t nc1 = 0;
    for (int s = 0; s < sweeps; ++s) nc1 += ((size_t)(off[s + 1] - off[s]) + chunk - 1) / chunk;
    const SortPlan p = sort_plan(g.n_passes, g.dbins, n, nc1, ((size_t)n + chunk - 1) / chunk, sweeps, colours, walk_blocks(g, shard), shard);
#define LE_SORT(f) if (p.f > c.sort.f) fail_line("sorted " #f, e, P, S, n, sweeps, p.f, c.sort.f);
    SORT_BUFFERS(LE_SORT)
    // s_misc: segment sums per pass | record count + odd-flag word | bin bases | seg_cnt
    bool ok = true;
    for (int i = 0; i < g.n_passes; ++i) ok = ok && p.o_seg[i] + (size_t)g.dbins[i] * 16 <= (i + 1 < g.n_passes ? p.o_seg[i + 1] : p.o_total);
    ok = ok && p.o_total + 8 <= p.o_base && p.o_base + ((size_t)g.dbins[g.n_passes - 1] + 1) * 4 <= p.o_segcnt &&
         p.o_segcnt + nc1 * kSortSegsPerChunk * 4 <= p.misc;
    if (!ok) fail_line("s_misc layout", e, P, S, n, sweeps, p.misc, p.o_segcnt);
}

static void check_pass(const PlanEnv& e, const Cover& c, long long P, int S, long long n, int sweeps, const long long* off, bool colours)
{
    const PassChoice ch = choose_pass(e, n, sweeps, fits_always);
    if (ch.geo.ok) { check_sort(e, c, ch.geo, P, S, n, sweeps, off, colours, false); return; }
    const TilePlan p = tile_plan(e, n, sweeps, sweeps > 1 ? off : nullptr);
    if (p.err) { fail_line("tile plan error", e, P, S, n, sweeps, (size_t)p.err, 0); return; }
#define LE_TILE(f) if (p.f > c.tile.f) fail_line("tile " #f, e, P, S, n, sweeps, p.f, c.tile.f);
    TILE_BUFFERS(LE_TILE)
}

// offsets of n points in `sweeps` sweeps: an equal split, or the most skewed one the header allows (one sweep at twice the mean)
static void split(long long n, int sweeps, bool skewed, long long* off)
{
    const long long first = skewed ? std::min(n, 2 * n / sweeps) : n / sweeps;
    off[0] = 0; off[1] = sweeps == 1 ? n : first;
    for (int s = 1; s < sweeps; ++s) off[s + 1] = off[1] + (n - off[1]) * s / (sweeps - 1);
}

int main()
{
    const int Ls[] = {64, 75, 200, 600, 2400}, chunks[] = {0, 1024, 4096}, passes[] = {0, 2, 3};
    const struct { long long P; int S; } bounds[] = {{5000, 1}, {131072, 1}, {150000, 1}, {199999, 1}, {307200, 1}, {786432, 6}, {4194304, 32}};
    long long combos = 0, skipped = 0, checked_passes = 0;
    for (int L : Ls) for (int form = 0; form <= 2; ++form) for (int np : passes) for (int chunk : chunks) for (int min1 = 0; min1 <= 1; ++min1)
    for (int ring = 2; ring <= 4; ++ring) for (const auto& b : bounds) for (int colours = 0; colours <= 1; ++colours) {
        PlanEnv e{};
        e.L = L; e.sort_form = form; e.sort_passes = np; e.sort_chunk = chunk; e.sort_ring = ring; e.sort_path = true;
        e.sort_min_points = min1 ? 1 : 200000; e.sort_min_points_batch = min1 ? 1 : 390000;
        ++combos;
        const Cover c = cover_of(e, b.P, b.S, 0, colours != 0);
        if (c.declined) { ++skipped; continue; }      // (a geometry that is not ok for the bound itself, or a descriptor table beyond what gem_reserve takes on)
        // (the last two: around the largest pass that takes the small sort chunk -- more chunks than a larger pass has)
        // (and the largest passes the tile pipeline takes, just below the sorted thresholds)
        const long long ns[] = {1, 63, 64, 65, 4095, 4097, b.P / 2, b.P - 1, b.P, std::min(b.P, kSmallChunkPoints), std::min(b.P, kSmallChunkPoints + 1),
                                std::max(1ll, std::min(b.P, e.sort_min_points - 1)), std::max(1ll, std::min(b.P, e.sort_min_points_batch - 1))};
        const int sw[] = {1, 2, 3, b.S / 2, b.S - 1, b.S};       // (between 2 and S: fewer, longer sweeps than the bound's)
        for (long long n : ns) for (int k = 0; k < 6; ++k) {
            const int sweeps = sw[k];
            if (sweeps < 1 || sweeps > b.S || (k > 0 && sweeps <= sw[k - 1])) continue;
            for (int skewed = 0; skewed <= (sweeps > 1 ? 1 : 0); ++skewed) for (int col = 0; col <= colours; ++col) {
                long long off[33];
                split(n, sweeps, skewed != 0, off);
                check_pass(e, c, b.P, b.S, n, sweeps, off, col != 0);
                ++checked_passes;
            }
        }
        if (ring == 2 && !colours && b.S > 1)
            for (int W : {2, 8}) {                    // a sharded step's share: block-sorted, with the strip words and the block ranges
                const Cover cs = cover_of(e, b.P, b.S, W, false);
                const SortGeometry g = sort_digits(L, np, b.S, true, fits_always);
                if (cs.declined || !g.ok) continue;
                const long long share = (b.P + W - 1) / W;
                for (long long n : {1ll, 4097ll, share, std::min(share, kSmallChunkPoints), std::min(share, kSmallChunkPoints + 1)}) for (int skewed = 0; skewed <= 1; ++skewed) {
                    long long off[33];
                    split(n, b.S, skewed != 0, off);
                    check_sort(e, cs, g, b.P, b.S, n, b.S, off, false, true);
                    ++checked_passes;
                }
            }
    }
    std::printf("combinations %lld, skipped %lld, checked %lld (%lld passes), failures %lld\n", combos, skipped, combos - skipped, checked_passes, failures);
    if (failures || (combos - skipped) * 10 < combos * 9) return 1;
    std::printf("ok\n");
    return 0;
}
