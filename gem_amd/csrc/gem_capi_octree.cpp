// gem_capi_octree.cpp -- gem_octree_build / _build_device / _read and gem_local_compose_octrees of include/gem_hip.h: the insertion
// loop of pointCloudtoOctomap (EMg.cpp:1158-1173) and fullMapToMsg's byte stream.  The kernels are in gem_octree.hip.
//
// One build: the two tables (value and blend p per hit count, built here in the host's float / double and libm: they are the only
// place log and exp occur) -> keys, sort, leaves, k*, walkers, node counts, the stream -> the state words (the one readback).  Blocks
// of 512 and more leaves that are all hit (k* >= 3) are not walked on the device: their records come down, an exact sequential tree
// (Tree below: the contract's functions one for one) gives their terminals, and the back half of the kernels runs again.  Every
// device buffer comes from ensure() and is sized by the call's n, so a second call of the same size allocates nothing.
#include "gem_capi_internal.hpp"
#include "gem_octree.hpp"

#include <algorithm>
#include <cmath>

namespace {

constexpr size_t kRec = sizeof(LocalRecord);

struct Tables { float f[kOctTable]; double p[kOctTable]; uint32_t sat; float hit, cmin, cmax; };

float log_odds(double p) { return (float)std::log(p / (1.0 - p)); }

// false: the parameters are not acceptable (the caller reports GEM_ERR_INVALID)
bool make_tables(const gem_octree_params* q, Tables& t)
{
    if (!q || !std::isfinite(q->resolution) || !(q->resolution > 0.0)) return false;
    if (q->prob_hit != 0.0 && !(q->prob_hit > 0.5 && q->prob_hit < 1.0)) return false;
    for (double c : {q->clamp_min, q->clamp_max}) if (c != 0.0 && !(c > 0.0 && c < 1.0)) return false;
    const float hit = q->prob_hit == 0.0 ? (float)std::log(0.7 / 0.3) : log_odds(q->prob_hit);
    const float cmin = q->clamp_min == 0.0 ? (float)std::log(0.1192 / 0.8808) : log_odds(q->clamp_min);
    const float cmax = q->clamp_max == 0.0 ? (float)std::log(0.971 / 0.029) : log_odds(q->clamp_max);
    t.hit = hit; t.cmin = cmin; t.cmax = cmax;
    for (int i = 0; i < kOctTable; ++i) { t.f[i] = 0.0f; t.p[i] = 0.0; }
    int n = 0;
    while (!(t.f[n] >= cmax)) {
        if (n + 1 >= kOctTable) return false;                            // no saturation within 64 steps
        float v = t.f[n] + hit;
        v = v < cmin ? cmin : v; v = v > cmax ? cmax : v;
        if (!(v > t.f[n])) return false;                                 // not strictly increasing
        t.f[++n] = v;
    }
    if (n < 1) return false;
    t.sat = (uint32_t)n;
    for (int i = 0; i <= n; ++i) t.p[i] = 1. - 1. / (1. + std::exp((double)t.f[i]));
    return true;
}

// ---- the contract's functions, one for one, for the records of k* >= 3 blocks -------------------------------------------------------
struct Tree {
    struct Node { float v = 0.0f; uint32_t col = kOctWhite; int ch[8] = {-1, -1, -1, -1, -1, -1, -1, -1}; };
    std::vector<Node> pool;
    int root = -1;
    float hit, cmin, cmax;

    int make() { pool.emplace_back(); return (int)pool.size() - 1; }
    bool has_children(int n) const { for (int c : pool[n].ch) if (c >= 0) return true; return false; }
    int search(unsigned long long key) const
    {
        if (root < 0) return -1;
        int n = root;
        for (int d = kOctDepth - 1; d >= 0; --d) {
            const int c = pool[n].ch[(key >> (3 * d)) & 7];
            if (c >= 0) n = c;
            else return has_children(n) ? -1 : n;
        }
        return n;
    }
    uint32_t average(int n) const
    {
        uint32_t s[3] = {0, 0, 0}, c = 0;
        for (int k : pool[n].ch) if (k >= 0 && pool[k].col != kOctWhite) {
            s[0] += pool[k].col & 255u; s[1] += (pool[k].col >> 8) & 255u; s[2] += pool[k].col >> 16; ++c;
        }
        return c ? (s[0] / c) | (s[1] / c) << 8 | (s[2] / c) << 16 : kOctWhite;
    }
    bool prune(int n)
    {
        const int c0 = pool[n].ch[0];
        for (int c : pool[n].ch) if (c < 0 || has_children(c) || !(pool[c].v == pool[c0].v)) return false;
        pool[n].v = pool[c0].v; pool[n].col = pool[c0].col;
        if (pool[n].col != kOctWhite) pool[n].col = average(n);
        for (int& c : pool[n].ch) c = -1;                                // (the pool keeps the nodes; nothing refers to them)
        return true;
    }
    void recurs(int n, bool just_created, unsigned long long key, int depth)
    {
        if (depth == kOctDepth) {
            float v = pool[n].v + hit;
            v = v < cmin ? cmin : v; v = v > cmax ? cmax : v;
            pool[n].v = v;
            return;
        }
        const int pos = (int)((key >> (3 * (kOctDepth - 1 - depth))) & 7);
        bool created = false;
        if (pool[n].ch[pos] < 0) {
            if (!has_children(n) && !just_created) {
                for (int k = 0; k < 8; ++k) { const int c = make(); pool[c].v = pool[n].v; pool[c].col = pool[n].col; pool[n].ch[k] = c; }
            } else { const int c = make(); pool[n].ch[pos] = c; created = true; }
        }
        recurs(pool[n].ch[pos], created, key, depth + 1);
        if (!prune(n)) {
            float m = 0.0f; bool any = false;
            for (int c : pool[n].ch) if (c >= 0) { m = any ? std::max(m, pool[c].v) : pool[c].v; any = true; }
            pool[n].v = m;
        }
    }
    void insert(unsigned long long key, uint32_t rgb)
    {
        int s = search(key);
        if (!(s >= 0 && pool[s].v >= cmax)) {
            bool created = false;
            if (root < 0) { root = make(); created = true; }
            recurs(root, created, key, 0);
        }
        s = search(key);
        if (s < 0) return;
        Node& n = pool[s];
        if (n.col == kOctWhite) { n.col = rgb; return; }
        const double p = 1. - 1. / (1. + std::exp((double)n.v));
        uint32_t out = 0;
        for (int sh = 0; sh < 24; sh += 8) {
            const double v = (double)((n.col >> sh) & 255u) * p + (double)((rgb >> sh) & 255u) * (0.99 - p);
            out |= (uint32_t)(uint8_t)v << sh;
        }
        n.col = out;
    }
    // the childless nodes in key order: (level above the leaves, value, colour)
    template <class F> void terminals(int n, int depth, F&& f) const
    {
        if (!has_children(n)) { f(kOctDepth - depth, pool[n].v, pool[n].col); return; }
        for (int c : pool[n].ch) if (c >= 0) terminals(c, depth + 1, f);
    }
};

struct Carve {
    unsigned char* base; size_t at = 0;
    template <class T> T* take(size_t count) { T* p = reinterpret_cast<T*>(base + at); at += (count * sizeof(T) + 255) & ~(size_t)255; return p; }
};

// the arena `work` for a call of n records; returns the bytes it takes (base may be NULL for that)
size_t carve(OctArgs& a, unsigned char* base, long long n)
{
    Carve c{base};
    const size_t m = (size_t)n;
    a.key_in = c.take<unsigned long long>(m);
    a.key[0] = c.take<unsigned long long>(m); a.key[1] = c.take<unsigned long long>(m);
    a.src[0] = c.take<uint32_t>(m); a.src[1] = c.take<uint32_t>(m);
    a.heads = c.take<uint32_t>((m + kOctThreads - 1) / kOctThreads + 1);
    a.leaf_key = c.take<unsigned long long>(m); a.leaf_start = c.take<uint32_t>(m + 1);
    a.term = c.take<OctTerm>(m);
    a.off = c.take<uint32_t>(m); a.d0 = c.take<uint8_t>(m); a.kstar = c.take<uint8_t>(m);
    a.blk[0] = c.take<uint32_t>(m / 8 + 1); a.blk[1] = c.take<uint32_t>(m / 64 + 1);
    return c.at;
}

size_t work_bytes(long long n) { OctArgs a{}; return carve(a, nullptr, n); }

int check_common(gem_handle* h, int slot, const char* what)
{
    const std::string w(what);
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, (w + ": not on a handle with a communicator").c_str());
    if (slot < 0 || slot >= gem_handle::Octree::kSlots) return fail(h, GEM_ERR_INVALID, (w + ": slot out of range (0 .. 3)").c_str());
    return GEM_OK;
}

// k* >= 3: the terminals of those leaves from the sequential tree, patched into OctArgs::term
int host_blocks(gem_handle* h, const OctArgs& a, const OctState& st, const Tables& t, const LocalRecord* host_in)
{
    const size_t nl = st.nleaves, S = st.S;
    std::vector<uint8_t> ks(nl);
    std::vector<unsigned long long> lkey(nl);
    std::vector<uint32_t> start(nl + 1), src(S);
    std::vector<OctTerm> term(nl);
    std::vector<LocalRecord> cloud;
    HostXfer d[6] = {{ks.data(), a.kstar, nl}, {lkey.data(), a.leaf_key, nl * 8}, {start.data(), a.leaf_start, (nl + 1) * 4},
                     {src.data(), a.src[(st.npass - 1u) & 1u], S * 4}, {term.data(), a.term, nl * sizeof(OctTerm)}, {nullptr, nullptr, 0}};
    int nd = 5, rc;
    if (!host_in) { cloud.resize((size_t)a.n); d[nd++] = HostXfer{cloud.data(), const_cast<LocalRecord*>(a.in), (size_t)a.n * kRec}; host_in = cloud.data(); }
    if ((rc = download_arrays(h, d, nd, 0))) return rc;
    struct Ev { uint32_t pos; unsigned long long key; };
    std::vector<Ev> ev;
    ev.reserve(st.fb_points);
    std::vector<uint32_t> leaves;
    for (size_t i = 0; i < nl; ++i) if (ks[i] >= 3) {
        leaves.push_back((uint32_t)i);
        for (uint32_t j = start[i]; j < start[i + 1]; ++j) ev.push_back(Ev{src[j], lkey[i]});
    }
    std::sort(ev.begin(), ev.end(), [](const Ev& x, const Ev& y) { return x.pos < y.pos; });
    Tree tree;
    tree.hit = t.hit; tree.cmin = t.cmin; tree.cmax = t.cmax;
    tree.pool.reserve(ev.size() + leaves.size() * 2 + 64);
    for (const Ev& e : ev) {
        const uint32_t c = host_in[e.pos].bgra;
        tree.insert(e.key, ((c >> 16) & 255u) | (c & 0xff00u) | ((c & 255u) << 16));
    }
    size_t at = 0;
    bool ok = true;
    if (tree.root >= 0) tree.terminals(tree.root, 0, [&](int level, float v, uint32_t col) {
        const size_t span = (size_t)1 << (3 * level);
        uint32_t cnt = 0;
        while (cnt <= t.sat && t.f[cnt] != v) ++cnt;
        if (cnt > t.sat || at + span > leaves.size()) { ok = false; return; }
        term[leaves[at]] = OctTerm{col | (uint32_t)level << 24, cnt};
        for (size_t k = 1; k < span; ++k) term[leaves[at + k]] = OctTerm{kOctWhite | kOctDead << 24, 0u};
        at += span;
    });
    if (!ok || at != leaves.size()) return fail(h, GEM_ERR_HIP, "gem_octree_build: the host blocks do not match the device's leaves");
    HostXfer u{term.data(), a.term, nl * sizeof(OctTerm)};
    return upload_arrays(h, &u, 1);
}

// d_in: n records on the device; host_in: the same on the host, or NULL
int build(gem_handle* h, int slot, const gem_octree_params* q, const Tables& t, const LocalRecord* d_in, const LocalRecord* host_in,
          long long n, gem_octree_stats* stats)
{
    auto& oc = h->octree;
    auto& sl = oc.slot[slot];
    gem_octree_stats s{};
    s.points_in = n;
    if (n == 0) { sl.bytes = 0; sl.stats = s; if (stats) *stats = s; return GEM_OK; }
    int rc;
    const long long nb = oct_blocks(n), cap = oct_max_nodes(n);
    const size_t state_cap = oc.state.cap, hist_cap = oc.hist.cap;
    if ((rc = ensure_zeroed(h, oc.state, 256)) || (rc = ensure_zeroed(h, oc.hist, (size_t)nb * kLsdBins * 4 * 2 + 256)) ||
        (rc = ensure(h, oc.tab, kOctTable * 12 + 256)) || (rc = ensure(h, oc.work, work_bytes(n))) ||
        (rc = ensure(h, sl.out, (size_t)cap * 8))) return rc;
    OctState* dst = static_cast<OctState*>(oc.state.p);
    // The kernels leave the tickets, the key accumulators and the histograms as a build needs to find them.  That holds only behind a
    // build that ran to its end, so after one that did not -- and in new arenas -- they are set here.
    if (oc.dirty || oc.state.cap != state_cap || oc.hist.cap != hist_cap) {
        GEM_HIP(h, hipMemsetAsync(oc.state.p, 0, 256, h->stream));
        GEM_HIP(h, hipMemsetAsync(&dst->acc_and, 0xff, 8, h->stream));
        GEM_HIP(h, hipMemsetAsync(oc.hist.p, 0, oc.hist.cap, h->stream));
    }
    oc.dirty = true;
    double* p_tab = static_cast<double*>(oc.tab.p);
    float* f_tab = reinterpret_cast<float*>(p_tab + kOctTable);
    if (oc.tab_key[0] != q->prob_hit || oc.tab_key[1] != q->clamp_min || oc.tab_key[2] != q->clamp_max) {
        HostXfer x[2] = {{const_cast<double*>(t.p), p_tab, sizeof t.p}, {const_cast<float*>(t.f), f_tab, sizeof t.f}};
        oc.tab_key[0] = -1;
        if ((rc = upload_arrays(h, x, 2))) return rc;
        oc.tab_key[0] = q->prob_hit; oc.tab_key[1] = q->clamp_min; oc.tab_key[2] = q->clamp_max;
    }
    OctArgs a{};
    carve(a, static_cast<unsigned char*>(oc.work.p), n);
    a.in = d_in; a.n = n; a.rf = 1.0 / q->resolution; a.sat = t.sat; a.f_tab = f_tab; a.p_tab = p_tab; a.st = dst;
    a.hist[0] = static_cast<uint32_t*>(oc.hist.p); a.hist[1] = a.hist[0] + (size_t)nb * kLsdBins;
    a.out = static_cast<uint2*>(sl.out.p); a.out_cap = cap; a.nb = (int)nb;
    sl.bytes = 0;                                                        // (a failure below leaves the slot empty, not half-written)
    GEM_HIP(h, launch_octree_front(h->stream, a));
    GEM_HIP(h, launch_octree_back(h->stream, a));
    OctState st{};
    { HostXfer c{&st, dst, sizeof st}; if ((rc = download_arrays(h, &c, 1, 0))) return rc; }
    if (st.fb_leaves) {
        if (st.nleaves > (uint32_t)n || st.S > (uint32_t)n) return fail(h, GEM_ERR_HIP, "gem_octree_build: leaf count out of range");
        if ((rc = host_blocks(h, a, st, t, host_in))) return rc;
        GEM_HIP(h, hipMemsetAsync(&dst->n_leaf_nodes, 0, 8, h->stream));
        GEM_HIP(h, launch_octree_back(h->stream, a));
        HostXfer c{&st, dst, sizeof st};
        if ((rc = download_arrays(h, &c, 1, 0))) return rc;
    }
    oc.dirty = false;
    if ((long long)st.nnodes > cap) return fail(h, GEM_ERR_HIP, "gem_octree_build: node count out of range");
    s.points_keyed = st.S; s.leaves_depth16 = st.n_leaf_nodes; s.pruned_leaves = st.n_pruned; s.nodes = st.nnodes; s.bytes = 8ll * st.nnodes;
    s.coupled_blocks[0] = st.nblk[0]; s.coupled_blocks[1] = st.nblk[1]; s.coupled_blocks[2] = st.nblk[2];
    s.fallback_points = st.fb_points;
    sl.bytes = s.bytes; sl.stats = s;
    if (stats) *stats = s;
    return GEM_OK;
}

int check_cloud(gem_handle* h, const char* what, const void* points, long long n)
{
    const std::string w(what);
    if (n < 0 || n > 2147483646ll) return fail(h, GEM_ERR_INVALID, (w + ": n out of range").c_str());
    if (n > 0 && !points) return fail(h, GEM_ERR_INVALID, (w + ": null points").c_str());
    return GEM_OK;
}

} // namespace

namespace gemi {

void octree_free(gem_handle* h)
{
    auto& oc = h->octree;
    for (Arena* a : {&oc.state, &oc.hist, &oc.tab, &oc.in, &oc.work, &oc.slot[0].out, &oc.slot[1].out, &oc.slot[2].out, &oc.slot[3].out}) {
        if (a->p) hipFree(a->p);
        a->p = nullptr; a->cap = 0;
    }
    oc = gem_handle::Octree{};
}

} // namespace gemi

extern "C" {

int gem_octree_build(gem_handle* h, int slot, const gem_octree_params* params, const void* points, long long n, gem_octree_stats* stats)
{
    GEM_ENTRY("gem_octree_build");
    int rc;
    Tables t;
    if ((rc = check_common(h, slot, "gem_octree_build")) || (rc = check_cloud(h, "gem_octree_build", points, n))) return rc;
    if (!make_tables(params, t)) return fail(h, GEM_ERR_INVALID, "gem_octree_build: parameters (resolution, prob_hit, clamps)");
    if (n > 0) {
        if ((rc = ensure(h, h->octree.in, (size_t)n * kRec))) return rc;
        HostXfer x{const_cast<void*>(points), h->octree.in.p, (size_t)n * kRec};
        if ((rc = upload_arrays(h, &x, 1))) return rc;
    }
    return build(h, slot, params, t, static_cast<const LocalRecord*>(h->octree.in.p), static_cast<const LocalRecord*>(points), n, stats);
}

int gem_octree_build_device(gem_handle* h, int slot, const gem_octree_params* params, const void* d_points, long long n, gem_octree_stats* stats)
{
    GEM_ENTRY("gem_octree_build_device");
    int rc;
    Tables t;
    if ((rc = check_common(h, slot, "gem_octree_build_device")) || (rc = check_cloud(h, "gem_octree_build_device", d_points, n))) return rc;
    if (!make_tables(params, t)) return fail(h, GEM_ERR_INVALID, "gem_octree_build_device: parameters (resolution, prob_hit, clamps)");
    return build(h, slot, params, t, static_cast<const LocalRecord*>(d_points), nullptr, n, stats);
}

int gem_local_compose_octrees(gem_handle* h, const gem_compose_params* p, const gem_octree_params* road_params,
                              const gem_octree_params* obstacle_params, int out_counts[3], double* out_threshold, gem_octree_stats stats[2])
{
    GEM_ENTRY("gem_local_compose_octrees");
    int rc;
    Tables tr, to;
    if ((rc = compose_check(h, p, "gem_local_compose_octrees"))) return rc;
    if (!make_tables(road_params, tr) || !make_tables(obstacle_params, to))
        return fail(h, GEM_ERR_INVALID, "gem_local_compose_octrees: octree parameters (resolution, prob_hit, clamps)");
    uint32_t tot[3] = {0, 0, 0};
    double thr = 0.0;
    if ((rc = compose_split(h, p, true, true, tot, &thr))) return rc;
    auto& cp = h->compose;
    if ((rc = build(h, GEM_OCTREE_ROAD, road_params, tr, static_cast<const LocalRecord*>(cp.road.p), nullptr, tot[0], stats ? &stats[0] : nullptr)) ||
        (rc = build(h, GEM_OCTREE_OBSTACLE, obstacle_params, to, static_cast<const LocalRecord*>(cp.obstacle.p), nullptr, tot[1], stats ? &stats[1] : nullptr)))
        return rc;
    if (out_counts) { out_counts[0] = (int)tot[0]; out_counts[1] = (int)tot[1]; out_counts[2] = (int)tot[2]; }
    if (out_threshold) *out_threshold = thr;
    return GEM_OK;
}

int gem_octree_read(gem_handle* h, int slot, void* data, size_t capacity, size_t* out_bytes)
{
    GEM_ENTRY("gem_octree_read");
    int rc;
    if ((rc = check_common(h, slot, "gem_octree_read"))) return rc;
    const auto& sl = h->octree.slot[slot];
    const size_t bytes = (size_t)sl.bytes;
    if (out_bytes) *out_bytes = bytes;
    if (!data) return GEM_OK;
    if (capacity < bytes) return fail(h, GEM_ERR_INVALID, "gem_octree_read: capacity below the stream's size");
    if (!bytes) return GEM_OK;
    HostXfer d{data, sl.out.p, bytes};
    return download_arrays(h, &d, 1, 0);
}

} // extern "C"
