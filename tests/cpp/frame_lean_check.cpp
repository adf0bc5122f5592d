// Host-only checks of gem_amd/csrc/gem_frame_lean.hpp (built with hipcc --offload-host-only, run by tests/test_frame_lean_args.py):
//   1. the multiply-high division of the lean form's block -> tile map equals `/` for every tiles_per_row in 1..256 and every
//      rank below tiles_per_row^2 + 64;
//   2. with it, frame_tile_of sends blocks [0, nf) onto every tile exactly once -- and onto the tiles the generic form's `/` sends
//      them to -- for tiles_per_row in {1, 2, 5, 7, 10, 38, 64, 150} and centres (0, 0), (tpr / 2, tpr / 2), (tpr - 1, 0);
//   3. frame_lean_args copies every field: FuseArgs / BinArgs filled with a distinct value per field, every field of the block
//      compared, and no word of the block outside its padding left zero.
#include "../../gem_amd/csrc/gem_frame_lean.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace gem;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails <= 20) { std::printf("FAIL %s:%d %s : ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void check_division()
{
    long long n_checked = 0;
    for (int tpr = 1; tpr <= 256; ++tpr) {
        const uint32_t m = frame_div_mul(tpr);
        for (int rnk = 0; rnk < tpr * tpr + 64; ++rnk, ++n_checked) CHECK(frame_div_by(rnk, m) == rnk / tpr, "tpr %d rnk %d", tpr, rnk);
    }
    std::printf("division: %lld (tiles_per_row, rank) pairs\n", n_checked);
}

static void check_tile_map()
{
    const int tprs[] = {1, 2, 5, 7, 10, 38, 64, 150};
    for (int tpr : tprs) {
        const int centres[3][2] = {{0, 0}, {tpr / 2, tpr / 2}, {tpr - 1, 0}};
        for (const auto& c : centres) {
            FuseArgs fa{};
            fa.T = tpr * tpr; fa.tiles_per_row = tpr; fa.center_tr = c[0]; fa.center_tc = c[1]; fa.B_total = 1; fa.U = 64;
            const FrameLeanArgs la = frame_lean_args(fa, BinArgs{});
            CHECK(la.t.nf >= fa.T && la.t.nf % kFrameGridUnit == 0 && la.t.nf - fa.T < kFrameGridUnit, "nf %d T %d", la.t.nf, fa.T);
            std::vector<int> hits((size_t)fa.T, 0);
            int mapped = 0;
            for (int b = 0; b < la.t.nf; ++b) {
                int tr = -1, tc = -1, gr = -1, gc = -1;
                const bool on = frame_tile_of(la.t, b, tr, tc), gen = frame_tile_of(fa, b, gr, gc);
                CHECK(on == gen, "tpr %d block %d", tpr, b);
                if (!on) continue;
                CHECK(tr == gr && tc == gc, "tpr %d block %d: (%d, %d) against (%d, %d)", tpr, b, tr, tc, gr, gc);
                CHECK(tr >= 0 && tr < tpr && tc >= 0 && tc < tpr, "tpr %d block %d: (%d, %d)", tpr, b, tr, tc);
                if (tr >= 0 && tr < tpr && tc >= 0 && tc < tpr) { ++hits[(size_t)tr * tpr + tc]; ++mapped; }
            }
            CHECK(mapped == fa.T, "tpr %d: %d blocks mapped", tpr, mapped);
            for (int t = 0; t < fa.T; ++t) CHECK(hits[(size_t)t] == 1, "tpr %d centre (%d, %d): tile %d taken %d times", tpr, c[0], c[1], t, hits[(size_t)t]);
        }
    }
    std::printf("tile map: 8 sizes x 3 centres\n");
}

template <class P> static P fake_ptr(uintptr_t v) { return reinterpret_cast<P>((v << 40) | (v << 8)); }

static void check_fill()
{
    FuseArgs fa{}; BinArgs ba{};
    uint32_t v = 100;                                                // every source field its own value
    auto nexti = [&] { return (int)++v; };
    auto nextf = [&] { return (float)++v + 0.5f; };
    fa.T = 1000; fa.tiles_per_row = 38; fa.B_total = 7; fa.U = 64;
    fa.dbg = fake_ptr<unsigned long long*>(++v); fa.bkt = fake_ptr<const uint32_t*>(++v); fa.bcount = fake_ptr<uint32_t*>(++v);
    fa.elevation = fake_ptr<float*>(++v); fa.variance = fake_ptr<float*>(++v); fa.lowest = fake_ptr<float*>(++v);
    fa.spill = fake_ptr<uint4*>(++v); fa.ctl = fake_ptr<uint32_t*>(++v); fa.form_seen = fake_ptr<uint32_t*>(++v);
    fa.L = nexti(); fa.center_tr = nexti(); fa.center_tc = nexti(); fa.row0 = nexti(); fa.row1 = nexti(); fa.start0 = nexti(); fa.start1 = nexti();
    fa.n_pending = nexti(); for (int i = 0; i < kMaxPending; ++i) fa.pending[i] = nextf();
    fa.dense = nexti(); fa.mahal = nextf(); fa.var_floor = nextf();
    FrameConst& fc = ba.frame0;
    ba.xyzi = fake_ptr<const float4*>(++v); ba.B = nexti(); ba.n = (long long)nexti();
    ba.keep_sentinel = nexti(); ba.tile_bits = nexti(); ba.tiles_per_row = nexti(); fc.filter_on = nexti();
    ba.bkt = fake_ptr<uint32_t*>(++v); ba.bcount = fake_ptr<uint32_t*>(++v); ba.spill = fake_ptr<uint4*>(++v); ba.ctl = fake_ptr<uint32_t*>(++v);
    ba.dbg = fake_ptr<unsigned long long*>(++v);
    for (int i = 0; i < 12; ++i) fc.T[i] = nextf();
    fc.lower_f = nextf(); fc.upper_f = nextf(); fc.fbx = nextf(); fc.fby = nextf(); fc.fband = nextf(); fc.fplane = nextf();
    fc.cx = nextf(); fc.cy = nextf(); fc.sx = nexti(); fc.sy = nexti(); fc.L = nexti(); fc.res = nextf(); fc.row0 = nexti(); fc.row1 = nexti();
    fc.beam_a = nextf(); fc.beam_c = nextf(); fc.t2 = nextf(); fc.Js[0] = nextf(); fc.Js[1] = nextf();

    const FrameLeanArgs la = frame_lean_args(fa, ba);
    const FrameLeanTile& t = la.t; const FrameLeanBin& b = la.b;
#define SAME(x, y) CHECK((x) == (y), "field differs")
    SAME(t.nf, 1024); SAME(t.T, fa.T); SAME(t.tiles_per_row, fa.tiles_per_row); SAME(t.tile_div, frame_div_mul(38));
    SAME(t.dbg, fa.dbg); SAME(t.bkt, fa.bkt); SAME(t.bcount, fa.bcount); SAME(t.elevation, fa.elevation); SAME(t.variance, fa.variance);
    SAME(t.lowest, fa.lowest); SAME(t.spill, fa.spill); SAME(t.ctl, fa.ctl); SAME(t.form_seen, fa.form_seen);
    SAME(t.L, fa.L); SAME(t.center_tr, fa.center_tr); SAME(t.center_tc, fa.center_tc); SAME(t.row0, fa.row0); SAME(t.row1, fa.row1);
    SAME(t.start0, fa.start0); SAME(t.start1, fa.start1); SAME(t.n_pending, fa.n_pending);
    for (int i = 0; i < kMaxPending; ++i) SAME(t.pending[i], fa.pending[i]);
    SAME(t.dense, fa.dense); SAME(t.mahal, fa.mahal); SAME(t.var_floor, fa.var_floor); SAME(t.nspill, 7u * 64u);
    SAME(b.xyzi, ba.xyzi); SAME(b.B, ba.B); SAME((long long)b.n, ba.n); SAME(b.keep_sentinel, ba.keep_sentinel); SAME(b.tile_bits, ba.tile_bits);
    SAME(b.tiles_per_row, ba.tiles_per_row); SAME(b.filter_on, fc.filter_on);
    SAME(b.bkt, ba.bkt); SAME(b.bcount, ba.bcount); SAME(b.spill, ba.spill); SAME(b.ctl, ba.ctl); SAME(b.dbg, ba.dbg);
    for (int i = 0; i < 12; ++i) SAME(b.T[i], fc.T[i]);
    SAME(b.lower_f, fc.lower_f); SAME(b.upper_f, fc.upper_f); SAME(b.fbx, fc.fbx); SAME(b.fby, fc.fby); SAME(b.fband, fc.fband); SAME(b.fplane, fc.fplane);
    SAME(b.cx, fc.cx); SAME(b.cy, fc.cy); SAME(b.sx, fc.sx); SAME(b.sy, fc.sy); SAME(b.L, fc.L); SAME(b.res, fc.res); SAME(b.row0, fc.row0); SAME(b.row1, fc.row1);
    SAME(b.beam_a, fc.beam_a); SAME(b.beam_c, fc.beam_c); SAME(b.t2, fc.t2); SAME(b.Js[0], fc.Js[0]); SAME(b.Js[1], fc.Js[1]);
#undef SAME
    // no field forgotten by the comparison above either: every word of the block that is not padding holds something
    static_assert(sizeof(FrameLeanTile) == 38 * 4 && sizeof(FrameLeanBin) == 50 * 4 && sizeof(FrameLeanArgs) == 88 * 4, "the block's layout (one word of padding at its end)");
    uint32_t w[sizeof(FrameLeanArgs) / 4];
    std::memcpy(w, &la, sizeof la);
    for (size_t i = 0; i + 1 < sizeof(FrameLeanArgs) / 4; ++i)
        CHECK(w[i] != 0, "word %zu of the block was not filled", i);
    std::printf("fill: %zu bytes\n", sizeof(FrameLeanArgs));
}

int main()
{
    check_division();
    check_tile_map();
    check_fill();
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
