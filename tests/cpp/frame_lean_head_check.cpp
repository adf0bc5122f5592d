// Host-only check of the head of a lean launch (gem_amd/csrc/gem_frame_lean.hpp: FrameLeanHead, frame_lean_head; built with
// hipcc --offload-host-only, run by tests/test_frame_preload.py): a block filled with a distinct value per field, every word of the
// head compared with the block's field, no word of the head left zero.  Prints "head dwords N": the count the kernels'
// preload length is compared with.
#include "../../gem_amd/csrc/gem_frame_lean.hpp"

#include <cstdio>
#include <cstring>

using namespace gem;

static int fails = 0;
#define SAME(x, y) do { if (!((x) == (y))) { ++fails; std::printf("FAIL %s:%d %s != %s\n", __FILE__, __LINE__, #x, #y); } } while (0)

template <class P> static P fake_ptr(uintptr_t v) { return reinterpret_cast<P>((v << 40) | (v << 8)); }

int main()
{
    FrameLeanArgs la{};
    uint32_t w[sizeof(FrameLeanArgs) / 4];
    for (size_t i = 0; i < sizeof(FrameLeanArgs) / 4; ++i) w[i] = 0x01010000u + (uint32_t)i * 0x10001u;   // every word of the block its own value
    std::memcpy(&la, w, sizeof la);
    // ... and the fields the head copies once more by name, each its own value
    uint32_t v = 500;
    la.t.nf = (int)++v; la.t.T = (int)++v; la.t.tiles_per_row = (int)++v; la.t.tile_div = ++v; la.t.center_tr = (int)++v; la.t.center_tc = (int)++v;
    la.t.bkt = fake_ptr<const uint32_t*>(++v); la.t.bcount = fake_ptr<uint32_t*>(++v);
    la.b.xyzi = fake_ptr<const float4*>(++v); la.b.B = (int)++v; la.b.n = ++v;
    la.b.bkt = fake_ptr<uint32_t*>(++v); la.b.bcount = fake_ptr<uint32_t*>(++v); la.b.tiles_per_row = (int)++v;   // the binning half's namesakes are not the head's

    const FrameLeanHead h = frame_lean_head(la);
    SAME(h.nf, la.t.nf); SAME(h.T, la.t.T); SAME(h.tiles_per_row, la.t.tiles_per_row); SAME(h.tile_div, la.t.tile_div);
    SAME(h.center_tr, la.t.center_tr); SAME(h.center_tc, la.t.center_tc); SAME(h.bkt, la.t.bkt); SAME(h.bcount, la.t.bcount);
    SAME(h.xyzi, la.b.xyzi); SAME(h.B, la.b.B); SAME(h.n, la.b.n);
    // the eleven fields above are the whole head: 14 dwords without padding, none of them zero, no two 32-bit fields equal
    static_assert(sizeof(FrameLeanHead) == 6 * 4 + 3 * 8 + 2 * 4 && kFrameHeadDwords == 14, "the head's layout");
    uint32_t hw[kFrameHeadDwords];
    std::memcpy(hw, &h, sizeof h);
    for (int i = 0; i < kFrameHeadDwords; ++i)
        if (hw[i] == 0) { ++fails; std::printf("FAIL word %d of the head was not filled\n", i); }
    const int ints[] = {h.nf, h.T, h.tiles_per_row, (int)h.tile_div, h.center_tr, h.center_tc, h.B, (int)h.n};
    for (int i = 0; i < 8; ++i) for (int j = i + 1; j < 8; ++j) if (ints[i] == ints[j]) { ++fails; std::printf("FAIL fields %d and %d hold the same value\n", i, j); }
    // the filled head of a real launch: frame_lean_args' block
    FuseArgs fa{}; BinArgs ba{};
    fa.T = 1000; fa.tiles_per_row = 38; fa.center_tr = 37; fa.center_tc = 3; fa.bkt = fake_ptr<const uint32_t*>(7); fa.bcount = fake_ptr<uint32_t*>(8);
    ba.xyzi = fake_ptr<const float4*>(9); ba.B = 17; ba.n = 1025; ba.bkt = fake_ptr<uint32_t*>(10); ba.bcount = fake_ptr<uint32_t*>(11);
    const FrameLeanHead g = frame_lean_head(frame_lean_args(fa, ba));
    SAME(g.nf, 1024); SAME(g.T, 1000); SAME(g.tiles_per_row, 38); SAME(g.tile_div, frame_div_mul(38)); SAME(g.center_tr, 37); SAME(g.center_tc, 3);
    SAME(g.bkt, fa.bkt); SAME(g.bcount, fa.bcount); SAME(g.xyzi, ba.xyzi); SAME(g.B, 17); SAME(g.n, 1025u);

    std::printf("head dwords %d\n", kFrameHeadDwords);
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
