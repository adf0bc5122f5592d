// frame_pair_check.cpp -- the hold / pair / flush decision of k_frame's stream of sweeps (gem_amd/csrc/gem_frame_pair.hpp) against a
// plain model, host only: every sequence of up to 8 events -- a pairable add, an add that may not share a launch, a flush.
// The model keeps the sweeps by number: which launches follow an event, and which sweeps each one fuses and bins.  Checked: every
// sweep is binned exactly once and fused exactly once, sweeps are fused in call order, a sweep is binned before it is fused and
// never by the launch that fuses it, a launch fuses and bins at most two, nothing is held or deferred after a flush, a held sweep
// waits for one call at most, and the policy of the issue: the first two pairable calls behind a flush launch as singles, then
// calls alternate between held and a launch of two.
#include "../../gem_amd/csrc/gem_frame_pair.hpp"

#include <cstdio>
#include <vector>

using namespace gem;

struct Model {
    std::vector<int> deferred;      // sweeps binned and not fused, oldest first
    int held = -1;
    int next = 0;                   // number of the next sweep
    int run = 0;                    // pairable adds since the last flush or non-pairable add
    std::vector<int> binned, fused; // how often each sweep was
    int last_fused = -1;
};

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void run_sequence(const int* ev, int n, long long& pairs, long long& held_flushed)
{
    FramePairState s{};
    Model m;
    for (int k = 0; k < n; ++k) {
        const FrameEvent e = (FrameEvent)ev[k];
        const bool was_held = s.held;
        const FramePairPlan p = frame_pair_step(s, e);
        pairs += p.pairs; held_flushed += p.held_flushed ? 1 : 0;
        int own = -1;
        if (e != kFrameFlush) { own = m.next++; m.binned.push_back(0); m.fused.push_back(0); }
        // the policy, stated independently: what the model expects of this event
        bool expect_hold = false;
        if (e == kFramePairable) { expect_hold = m.held < 0 && m.run >= 2; ++m.run; }
        else m.run = 0;
        CHECK(p.hold == expect_hold, "event %d of the sequence: hold %d, expected %d", k, (int)p.hold, (int)expect_hold);
        CHECK(p.held_flushed == (was_held && e != kFramePairable), "held_flushed");
        if (p.hold) { CHECK(p.n == 0, "a held call launches"); m.held = own; own = -1; }
        for (int l = 0; l < p.n; ++l) {
            const int nf = p.launch[l].fuse, nb = p.launch[l].bin;
            CHECK(nf >= 0 && nf <= 2 && nb >= 0 && nb <= 2 && nf + nb > 0, "launch %d: fuse %d bin %d", l, nf, nb);
            CHECK(nf == (int)m.deferred.size(), "a launch fuses everything deferred: %d of %d", nf, (int)m.deferred.size());
            for (int f : m.deferred) {
                CHECK(m.binned[f] == 1 && m.fused[f] == 0, "sweep %d fused: binned %d fused %d", f, m.binned[f], m.fused[f]);
                CHECK(f == m.last_fused + 1, "sweep %d fused behind %d", f, m.last_fused);
                ++m.fused[f]; m.last_fused = f;
            }
            m.deferred.clear();
            for (int b = 0; b < nb; ++b) {
                int sw;
                if (m.held >= 0) { sw = m.held; m.held = -1; }
                else { sw = own; own = -1; CHECK(l == p.n - 1, "the event's own sweep is binned by its last launch"); }
                CHECK(sw >= 0, "launch %d bins a sweep nobody has", l);
                if (sw < 0) continue;
                CHECK(m.binned[sw] == 0, "sweep %d binned twice", sw);
                ++m.binned[sw];
                m.deferred.push_back(sw);
            }
        }
        CHECK(own < 0, "event %d: the call's sweep was neither held nor binned", k);
        CHECK(s.held == (m.held >= 0) && s.deferred == (int)m.deferred.size(), "state: held %d deferred %d, model %d %d", (int)s.held, s.deferred, (int)(m.held >= 0), (int)m.deferred.size());
        if (e == kFrameFlush) {
            CHECK(!s.held && s.deferred == 0 && s.streak == 0, "something is put off behind a flush");
            for (int i = 0; i < m.next; ++i) CHECK(m.binned[i] == 1 && m.fused[i] == 1, "behind a flush: sweep %d binned %d fused %d", i, m.binned[i], m.fused[i]);
        }
        if (e == kFrameSingle) CHECK(!s.held && s.deferred == 1, "behind an add that may not share a launch: one sweep deferred");
    }
}

int main()
{
    long long sequences = 0, pairs = 0, held_flushed = 0;
    int ev[8];
    for (int n = 1; n <= 8; ++n) {
        long long total = 1;
        for (int i = 0; i < n; ++i) total *= 3;
        for (long long code = 0; code < total; ++code) {
            long long c = code;
            for (int i = 0; i < n; ++i) { ev[i] = (int)(c % 3); c /= 3; }
            run_sequence(ev, n, pairs, held_flushed);
            ++sequences;
        }
    }
    // the issue's table: eight pairable calls and a flush
    {
        FramePairState s{};
        const int want[8][3] = {{0, 1, 0}, {1, 1, 0}, {-1, -1, 1}, {1, 2, 0}, {-1, -1, 1}, {2, 2, 0}, {-1, -1, 1}, {2, 2, 0}};    // fuse, bin, hold
        for (int k = 0; k < 8; ++k) {
            const FramePairPlan p = frame_pair_step(s, kFramePairable);
            if (want[k][2]) CHECK(p.hold && p.n == 0, "call %d is held", k);
            else CHECK(!p.hold && p.n == 1 && p.launch[0].fuse == want[k][0] && p.launch[0].bin == want[k][1], "call %d: fuse %d bin %d", k, p.launch[0].fuse, p.launch[0].bin);
        }
        const FramePairPlan f = frame_pair_step(s, kFrameFlush);
        CHECK(f.n == 1 && f.launch[0].fuse == 2 && f.launch[0].bin == 0 && !f.held_flushed, "the fuse-only launch fuses a pair");
        // the node patterns never pair: add, read; add, add, read
        long long pp = 0;
        for (int r = 0; r < 8; ++r) { pp += frame_pair_step(s, kFramePairable).pairs; pp += frame_pair_step(s, kFrameFlush).pairs; }
        for (int r = 0; r < 8; ++r) { pp += frame_pair_step(s, kFramePairable).pairs; pp += frame_pair_step(s, kFramePairable).pairs; pp += frame_pair_step(s, kFrameFlush).pairs; }
        CHECK(pp == 0, "a node pattern paired");
    }
    printf("sequences %lld pairs %lld held_flushed %lld\n", sequences, pairs, held_flushed);
    CHECK(pairs > 0 && held_flushed > 0, "no sequence paired");
    if (fails) printf("FAILED %d\n", fails);
    else printf("ok\n");
    return fails ? 1 : 0;
}
