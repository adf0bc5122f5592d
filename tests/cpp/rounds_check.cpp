// rounds_check.cpp -- gem_amd/csrc/gem_rounds.hpp on its own (no GPU, no HIP): run_tile_rounds driven by counting lambdas.  What no
// converging kernel can show: the bound of cells + 2 rounds, the cut of the last chunk at it, and that nothing is enqueued behind it;
// besides the order of rounds and closes, the chunk count, and a lambda's non-zero return stopping the loop at once.
#include "../../gem_amd/csrc/gem_rounds.hpp"

#include <cstdio>
#include <vector>

namespace {

int failures = 0;

void check(bool ok, const char* what, int line)
{
    if (ok) return;
    std::printf("line %d: %s\n", line, what);
    ++failures;
}
#define CHECK(cond) check((cond), #cond, __LINE__)

using Ints = std::vector<int>;

// what a run enqueued, in order: the rounds, the round each close saw, the rounds between closes
struct Fake {
    int converge_at_close = 0;          // the close (1-based) that reports converged; 0: never
    int fail_round = -1, fail_close = 0;    // the round / the close (1-based) that returns `code`
    int code = 0;
    Ints rounds, closes, chunk_lens;
    int open = 0;                       // rounds since the last close
    gem::RoundsResult res;
    int rc = 0;

    void run(long long cells, long long chunk)
    {
        res.rounds = -5; res.chunks = -5; res.converged = true;         // (the driver resets them)
        rc = gem::run_tile_rounds(
            cells, chunk,
            [&](int round) -> int {
                rounds.push_back(round);
                ++open;
                return round == fail_round ? code : 0;
            },
            [&](int round, bool& converged) -> int {
                closes.push_back(round);
                chunk_lens.push_back(open);
                open = 0;
                if ((int)closes.size() == fail_close) return code;
                converged = (int)closes.size() == converge_at_close;
                return 0;
            },
            res);
    }
};

Ints iota(int n)
{
    Ints v;
    for (int i = 0; i < n; ++i) v.push_back(i);
    return v;
}

} // namespace

int main()
{
    {   // convergence at the close of the third chunk
        Fake f;
        f.converge_at_close = 3;
        f.run(1000, 4);
        CHECK(f.rc == 0 && f.res.converged && f.res.chunks == 3 && f.res.rounds == 12);
        CHECK(f.rounds == iota(12));
        CHECK((f.closes == Ints{4, 8, 12}));
        CHECK((f.chunk_lens == Ints{4, 4, 4}));
    }
    {   // ... at the first close
        Fake f;
        f.converge_at_close = 1;
        f.run(1000, 4);
        CHECK(f.rc == 0 && f.res.converged && f.res.chunks == 1 && f.res.rounds == 4);
        CHECK(f.rounds == iota(4) && (f.closes == Ints{4}));
    }
    {   // never: cells = 10, the bound of 12 rounds is a whole number of chunks
        Fake f;
        f.run(10, 4);
        CHECK(f.rc == 0 && !f.res.converged && f.res.chunks == 3 && f.res.rounds == 12);
        CHECK(f.rounds == iota(12));
        CHECK((f.chunk_lens == Ints{4, 4, 4}) && (f.closes == Ints{4, 8, 12}));
    }
    {   // never: cells = 9, the last chunk is cut at 11 rounds and no round number reaches cells + 2
        Fake f;
        f.run(9, 4);
        CHECK(f.rc == 0 && !f.res.converged && f.res.chunks == 3 && f.res.rounds == 11);
        CHECK(f.rounds == iota(11));
        for (int r : f.rounds) CHECK(r < 9 + 2);
        CHECK((f.chunk_lens == Ints{4, 4, 3}) && (f.closes == Ints{4, 8, 11}));
    }
    {   // a chunk longer than the bound: one chunk of cells + 2 = 5 rounds
        Fake f;
        f.run(3, 100);
        CHECK(f.rc == 0 && !f.res.converged && f.res.chunks == 1 && f.res.rounds == 5);
        CHECK(f.rounds == iota(5) && (f.chunk_lens == Ints{5}) && (f.closes == Ints{5}));
    }
    {   // ... that converges at its close
        Fake f;
        f.converge_at_close = 1;
        f.run(3, 100);
        CHECK(f.rc == 0 && f.res.converged && f.res.chunks == 1 && f.rounds == iota(5));
    }
    {   // a round's non-zero return stops the loop at once and is returned: nothing behind round 5, no second close
        Fake f;
        f.converge_at_close = 3; f.fail_round = 5; f.code = 77;
        f.run(1000, 4);
        CHECK(f.rc == 77 && !f.res.converged && f.res.chunks == 1);
        CHECK(f.rounds == iota(6) && (f.closes == Ints{4}));
    }
    {   // a close's non-zero return likewise: no round behind the second close
        Fake f;
        f.converge_at_close = 3; f.fail_close = 2; f.code = -3;
        f.run(1000, 4);
        CHECK(f.rc == -3 && !f.res.converged && f.res.chunks == 1);
        CHECK(f.rounds == iota(8) && (f.closes == Ints{4, 8}));
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
