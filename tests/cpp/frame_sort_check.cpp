// Host-only check of gem_amd/csrc/gem_frame_sort.hpp (built with hipcc --offload-host-only, run by tests/test_frame_sized_sort.py):
// the network frame_tile's owner picks by the wave's largest count returns what the full 8-key network returns.
//   For every size N in {2, 4, 8}, every count n from 0 up to the largest count N is picked for (2, 4, 7) and every permutation of
//   n distinct keys padded with ~0u to eight entries: frame_sort_keys<N> over the first N entries == frame_sort_keys<8> over all
//   eight, entry by entry.  Counts below the size class (a lane with fewer records than the wave's largest) are among them.
//   frame_sort_size maps every largest count 1..7 to the size whose network holds it.
#include "../../gem_amd/csrc/gem_frame_sort.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace gem;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails <= 20) { std::printf("FAIL %s:%d %s : ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

template <int N>
static long long check_size(int n_top)
{
    long long checked = 0;
    for (int n = 0; n <= n_top; ++n) {
        // keys as the kernel forms them: point index << 10 | slot, distinct in both parts, not in slot order
        uint32_t live[8];
        for (int i = 0; i < n; ++i) live[i] = ((uint32_t)(1000 + 37 * i) << 10) | (uint32_t)((5 * i + 3) % 8);
        std::sort(live, live + n);
        do {
            uint32_t sized[8], full[8];
            for (int i = 0; i < 8; ++i) sized[i] = full[i] = i < n ? live[i] : 0xffffffffu;
            frame_sort_keys<N>(sized);
            frame_sort_keys<8>(full);
            CHECK(std::memcmp(sized, full, sizeof full) == 0, "size %d, count %d", N, n);
            for (int i = 0; i + 1 < 8; ++i) CHECK(full[i] <= full[i + 1], "the full network itself: entry %d", i);
            ++checked;
        } while (std::next_permutation(live, live + n));
    }
    return checked;
}

int main()
{
    const long long c2 = check_size<2>(2), c4 = check_size<4>(4), c8 = check_size<8>(7);
    std::printf("sizes 2 / 4 / 8: %lld / %lld / %lld permutations\n", c2, c4, c8);
    CHECK(c2 == 1 + 1 + 2 && c4 == 1 + 1 + 2 + 6 + 24 && c8 == 1 + 1 + 2 + 6 + 24 + 120 + 720 + 5040, "permutation counts");
    for (int nmax = 1; nmax <= 7; ++nmax) {
        const int s = frame_sort_size(nmax);
        CHECK((s == 2 || s == 4 || s == 8) && s >= nmax && (s == 2 || s / 2 < nmax), "largest count %d -> size %d", nmax, s);
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
