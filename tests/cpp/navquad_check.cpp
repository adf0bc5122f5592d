// gem_amd/csrc/gem_navquad.hpp on its own, compiled by the host compiler: the quotient the kernel and the host twin compute without a
// divide.  Prints, for every weight hf = 1 .. 462, one line "hf q(0) q(1) ... q(hf - 1)" -- navquad_quot for every dc below hf -- then
// a line "inc hf i(0) ... i(hf)" with navquad_inc for dc = 0 .. hf; the test compares both with Python's integer floor.  It checks the
// quotient against a 64-bit divide itself as well, so a failure names the pair.
#include "../../gem_amd/csrc/gem_navquad.hpp"

#include <cstdio>

int main()
{
    int fails = 0;
    for (int hf = 1; hf <= gem::kNavQuadMaxWeight; ++hf) {
        const unsigned word = gem::navquad_word(hf);
        if ((int)(word & gem::kNavQuadHfMask) != hf) { std::printf("FAIL word %d\n", hf); ++fails; }
        std::printf("%d", hf);
        for (int dc = 0; dc < hf; ++dc) {
            const int q = gem::navquad_quot(word, (unsigned)dc);
            const long long num = -2301ll * dc * dc + 5307ll * dc * hf + 7040ll * hf * hf, den = 10000ll * hf;
            if (num < 0 || num >= (1ll << 31) || q != (int)(num / den)) { std::printf("\nFAIL hf %d dc %d: %d, not %lld\n", hf, dc, q, num / den); ++fails; }
            std::printf(" %d", q);
        }
        std::printf("\ninc %d", hf);
        for (int dc = 0; dc <= hf; ++dc) std::printf(" %d", gem::navquad_inc(word, (unsigned)dc));
        std::printf("\n");
    }
    if (gem::navquad_word(0) != 0u || gem::navquad_update(0u, 0, 0, 0, 0) != gem::kNavUnreached) { std::printf("FAIL impassable\n"); ++fails; }
    std::printf(fails ? "FAILED\n" : "OK\n");
    return fails ? 1 : 0;
}
