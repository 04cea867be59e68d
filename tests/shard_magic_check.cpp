// shard_magic_check.cpp -- CPU check of the division-free tile coordinates of process_item (csrc/rt_kparams.h,
// DESIGN.md §4.28): udiv_by_magic against t / d and t % d, shard_tile_xy_m against shard_tile_xy.
//   g++ -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM/include tests/shard_magic_check.cpp -o shard_magic_check
#include "../cpp-11-ray-trace-march-framework_amd/csrc/rt_kparams.h"

#include <cstdio>
#include <random>

int main()
{
    std::mt19937_64 g(20261019);
    unsigned long long div_cases = 0, div_bad = 0, deal_cases = 0, deal_bad = 0;
    auto one = [&](uint32_t t, uint32_t d) {
        uint32_t rem;
        const uint32_t q = rtk::udiv_by_magic(t, d, rtk::udiv_magic(d), rem);
        div_cases++;
        div_bad += q != t / d || rem != t % d;
    };
    // every divisor a frame can have (1 .. 4096 tiles across: 65536 pixels) against dividends at the edges of
    // every quotient step and of the 32-bit range, then random pairs over the whole range
    const uint32_t edge[] = { 0u, 1u, 2u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu };
    for (uint32_t d = 1; d <= 4096; d++)
    {
        for (uint32_t t : edge) one(t, d);
        for (int k = 0; k < 64; k++)
        {
            const uint32_t q = uint32_t(g() % (0xFFFFFFFFull / d + 1ull));
            const uint64_t b = uint64_t(q) * d;
            for (int o = -1; o <= 1; o++)
                if (b + o >= 0 && b + uint64_t(o + 1) <= 0x100000000ull && !(b == 0 && o < 0)) one(uint32_t(b + o), d);
        }
    }
    for (int i = 0; i < 4000000; i++)
    {
        const uint32_t d = uint32_t(g()) >> (g() % 32);
        one(uint32_t(g()), d ? d : 1u);
    }
    // the shard deal: every tile of frames up to 4096 tiles across, ranks 1 .. 9
    for (uint32_t tiles_x : { 1u, 2u, 3u, 7u, 8u, 16u, 120u, 121u, 255u, 256u, 1000u, 4095u, 4096u })
        for (uint32_t nranks = 1; nranks <= 9; nranks++)
            for (uint32_t rank = 0; rank < nranks; rank += (nranks > 3 ? nranks - 1 : 1))
            {
                const uint32_t m = rtk::udiv_magic(tiles_x);
                const uint32_t ntiles = tiles_x * (tiles_x > 1000u ? 64u : 70u);
                for (uint32_t k = 0; rank + k * nranks < ntiles; k++)
                {
                    uint32_t ax, ay, bx, by;
                    rtk::shard_tile_xy(k, rank, nranks, tiles_x, ax, ay);
                    rtk::shard_tile_xy_m(k, rank, nranks, tiles_x, m, bx, by);
                    deal_cases++;
                    deal_bad += ax != bx || ay != by;
                }
            }
    std::printf("{\"div_cases\": %llu, \"div_mismatches\": %llu, \"deal_cases\": %llu, \"deal_mismatches\": %llu}\n",
                div_cases, div_bad, deal_cases, deal_bad);
    return 0;
}
