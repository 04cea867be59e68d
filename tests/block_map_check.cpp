// block_map_check.cpp -- CPU check of the division-free XCD-band block map (csrc/rt_kparams.h):
// xcd_band_block with the host's udiv_magic(chunk) and xcd_band_full(nb, chunk) against the formula it replaced
// (two runtime divisions per wave), for every block of every launch size listed below; and that the map is a
// bijection on [0, nb).
//   g++ -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM/include tests/block_map_check.cpp -o block_map_check
#include "../cpp-11-ray-trace-march-framework_amd/csrc/rt_kparams.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

namespace {

// the map as the render kernels computed it before (rt_kernels.hip, xcd_band_block(b, nb, chunk))
uint32_t old_band_block(uint32_t b, uint32_t nb, uint32_t chunk)
{
    constexpr uint32_t kXcds = rtk::kXcds;
    if (chunk == 0u)
    {
        const uint32_t q = nb / kXcds, r = nb % kXcds;
        const uint32_t x = b % kXcds, i = b / kXcds;
        return x < r ? x * (q + 1u) + i : r * (q + 1u) + (x - r) * q + i;
    }
    const uint32_t full = nb / (kXcds * chunk) * (kXcds * chunk);
    if (b >= full) return b;
    const uint32_t x = b % kXcds, i = b / kXcds;
    const uint32_t row = (i / chunk) * kXcds + x;
    return row * chunk + i % chunk;
}

unsigned long long cases = 0, mismatches = 0, full_bad = 0, launches = 0, not_bijective = 0, remapped = 0;
std::vector<uint8_t> seen;

void one_launch(uint32_t nb, uint32_t chunk)
{
    const uint32_t m = rtk::udiv_magic(chunk), full = rtk::xcd_band_full(nb, chunk);
    launches++;
    if (chunk != 0u) full_bad += full != nb / (8u * chunk) * (8u * chunk);
    seen.assign(nb, 0);
    bool bij = true;
    for (uint32_t b = 0; b < nb; b++)
    {
        const uint32_t got = rtk::xcd_band_block(b, nb, chunk, m, full);
        cases++;
        mismatches += got != old_band_block(b, nb, chunk);
        if (got >= nb || seen[got]) bij = false;
        else seen[got] = 1;
    }
    not_bijective += !bij;
}

}  // namespace

int main()
{
    // every launch of 1 .. 3,000 blocks at turn sizes around the cases of the map: one band per XCD (0), one block,
    // a few, one tile row of the bench frame at 1 to 16 samples (120 x 4 = 480) and beside it, a frame 65,536 wide
    for (uint32_t chunk : { 0u, 1u, 2u, 3u, 4u, 7u, 12u, 28u, 36u, 480u, 481u, 4096u })
        for (uint32_t nb = 1; nb <= 3000; nb++) one_launch(nb, chunk);
    const unsigned long long listed = launches;
    // random launches: nb < 2^22 blocks, chunk < 2^16
    std::mt19937_64 g(20261020);
    for (int i = 0; i < 20000; i++)
    {
        // (mostly small launches, so that 20,000 of them stay a matter of seconds; every 64th over the whole range)
        const uint32_t nb_bits = i % 64 == 0 ? 22u : 1u + uint32_t(g() % 14u);
        const uint32_t nb = 1u + uint32_t(g() % ((1ull << nb_bits) - 1ull));
        // chunk < 2^16: every other launch draws it from [1, nb / 8], so that 8 chunk <= nb and the launch has whole
        // rounds to remap (with nb mostly below 2^14 an unweighted chunk leaves `full` 0 and the map the identity)
        uint32_t chunk = uint32_t(g() % 65536ull) >> (g() % 16u);
        if (i % 2 == 0 && nb >= 8u) chunk = 1u + uint32_t(g() % std::min<uint64_t>(nb / 8u, 65535ull));
        remapped += chunk != 0u && rtk::xcd_band_full(nb, chunk) != 0u;
        one_launch(nb, chunk);
    }
    std::printf("{\"listed_launches\": %llu, \"random_launches\": %llu, \"cases\": %llu, \"mismatches\": %llu, "
                "\"full_mismatches\": %llu, \"not_bijective\": %llu, \"random_with_whole_rounds\": %llu}\n",
                listed, launches - listed, cases, mismatches, full_bad, not_bijective, remapped);
    return 0;
}
