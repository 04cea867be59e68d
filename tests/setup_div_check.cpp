// setup_div_check.cpp -- CPU check of the DDA setup's quotients (csrc/rt_setup_div.h):
// the header librt_tracer.so runs (setup_div_operand_ok, setup_div) against the IEEE n / d, bit for bit.
//   g++ -O2 -std=c++17 -pthread -ffp-contract=off tests/setup_div_check.cpp -o setup_div_check
//   setup_div_check scene data/scenes/scene8.rtscene 1920 1080 4 16      every 16th tile of the frame
//   setup_div_check families 20261019 10000000                           seeded families, pairs each
// The reciprocal is 1.0f / d, which the device's rtd::rcp_nr equals wherever the window admits d
// (rt_debug_rcp_check).  A pair inside the window must give n / d's bits; a pair outside must report the
// fall-back (lane_quotient: the decision of one lane of dda_setup's vote).
#include "../oracle/cpu_tracer.cpp"
#include "../cpp-11-ray-trace-march-framework_amd/csrc/rt_setup_div.h"

#include <atomic>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

namespace {

uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
float from_bits(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }

struct Acc
{
    uint64_t pairs = 0, fast = 0, fallback = 0, mismatches = 0;
    uint64_t outside_would_differ = 0;      // information: pairs outside the window where the fast form differs
    uint64_t window_errors = 0;             // the lane's decision disagrees with the window as documented
    void add(const Acc& o)
    {
        pairs += o.pairs; fast += o.fast; fallback += o.fallback; mismatches += o.mismatches;
        outside_would_differ += o.outside_would_differ; window_errors += o.window_errors;
    }
};

// the window of rt_setup_div.h, restated independently on the bit patterns: 2^-40 <= |x| <= 2^40
bool in_window_bits(float x)
{
    const uint32_t a = bits(x) & 0x7FFFFFFFu;
    return a >= bits(0x1p-40f) && a <= bits(0x1p40f);
}

// one lane of dda_setup: the fast quotient inside the window, the division outside
float lane_quotient(float n, float d, bool& fast)
{
    fast = rtk::setup_div_operand_ok(n) && rtk::setup_div_operand_ok(d);
    return fast ? rtk::setup_div(n, d, 1.0f / d) : n / d;
}

void check(Acc& a, float n, float d)
{
    bool fast;
    const float q = lane_quotient(n, d, fast);
    const float ref = n / d;
    a.pairs++;
    if (fast != (in_window_bits(n) && in_window_bits(d))) a.window_errors++;
    if (fast)
    {
        a.fast++;
        if (bits(q) != bits(ref)) a.mismatches++;
    }
    else
    {
        a.fallback++;
        const float f = rtk::setup_div(n, d, 1.0f / d);
        if (bits(f) != bits(ref) && !(f != f && ref != ref)) a.outside_would_differ++;
    }
}

void print_acc(const char *name, const Acc& a, const char *tail)
{
    std::printf("\"%s\": {\"pairs\": %llu, \"fast\": %llu, \"fallback\": %llu, \"mismatches\": %llu, "
                "\"window_errors\": %llu, \"outside_would_differ\": %llu}%s",
                name, (unsigned long long)a.pairs, (unsigned long long)a.fast, (unsigned long long)a.fallback,
                (unsigned long long)a.mismatches, (unsigned long long)a.window_errors,
                (unsigned long long)a.outside_would_differ, tail);
}

// ---------------------------------------------------------------------------------- scene mode
uint32_t compact_bits(uint32_t v)
{
    v &= 0x55u; v = (v | (v >> 1)) & 0x33u; v = (v | (v >> 2)) & 0x0Fu; return v;
}

// the (n, d) pairs of one ray's setup (grid.cpp:174-216, as rt_walk.h dda_setup forms them)
void ray_pairs(const Scene& s, const V3& o, const V3& d, Acc& a, uint64_t& rays_in)
{
    float enter_t, leave_t;
    V3 g;
    if (PointAABB(o, s.aabb_min, s.aabb_max)) { enter_t = 0.0f; g = o; }
    else if (RayAABB(o, d, s.aabb_min, s.aabb_max, enter_t, leave_t))
        g = mk(o.x + d.x * enter_t, o.y + d.y * enter_t, o.z + d.z * enter_t);
    else return;
    rays_in++;
    for (int ax = 0; ax < 3; ax++)
    {
        const int pos = s.ToVoxel(g, ax);
        const float da = comp(d, ax);
        if (da == 0.0f) continue;
        if (da > 0.0f)
        {
            check(a, s.ToPos(pos + 1, ax) - comp(g, ax), da);
            check(a, s.cell_wdh, da);
        }
        else
        {
            check(a, s.ToPos(pos, ax) - comp(g, ax), da);
            check(a, -s.cell_wdh, da);
        }
    }
}

int scene_mode(int argc, char **argv)
{
    if (argc < 7) { std::fprintf(stderr, "usage: setup_div_check scene file.rtscene W H spp tile_stride\n"); return 2; }
    Scene s;
    if (!ReadScene(argv[2], s)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
    BuildGrid(s, 64);
    const uint32_t W = std::atoi(argv[3]), H = std::atoi(argv[4]), spp = std::atoi(argv[5]);
    const uint32_t stride = std::max(1, std::atoi(argv[6]));
    const std::vector<float> smp = Hammersley(spp);
    const uint32_t tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16;
    std::vector<uint32_t> tiles;
    for (uint32_t t = 0; t < tiles_x * tiles_y; t += stride) tiles.push_back(t);
    const uint32_t nth = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<Acc> acc(nth);
    std::vector<uint64_t> rays(nth, 0);
    std::atomic<uint32_t> next(0);
    std::vector<std::thread> pool;
    for (uint32_t th = 0; th < nth; th++)
        pool.emplace_back([&, th]() {
            for (;;)
            {
                const uint32_t i = next.fetch_add(1);
                if (i >= tiles.size()) break;
                const uint32_t tx0 = (tiles[i] % tiles_x) * 16, ty0 = (tiles[i] / tiles_x) * 16;
                for (uint32_t p = 0; p < 256; p++)
                {
                    const uint32_t x = tx0 + compact_bits(p), y = ty0 + compact_bits(p >> 1);
                    if (x >= W || y >= H) continue;
                    for (uint32_t si = 0; si < spp; si++)
                    {
                        V3 o, d;
                        GenRay(s.cam, x, y, W, H, smp[2 * si], smp[2 * si + 1], s.fov, o, d);
                        ray_pairs(s, o, d, acc[th], rays[th]);
                    }
                }
            }
        });
    for (auto& t : pool) t.join();
    Acc a;
    uint64_t r = 0;
    for (uint32_t th = 0; th < nth; th++) { a.add(acc[th]); r += rays[th]; }
    std::printf("{\"mode\": \"scene\", \"tiles\": %u, \"rays_in_grid\": %llu, ", uint32_t(tiles.size()), (unsigned long long)r);
    print_acc("setup", a, "}\n");
    return 0;
}

// ------------------------------------------------------------------------------- families mode
typedef std::mt19937_64 Rng;
uint32_t urand(Rng& g, uint32_t a, uint32_t b) { return a + uint32_t(g() % uint64_t(b - a + 1)); }
int irand(Rng& g, int a, int b) { return a + int(g() % uint64_t(b - a + 1)); }
float sgn(Rng& g) { return (g() & 1) ? 1.0f : -1.0f; }
// a float of random sign and mantissa with binary exponent in [elo, ehi] (normal range)
float rand_float(Rng& g, int elo, int ehi)
{
    return from_bits((uint32_t(g() & 1) << 31) | (uint32_t(irand(g, elo, ehi) + 127) << 23) | (uint32_t(g()) & 0x7FFFFFu));
}
float nudge(float x, int ulps)
{
    for (int i = 0; i < (ulps < 0 ? -ulps : ulps); i++) x = std::nextafterf(x, ulps < 0 ? -INFINITY : INFINITY);
    return x;
}

int families_mode(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: setup_div_check families seed pairs_per_family\n"); return 2; }
    Rng g(std::strtoull(argv[2], nullptr, 0));
    const uint64_t N = std::strtoull(argv[3], nullptr, 0);
    // exponents of operands meant to lie inside the window, with room for the quotient's construction
    const int E = 39;
    std::printf("{\"mode\": \"families\", \"families\": {\n  ");
    {   // d with an all-ones mantissa (1 / d rounds up to just above a power of two)
        Acc a;
        for (uint64_t i = 0; i < N; i++)
        {
            const float d = from_bits((uint32_t(g() & 1) << 31) | (uint32_t(irand(g, -E, E) + 127) << 23) | 0x7FFFFFu);
            check(a, rand_float(g, -E, E), d);
        }
        print_acc("d_all_ones_mantissa", a, ",\n  ");
    }
    {   // d a power of two (the reciprocal is exact)
        Acc a;
        for (uint64_t i = 0; i < N; i++) check(a, rand_float(g, -E, E), sgn(g) * std::ldexp(1.0f, irand(g, -E - 1, E + 1)));
        print_acc("d_power_of_two", a, ",\n  ");
    }
    {   // n an exact multiple of d (12-bit d, multiplier below 2^12: the product is exact, the quotient a float)
        Acc a;
        for (uint64_t i = 0; i < N; i++)
        {
            const float d = sgn(g) * std::ldexp(float(urand(g, 1, 4095)), irand(g, -40, 20));
            const float n = d * (sgn(g) * float(urand(g, 1, 4095)));
            check(a, n, d);
        }
        print_acc("n_multiple_of_d", a, ",\n  ");
    }
    {   // quotients within 2 ulp of a binade edge: n = fl(q d) for q = 2^k nudged by -2 .. 2 ulp, then n +- 1 ulp
        Acc a;
        for (uint64_t i = 0; i < N; i++)
        {
            const float d = rand_float(g, -19, 19);
            const float q = nudge(std::ldexp(1.0f, irand(g, -19, 19)), irand(g, -2, 2));
            const float n = nudge(float(double(q) * double(d)), irand(g, -1, 1));
            check(a, sgn(g) * n, d);
        }
        print_acc("quotient_near_binade_edge", a, ",\n  ");
    }
    {   // quotients within 2^-24 (relative) of a rounding midpoint: n = fl((q + ulp(q) / 2) d), constructed from d
        Acc a;
        for (uint64_t i = 0; i < N; i++)
        {
            const float d = rand_float(g, -19, 19);
            const float q = rand_float(g, -19, 19);
            const double mid = (double(q) + double(std::nextafterf(q, q < 0 ? -INFINITY : INFINITY))) * 0.5;
            const float n = nudge(float(mid * double(d)), irand(g, -1, 1));
            check(a, n, d);
        }
        print_acc("quotient_near_midpoint", a, ",\n  ");
    }
    {   // magnitudes 2^-140 .. 2^127, subnormals included
        Acc a;
        auto any = [&]() {
            const int e = irand(g, -140, 127);
            if (e >= -126) return rand_float(g, e, e);
            return sgn(g) * std::ldexp(float(1.0 + double(g() >> 11) * (1.0 / 9007199254740992.0)), e);   // subnormal
        };
        for (uint64_t i = 0; i < N; i++) check(a, any(), any());
        print_acc("magnitudes_2^-140_to_2^127", a, ",\n  ");
    }
    {   // pairs that straddle the window's edges on both sides (one operand within 3 ulp of 2^-40 or 2^40),
        // with zeros, infinities and NaN mixed in
        Acc a;
        for (uint64_t i = 0; i < N; i++)
        {
            const float edge = nudge((g() & 1) ? rtk::kSetupDivLo : rtk::kSetupDivHi, irand(g, -3, 3)) * sgn(g);
            float other = rand_float(g, -45, 45);
            const uint32_t k = urand(g, 0, 63);
            if (k == 0) other = 0.0f; else if (k == 1) other = -0.0f; else if (k == 2) other = INFINITY;
            else if (k == 3) other = -INFINITY; else if (k == 4) other = NAN;
            else if (k < 16) other = nudge((g() & 1) ? rtk::kSetupDivLo : rtk::kSetupDivHi, irand(g, -3, 3)) * sgn(g);
            if (g() & 1) check(a, edge, other); else check(a, other, edge);
        }
        print_acc("window_straddle", a, "\n");
    }
    std::printf("}}\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && std::string(argv[1]) == "scene") return scene_mode(argc, argv);
    if (argc >= 2 && std::string(argv[1]) == "families") return families_mode(argc, argv);
    std::fprintf(stderr, "usage: setup_div_check scene|families ...\n");
    return 2;
}
