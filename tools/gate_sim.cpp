// gate_sim.cpp -- analysis only (links the oracle restatement; never part of the product): what the
// record gate (csrc/rt_record_gate.h) would skip in AUTO's wave-uniform record loop.
//   g++ -O2 -std=c++17 -pthread -ffp-contract=off tools/gate_sim.cpp -o /tmp/gate_sim
//   /tmp/gate_sim data/scenes/scene8.rtscene 1920 1080 4
// Waves and lock-step as in tools/wave_sim.cpp.  For every record of every wave-uniform list: the wave's
// vote on ok1 (the first half of the record test, rtd::mt_rec_first) and on the gate, by list length; for
// the gated loop's pairs (list positions 2i, 2i + 1) how many skip entirely; and over every lane test
// (uniform and per-lane lists) the count of ok1-true lanes the gate rejects, which must be 0.
// tests/record_gate_check.cpp is the checked version of the same walk (every 16th tile, in the suite).
#define main record_gate_check_main
#include "../tests/record_gate_check.cpp"
#undef main

namespace {

struct Hist
{
    static constexpr int kB = 9;                    // 1, 2, 3, 4-7, 8-15, 16-31, 32-63, 64-127, 128+
    uint64_t recs[kB] = {}, ok1[kB] = {}, gate[kB] = {};
    uint64_t pairs = 0, pairs_skip = 0, lists = 0, lane_tests = 0, violations = 0, lane_iters = 0, lane_pass = 0;
    static int bucket(uint32_t L) { return L <= 3 ? int(L) - 1 : (L < 8 ? 3 : (L < 16 ? 4 : (L < 32 ? 5 : (L < 64 ? 6 : (L < 128 ? 7 : 8))))); }
    void add(const Hist& o)
    {
        for (int i = 0; i < kB; i++) { recs[i] += o.recs[i]; ok1[i] += o.ok1[i]; gate[i] += o.gate[i]; }
        pairs += o.pairs; pairs_skip += o.pairs_skip; lists += o.lists; lane_tests += o.lane_tests;
        violations += o.violations; lane_iters += o.lane_iters; lane_pass += o.lane_pass;
    }
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 5) { std::fprintf(stderr, "usage: gate_sim scene.rtscene W H spp\n"); return 2; }
    Scene s;
    if (!ReadScene(argv[1], s)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    BuildGrid(s, 64);
    const uint32_t W = std::atoi(argv[2]), H = std::atoi(argv[3]), spp = std::atoi(argv[4]);
    const std::vector<float> smp = Hammersley(spp);
    const uint32_t tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16, items_per_tile = 256 * spp / 64;
    const uint32_t nitems = tiles_x * tiles_y * items_per_tile;
    V3 org, d0;
    GenRay(s.cam, 0, 0, W, H, smp[0], smp[1], s.fov, org, d0);
    std::vector<Rec> recs(s.refs.size());
    for (size_t k = 0; k < s.refs.size(); k++)
    {
        const Triangle& tr = s.tris[s.refs[k]];
        recs[k] = make_rec(org, s.verts[tr.v0].p, s.verts[tr.v1].p, s.verts[tr.v2].p);
    }
    const uint32_t nth = std::max(1u, std::thread::hardware_concurrency());
    std::vector<Hist> acc(nth);
    std::atomic<uint32_t> next(0);
    std::vector<std::thread> pool;
    for (uint32_t th = 0; th < nth; th++)
        pool.emplace_back([&, th]() {
            std::vector<Walk> lanes(64);
            V3 dir[64];
            Hist& a = acc[th];
            for (;;)
            {
                const uint32_t item = next.fetch_add(1);
                if (item >= nitems) break;
                const uint32_t t = item / items_per_tile, sub_i = item % items_per_tile;
                const uint32_t tx0 = (t % tiles_x) * 16, ty0 = (t / tiles_x) * 16;
                uint32_t maxlen = 0;
                for (uint32_t l = 0; l < 64; l++)
                {
                    const uint32_t slot = sub_i * 64 + l, p = slot / spp, si = slot % spp;
                    const uint32_t x = tx0 + compact_bits(p), y = ty0 + compact_bits(p >> 1);
                    lanes[l].cell.clear(); lanes[l].len.clear();
                    if (x >= W || y >= H) continue;
                    V3 o;
                    GenRay(s.cam, x, y, W, H, smp[2 * si], smp[2 * si + 1], s.fov, o, dir[l]);
                    walk(s, o, dir[l], lanes[l]);
                    maxlen = std::max<uint32_t>(maxlen, uint32_t(lanes[l].cell.size()));
                }
                for (uint32_t j = 0; j < maxlen; j++)
                {
                    uint32_t c0 = 0xFFFFFFFFu, L = 0, mx = 0;
                    bool uni = true;
                    for (uint32_t l = 0; l < 64; l++)
                    {
                        if (j >= lanes[l].cell.size() || lanes[l].len[j] == 0) continue;
                        mx = std::max(mx, lanes[l].len[j]);
                        if (c0 == 0xFFFFFFFFu) { c0 = lanes[l].cell[j]; L = lanes[l].len[j]; }
                        else if (lanes[l].cell[j] != c0) uni = false;
                    }
                    if (c0 == 0xFFFFFFFFu) continue;
                    if (!uni)
                    {
                        // the per-lane loop: iteration i tests record i of every lane's own list
                        for (uint32_t i = 0; i < mx; i++)
                        {
                            bool pass = false;
                            for (uint32_t l = 0; l < 64; l++)
                            {
                                if (j >= lanes[l].cell.size() || i >= lanes[l].len[j]) continue;
                                const Rec& r = recs[s.off[lanes[l].cell[j]] + i];
                                const bool p = ok1(r, dir[l].x, dir[l].y, dir[l].z), rej = gate(r, dir[l].x, dir[l].y, dir[l].z);
                                a.lane_tests++; a.violations += p && rej; pass |= !rej;
                            }
                            a.lane_iters++; a.lane_pass += pass;
                        }
                        continue;
                    }
                    a.lists++;
                    const int b = Hist::bucket(L);
                    bool prev_pass = false;
                    for (uint32_t i = 0; i < L; i++)
                    {
                        const Rec& r = recs[s.off[c0] + i];
                        bool any_ok1 = false, any_pass = false;
                        for (uint32_t l = 0; l < 64; l++)
                        {
                            if (j >= lanes[l].cell.size() || lanes[l].len[j] == 0) continue;
                            const bool p = ok1(r, dir[l].x, dir[l].y, dir[l].z), rej = gate(r, dir[l].x, dir[l].y, dir[l].z);
                            a.lane_tests++; a.violations += p && rej; any_ok1 |= p; any_pass |= !rej;
                        }
                        a.recs[b]++; a.ok1[b] += any_ok1; a.gate[b] += any_pass;
                        if (i & 1u) { a.pairs++; a.pairs_skip += !prev_pass && !any_pass; }
                        prev_pass = any_pass;
                    }
                }
            }
        });
    for (auto& t : pool) t.join();
    Hist a;
    for (auto& x : acc) a.add(x);
    const char *names[Hist::kB] = { "1", "2", "3", "4-7", "8-15", "16-31", "32-63", "64-127", "128+" };
    uint64_t R = 0, O = 0, G = 0;
    for (int i = 0; i < Hist::kB; i++) { R += a.recs[i]; O += a.ok1[i]; G += a.gate[i]; }
    std::printf("{\"waves\": %u, \"uniform_lists\": %llu, \"uniform_records\": %llu, \"ok1_vote_rate\": %.4f, \"gate_vote_rate\": %.4f,\n",
                nitems, (unsigned long long)a.lists, (unsigned long long)R, double(O) / double(R), double(G) / double(R));
    std::printf(" \"by_list_length\": {");
    for (int i = 0; i < Hist::kB; i++)
        std::printf("%s\"%s\": {\"records\": %llu, \"ok1\": %.4f, \"gate\": %.4f}", i ? ", " : "", names[i],
                    (unsigned long long)a.recs[i], a.recs[i] ? double(a.ok1[i]) / a.recs[i] : 0.0,
                    a.recs[i] ? double(a.gate[i]) / a.recs[i] : 0.0);
    std::printf("},\n \"adjacent_pairs\": %llu, \"pairs_neither_passes\": %.4f,\n", (unsigned long long)a.pairs,
                a.pairs ? double(a.pairs_skip) / a.pairs : 0.0);
    std::printf(" \"lane_loop_iterations\": %llu, \"lane_loop_gate_pass_rate\": %.4f,\n", (unsigned long long)a.lane_iters,
                a.lane_iters ? double(a.lane_pass) / a.lane_iters : 0.0);
    std::printf(" \"lane_tests\": %llu, \"ok1_true_and_gate_rejects\": %llu}\n", (unsigned long long)a.lane_tests,
                (unsigned long long)a.violations);
    return a.violations ? 1 : 0;
}
