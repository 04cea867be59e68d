// record_gate_check.cpp -- CPU check of the record gate (csrc/rt_record_gate.h): the
// header librt_tracer.so runs (make_gate, gate_rejects) against the first half of the per-camera-record
// test (rtd::mt_rec_first: det and u of triangle.h:77-87, restated here operation for operation).
//   g++ -O2 -std=c++17 -pthread -ffp-contract=off tests/record_gate_check.cpp -o record_gate_check
//   record_gate_check scene data/scenes/scene8.rtscene 1920 1080 4 16     every 16th tile of the frame
//   record_gate_check adversarial 1 1000000                               seeded families, cases each
//   record_gate_check adversarial 1 1000000 m0 .. m8      ... every direction through the camera's 3x3 first
//   record_gate_check scene FILE W H spp stride [min_list] [--cam c0 .. c15] [--fov deg] [--grid-res n]
//                                               [--offsets x0 y0 ..]     another view, grid, sample table
//   record_gate_check bound m0 .. m8            rtk::cam_dir_bound of a 3x3 and what the library does with it
// rt_frame.cam's 3x3 need not be orthonormal: the direction is normalised first and multiplied by the matrix
// afterwards (rtd::dir_from_xy), so a scaled matrix gives directions the gate's bound E was not computed for.
// csrc/rt_cam_bound.h (the function the library calls per frame) says which matrices keep the gate; the
// checker shows that the gate is sound for those and is NOT for others (why the library's fall-back exists).
// Soundness: no (ray, record) pair with ok1 true and the gate rejecting.  Selectivity (scene mode): how
// often a wave's vote passes a record of a wave-uniform list, for ok1 and for the gate (waves as in
// tools/wave_sim.cpp: 64 consecutive sample slots of a 16x16 tile in Morton order, in lock-step).
// wholly_gated_ok1 (scene mode): records of wave-uniform lists of min_list or more that the gate vote skips
// (every lane rejects) while some lane's ok1 holds -- each one a record the gated loop would wrongly skip.
#include "../oracle/cpu_tracer.cpp"
#include "../cpp-11-ray-trace-march-framework_amd/csrc/rt_record_gate.h"
#include "../cpp-11-ray-trace-march-framework_amd/csrc/rt_cam_bound.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

namespace {

// the pair type of gate_rejects on the host: two plain f32 operations per operator
struct P2 { float x, y; };
inline P2 operator*(P2 a, float s) { P2 r; r.x = a.x * s; r.y = a.y * s; return r; }
inline P2 operator+(P2 a, P2 b) { P2 r; r.x = a.x + b.x; r.y = a.y + b.y; return r; }

struct Rec { float e1[3], e2[3], t[3], g[rtk::kGateFloats]; };

// a reference's record terms as rtd::make_frec forms them, and its gate record
Rec make_rec(const V3& o, const V3& v0, const V3& v1, const V3& v2)
{
    Rec r;
    const V3 e1 = sub(v1, v0), e2 = sub(v2, v0), t = sub(o, v0);
    r.e1[0] = e1.x; r.e1[1] = e1.y; r.e1[2] = e1.z;
    r.e2[0] = e2.x; r.e2[1] = e2.y; r.e2[2] = e2.z;
    r.t[0] = t.x; r.t[1] = t.y; r.t[2] = t.z;
    rtk::make_gate(e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, t.x, t.y, t.z, r.g);
    return r;
}

// rtd::mt_rec_first: (pz, px) = (dx e2y, dy e2z) - (dy e2x, dz e2y), py = dz e2x - dx e2z,
// (det, y) = ((e1x, tx) px + (e1y, ty) py) + (e1z, tz) pz, u = y * (1 / det)
bool ok1(const Rec& r, float dx, float dy, float dz, float *det_out = nullptr, float *u_out = nullptr)
{
    const float pz = dx * r.e2[1] - dy * r.e2[0];
    const float px = dy * r.e2[2] - dz * r.e2[1];
    const float py = dz * r.e2[0] - dx * r.e2[2];
    const float det = (r.e1[0] * px + r.e1[1] * py) + r.e1[2] * pz;
    const float y = (r.t[0] * px + r.t[1] * py) + r.t[2] * pz;
    const float inv = 1.0f / det;
    const float u = y * inv;
    if (det_out) *det_out = det;
    if (u_out) *u_out = u;
    return !(det > -0.00000001f && det < 0.00000001f) & !(u < 0.0f || u > 1.0f);
}

bool gate(const Rec& r, float dx, float dy, float dz)
{
    const P2 n0 = { r.g[0], r.g[1] }, n1 = { r.g[2], r.g[3] }, n2 = { r.g[4], r.g[5] };
    return rtk::gate_rejects(dx, dy, dz, n0, n1, n2, r.g[6]);
}

// ---------------------------------------------------------------------------------- scene mode
struct Walk { std::vector<uint32_t> cell, len; };

// the cells of Grid::Intersect's walk (grid.cpp:159-281), as tools/wave_sim.cpp records them
void walk(const Scene& s, const V3 o, const V3 d, Walk& w)
{
    w.cell.clear(); w.len.clear();
    float enter_t, leave_t;
    V3 g;
    if (PointAABB(o, s.aabb_min, s.aabb_max)) { enter_t = 0.0f; g = o; }
    else if (RayAABB(o, d, s.aabb_min, s.aabb_max, enter_t, leave_t))
        g = mk(o.x + d.x * enter_t, o.y + d.y * enter_t, o.z + d.z * enter_t);
    else return;
    float nct[3], dt[3] = {0, 0, 0};
    int step[3] = {0, 0, 0}, out[3] = {0, 0, 0}, pos[3];
    for (int ax = 0; ax < 3; ax++)
    {
        pos[ax] = s.ToVoxel(g, ax);
        const float da = comp(d, ax);
        if (da == 0.0f) nct[ax] = std::numeric_limits<float>::max();
        else if (da > 0.0f)
        {
            nct[ax] = enter_t + (s.ToPos(pos[ax] + 1, ax) - comp(g, ax)) / da;
            dt[ax] = s.cell_wdh / da; step[ax] = 1; out[ax] = int(s.dim[ax]);
        }
        else
        {
            nct[ax] = enter_t + (s.ToPos(pos[ax], ax) - comp(g, ax)) / da;
            dt[ax] = -s.cell_wdh / da; step[ax] = -1; out[ax] = -1;
        }
    }
    float t = std::numeric_limits<float>::max();
    while (true)
    {
        const int ax = (nct[0] < nct[1]) ? ((nct[0] < nct[2]) ? 0 : 2) : ((nct[1] < nct[2]) ? 1 : 2);
        const uint32_t cell = s.GridIdx(pos[0], pos[1], pos[2]);
        const uint32_t k0 = s.off[cell], k1 = s.off[cell + 1];
        w.cell.push_back(cell);
        w.len.push_back(k1 - k0);
        for (uint32_t k = k0; k < k1; k++)
        {
            const Triangle& tr = s.tris[s.refs[k]];
            float ct, cu, cv;
            if (RayTri(o, d, s.verts[tr.v0].p, s.verts[tr.v1].p, s.verts[tr.v2].p, ct, cu, cv) && ct < t && ct < nct[ax])
                t = ct;
        }
        if (t != std::numeric_limits<float>::max()) break;
        pos[ax] += step[ax];
        if (pos[ax] == out[ax]) break;
        nct[ax] += dt[ax];
    }
}

uint32_t compact_bits(uint32_t v)
{
    v &= 0x55u; v = (v | (v >> 1)) & 0x33u; v = (v | (v >> 2)) & 0x0Fu; return v;
}

struct Acc
{
    uint64_t lane_tests = 0, ok1_true = 0, gate_rejects = 0, violations = 0;
    uint64_t uni_recs = 0, uni_ok1 = 0, uni_gate = 0;           // uniform lists: records, wave votes passed
    uint64_t long_recs = 0, long_ok1 = 0, long_gate = 0;        // ... of lists of min_list records or more
    uint64_t wholly_gated_ok1 = 0;                              // ... skipped by the vote though a lane's ok1 holds
    void add(const Acc& o)
    {
        lane_tests += o.lane_tests; ok1_true += o.ok1_true; gate_rejects += o.gate_rejects; violations += o.violations;
        uni_recs += o.uni_recs; uni_ok1 += o.uni_ok1; uni_gate += o.uni_gate;
        long_recs += o.long_recs; long_ok1 += o.long_ok1; long_gate += o.long_gate;
        wholly_gated_ok1 += o.wholly_gated_ok1;
    }
};

int scene_mode(int argc, char **argv)
{
    if (argc < 7)
    {
        std::fprintf(stderr, "usage: record_gate_check scene file.rtscene W H spp tile_stride [min_list] [--cam c0 .. c15] "
                             "[--fov deg] [--grid-res n] [--offsets x0 y0 ..]\n");
        return 2;
    }
    Scene s;
    if (!ReadScene(argv[2], s)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
    const uint32_t W = std::atoi(argv[3]), H = std::atoi(argv[4]), spp = std::atoi(argv[5]);
    const uint32_t stride = std::max(1, std::atoi(argv[6]));
    uint32_t min_list = 8, grid_res = 64;
    std::vector<float> smp = Hammersley(spp);
    int ai = 7;
    if (ai < argc && argv[ai][0] != '-') min_list = std::atoi(argv[ai++]);
    while (ai < argc)
    {
        const std::string opt = argv[ai++];
        const uint32_t need = opt == "--cam" ? 16u : (opt == "--offsets" ? 2u * spp : 1u);
        if (uint32_t(argc - ai) < need) { std::fprintf(stderr, "%s takes %u values\n", opt.c_str(), need); return 2; }
        if (opt == "--cam")
            for (int k = 0; k < 16; k++) s.cam[k / 4][k % 4] = std::strtof(argv[ai++], nullptr);   // (hex floats too)
        else if (opt == "--fov") s.fov = std::strtof(argv[ai++], nullptr);
        else if (opt == "--grid-res") grid_res = std::atoi(argv[ai++]);
        else if (opt == "--offsets")
            for (uint32_t k = 0; k < 2u * spp; k++) smp[k] = std::strtof(argv[ai++], nullptr);
        else { std::fprintf(stderr, "unknown option %s\n", opt.c_str()); return 2; }
    }
    BuildGrid(s, grid_res);
    const float m9[9] = { s.cam[0][0], s.cam[0][1], s.cam[0][2], s.cam[1][0], s.cam[1][1], s.cam[1][2],
                          s.cam[2][0], s.cam[2][1], s.cam[2][2] };
    const double bound = rtk::cam_dir_bound(m9);
    const uint32_t tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16, items_per_tile = 256 * spp / 64;
    // every camera ray starts at the same origin (camera.h:43): the gate records of every reference
    V3 org, d0;
    GenRay(s.cam, 0, 0, W, H, smp[0], smp[1], s.fov, org, d0);
    std::vector<Rec> recs(s.refs.size());
    for (size_t k = 0; k < s.refs.size(); k++)
    {
        const Triangle& tr = s.tris[s.refs[k]];
        recs[k] = make_rec(org, s.verts[tr.v0].p, s.verts[tr.v1].p, s.verts[tr.v2].p);
    }
    std::vector<uint32_t> tiles;
    for (uint32_t t = 0; t < tiles_x * tiles_y; t += stride) tiles.push_back(t);
    const uint32_t nitems = uint32_t(tiles.size()) * items_per_tile;
    const uint32_t nth = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<Acc> acc(nth);
    std::atomic<uint32_t> next(0);
    std::atomic<int> bad_origin(0);
    std::vector<std::thread> pool;
    for (uint32_t th = 0; th < nth; th++)
        pool.emplace_back([&, th]() {
            std::vector<Walk> lanes(64);
            V3 dir[64];
            for (;;)
            {
                const uint32_t item = next.fetch_add(1);
                if (item >= nitems) break;
                const uint32_t t = tiles[item / items_per_tile], sub_i = item % items_per_tile;
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
                    if (std::memcmp(&o, &org, sizeof(V3)) != 0) bad_origin = 1;
                    walk(s, o, dir[l], lanes[l]);
                    maxlen = std::max<uint32_t>(maxlen, uint32_t(lanes[l].cell.size()));
                }
                Acc& a = acc[th];
                for (uint32_t j = 0; j < maxlen; j++)
                {
                    uint32_t c0 = 0xFFFFFFFFu, L = 0;
                    bool uni = true;
                    for (uint32_t l = 0; l < 64; l++)
                    {
                        if (j >= lanes[l].cell.size() || lanes[l].len[j] == 0) continue;
                        if (c0 == 0xFFFFFFFFu) { c0 = lanes[l].cell[j]; L = lanes[l].len[j]; }
                        else if (lanes[l].cell[j] != c0) uni = false;
                    }
                    if (c0 == 0xFFFFFFFFu) continue;
                    if (!uni)
                    {
                        // per-lane lists: every (lane, record) test
                        for (uint32_t l = 0; l < 64; l++)
                        {
                            if (j >= lanes[l].cell.size()) continue;
                            const uint32_t k0 = s.off[lanes[l].cell[j]], k1 = s.off[lanes[l].cell[j] + 1];
                            for (uint32_t k = k0; k < k1; k++)
                            {
                                const bool p = ok1(recs[k], dir[l].x, dir[l].y, dir[l].z);
                                const bool r = gate(recs[k], dir[l].x, dir[l].y, dir[l].z);
                                a.lane_tests++; a.ok1_true += p; a.gate_rejects += r; a.violations += p && r;
                            }
                        }
                        continue;
                    }
                    const uint32_t k0 = s.off[c0];
                    for (uint32_t k = k0; k < k0 + L; k++)
                    {
                        bool any_ok1 = false, any_pass = false;
                        for (uint32_t l = 0; l < 64; l++)
                        {
                            if (j >= lanes[l].cell.size() || lanes[l].len[j] == 0) continue;
                            const bool p = ok1(recs[k], dir[l].x, dir[l].y, dir[l].z);
                            const bool r = gate(recs[k], dir[l].x, dir[l].y, dir[l].z);
                            a.lane_tests++; a.ok1_true += p; a.gate_rejects += r; a.violations += p && r;
                            any_ok1 |= p; any_pass |= !r;
                        }
                        a.uni_recs++; a.uni_ok1 += any_ok1; a.uni_gate += any_pass;
                        if (L >= min_list)
                        {
                            a.long_recs++; a.long_ok1 += any_ok1; a.long_gate += any_pass;
                            a.wholly_gated_ok1 += any_ok1 && !any_pass;
                        }
                    }
                }
            }
        });
    for (auto& t : pool) t.join();
    Acc a;
    for (auto& x : acc) a.add(x);
    std::printf("{\"mode\": \"scene\", \"tiles\": %u, \"waves\": %u, \"min_list\": %u, \"one_origin\": %s,\n"
                " \"lane_tests\": %llu, \"ok1_true\": %llu, \"gate_rejects\": %llu, \"violations\": %llu,\n"
                " \"uniform_records\": %llu, \"uniform_ok1_votes\": %llu, \"uniform_gate_votes\": %llu,\n"
                " \"long_records\": %llu, \"long_ok1_votes\": %llu, \"long_gate_votes\": %llu,\n"
                " \"wholly_gated_ok1\": %llu, \"cam_bound\": %.17g, \"gate_ok\": %s}\n",
                uint32_t(tiles.size()), nitems, min_list, bad_origin ? "false" : "true",
                (unsigned long long)a.lane_tests, (unsigned long long)a.ok1_true, (unsigned long long)a.gate_rejects,
                (unsigned long long)a.violations, (unsigned long long)a.uni_recs, (unsigned long long)a.uni_ok1,
                (unsigned long long)a.uni_gate, (unsigned long long)a.long_recs, (unsigned long long)a.long_ok1,
                (unsigned long long)a.long_gate, (unsigned long long)a.wholly_gated_ok1, bound,
                rtk::cam_gate_ok(bound) ? "true" : "false");
    return 0;
}

// ---------------------------------------------------------------------------- adversarial mode
typedef std::mt19937_64 Rng;
double uni(Rng& g, double a, double b) { return a + (b - a) * (double(g() >> 11) * (1.0 / 9007199254740992.0)); }
int irand(Rng& g, int a, int b) { return a + int(g() % uint64_t(b - a + 1)); }

V3 rand_v(Rng& g, double r) { return mk(float(uni(g, -r, r)), float(uni(g, -r, r)), float(uni(g, -r, r))); }
float nudge(float x, int ulps)
{
    for (int i = 0; i < (ulps < 0 ? -ulps : ulps); i++) x = std::nextafterf(x, ulps < 0 ? -INFINITY : INFINITY);
    return x;
}
// GenerateRay's normalisation of a direction given in doubles
V3 dir_of(double x, double y, double z)
{
    const V3 v = mk(float(x), float(y), float(z));
    return normalize(v);
}

struct Fam
{
    const char *name;
    uint64_t cases = 0, ok1_true = 0, gate_rejects = 0, violations = 0, e_finite = 0, e_inf = 0;
};

struct Case { V3 o, v0, v1, v2, d; };

// the camera's 3x3 (adversarial mode's optional argument): applied to a normalised direction as rtd::dir_from_xy
// applies it (Transf3x3, row-vector convention), or not at all.  Which normalised direction: the one the camera
// would need for the ray to leave along the family's direction c.d -- c.d times the inverse matrix (fp64),
// normalised as GenerateRay normalises -- so the family still aims where it means to, a few ulp off, whatever the
// matrix rotates or scales; c.d itself for a singular matrix.
bool g_have_m = false, g_have_inv = false;
float g_m[9];
double g_minv[9];

void set_matrix(const float m[9])
{
    std::memcpy(g_m, m, sizeof(g_m));
    g_have_m = true;
    const double a[9] = { m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8] };
    const double c[9] = { a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                          a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                          a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3] };
    const double det = a[0] * c[0] + a[1] * c[3] + a[2] * c[6];
    const double scale = std::fabs(a[0]) + std::fabs(a[1]) + std::fabs(a[2]) + std::fabs(a[3]) + std::fabs(a[4]) +
                         std::fabs(a[5]) + std::fabs(a[6]) + std::fabs(a[7]) + std::fabs(a[8]);
    g_have_inv = std::isfinite(det) && std::fabs(det) > 1e-6 * scale * scale * scale;
    for (int k = 0; g_have_inv && k < 9; k++) g_minv[k] = c[k] / det;
}

void run_case(Fam& f, const Case& c)
{
    const Rec r = make_rec(c.o, c.v0, c.v1, c.v2);
    V3 d = c.d;
    if (g_have_m)
    {
        V3 p = c.d;
        if (g_have_inv)
            p = dir_of(double(c.d.x) * g_minv[0] + double(c.d.y) * g_minv[3] + double(c.d.z) * g_minv[6],
                       double(c.d.x) * g_minv[1] + double(c.d.y) * g_minv[4] + double(c.d.z) * g_minv[7],
                       double(c.d.x) * g_minv[2] + double(c.d.y) * g_minv[5] + double(c.d.z) * g_minv[8]);
        d = mk(p.x * g_m[0] + p.y * g_m[3] + p.z * g_m[6], p.x * g_m[1] + p.y * g_m[4] + p.z * g_m[7],
               p.x * g_m[2] + p.y * g_m[5] + p.z * g_m[8]);
    }
    const bool p = ok1(r, d.x, d.y, d.z), rej = gate(r, d.x, d.y, d.z);
    f.cases++; f.ok1_true += p; f.gate_rejects += rej; f.violations += p && rej;
    if (r.g[6] < INFINITY) f.e_finite++; else f.e_inf++;
}

// a random triangle of edge scale sc around a point at distance ~dist from the origin o
void rand_tri(Rng& g, double sc, double dist, Case& c)
{
    c.o = rand_v(g, 4.0);
    const V3 ctr = rand_v(g, dist);
    c.v0 = mk(c.o.x + ctr.x, c.o.y + ctr.y, c.o.z + ctr.z);
    const V3 a = rand_v(g, sc), b = rand_v(g, sc);
    c.v1 = mk(c.v0.x + a.x, c.v0.y + a.y, c.v0.z + a.z);
    c.v2 = mk(c.v0.x + b.x, c.v0.y + b.y, c.v0.z + b.z);
}

// direction from the origin to the point v0 + u e1 + v e2 of the triangle's plane (exact edges, doubles)
V3 dir_to(const Case& c, double u, double v)
{
    const double e1[3] = { double(c.v1.x) - c.v0.x, double(c.v1.y) - c.v0.y, double(c.v1.z) - c.v0.z };
    const double e2[3] = { double(c.v2.x) - c.v0.x, double(c.v2.y) - c.v0.y, double(c.v2.z) - c.v0.z };
    return dir_of(c.v0.x + u * e1[0] + v * e2[0] - c.o.x, c.v0.y + u * e1[1] + v * e2[1] - c.o.y,
                  c.v0.z + u * e1[2] + v * e2[2] - c.o.z);
}

int adversarial_mode(int argc, char **argv)
{
    if (argc != 4 && argc != 13)
    {
        std::fprintf(stderr, "usage: record_gate_check adversarial seed cases_per_family [m0 .. m8]\n");
        return 2;
    }
    if (argc == 13)
    {
        float m[9];
        for (int k = 0; k < 9; k++) m[k] = std::strtof(argv[4 + k], nullptr);
        set_matrix(m);
    }
    const float ident[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    const double bound = rtk::cam_dir_bound(g_have_m ? g_m : ident);
    Rng g(std::strtoull(argv[2], nullptr, 0));
    const uint64_t N = std::strtoull(argv[3], nullptr, 0);
    std::vector<Fam> fams;

    {   // rays nearly parallel to the triangle's plane: det_r in +-[0.5e-8, 2e-8] (only those are counted)
        Fam f; f.name = "det_near_1e-8";
        uint64_t tries = 0;
        while (f.cases < N && tries < 400 * N)
        {
            tries++;
            Case c;
            rand_tri(g, std::ldexp(1.0, -irand(g, 1, 8)), 2.0, c);
            if (irand(g, 0, 1))
            {   // the origin (nearly) in the plane too: T . pvec is as small as det, u = O(1) and ok1 can hold
                const double a = uni(g, -1.0, 2.0), b = uni(g, -1.0, 2.0);
                c.o = mk(float(c.v0.x + a * (double(c.v1.x) - c.v0.x) + b * (double(c.v2.x) - c.v0.x)),
                         float(c.v0.y + a * (double(c.v1.y) - c.v0.y) + b * (double(c.v2.y) - c.v0.y)),
                         float(c.v0.z + a * (double(c.v1.z) - c.v0.z) + b * (double(c.v2.z) - c.v0.z)));
            }
            const Rec r0 = make_rec(c.o, c.v0, c.v1, c.v2);
            // N = e2 x e1; a direction in the plane plus eps N / |N|^2 has det = eps
            const double n[3] = { double(r0.e2[1]) * r0.e1[2] - double(r0.e2[2]) * r0.e1[1],
                                  double(r0.e2[2]) * r0.e1[0] - double(r0.e2[0]) * r0.e1[2],
                                  double(r0.e2[0]) * r0.e1[1] - double(r0.e2[1]) * r0.e1[0] };
            const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
            if (!(nn > 0.0)) continue;
            const double a = uni(g, -1.0, 1.0), b = uni(g, -1.0, 1.0);
            double p[3] = { a * r0.e1[0] + b * r0.e2[0], a * r0.e1[1] + b * r0.e2[1], a * r0.e1[2] + b * r0.e2[2] };
            const double pl = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
            if (!(pl > 0.0)) continue;
            double eps = (irand(g, 0, 1) ? 1.0 : -1.0) * uni(g, 0.5e-8, 2e-8);
            float det = 0.0f;
            for (int it = 0; it < 3; it++)
            {
                c.d = dir_of(p[0] / pl + eps * n[0] / nn, p[1] / pl + eps * n[1] / nn, p[2] / pl + eps * n[2] / nn);
                ok1(r0, c.d.x, c.d.y, c.d.z, &det);
                const float ad = std::fabs(det);
                if (ad >= 0.5e-8f && ad <= 2e-8f) break;
                // a few ulp of one component move det by about u |N|: walk towards the band
                const int ax = irand(g, 0, 2);
                float *q = ax == 0 ? &c.d.x : (ax == 1 ? &c.d.y : &c.d.z);
                *q = nudge(*q, irand(g, -4, 4));
                ok1(r0, c.d.x, c.d.y, c.d.z, &det);
                if (std::fabs(det) >= 0.5e-8f && std::fabs(det) <= 2e-8f) break;
                eps *= 1.0 + uni(g, -0.5, 0.5);
            }
            if (!(std::fabs(det) >= 0.5e-8f && std::fabs(det) <= 2e-8f)) continue;
            run_case(f, c);
        }
        fams.push_back(f);
    }
    {   // rays within 4 ulp of the lines u = 0 and u = 1
        Fam f; f.name = "u_lines";
        for (uint64_t i = 0; i < N; i++)
        {
            Case c;
            rand_tri(g, std::ldexp(1.0, -irand(g, 0, 6)), 3.0, c);
            c.d = dir_to(c, irand(g, 0, 1) ? 1.0 : 0.0, uni(g, -0.5, 1.5));
            c.d.x = nudge(c.d.x, irand(g, -4, 4)); c.d.y = nudge(c.d.y, irand(g, -4, 4)); c.d.z = nudge(c.d.z, irand(g, -4, 4));
            run_case(f, c);
        }
        fams.push_back(f);
    }
    {   // vertex and edge hits
        Fam f; f.name = "vertex_edge_hits";
        for (uint64_t i = 0; i < N; i++)
        {
            Case c;
            rand_tri(g, std::ldexp(1.0, -irand(g, 0, 6)), 3.0, c);
            const int k = irand(g, 0, 5);
            const double w = uni(g, 0.0, 1.0);
            const double uv[6][2] = { {0, 0}, {1, 0}, {0, 1}, {w, 0}, {0, w}, {w, 1.0 - w} };
            c.d = dir_to(c, uv[k][0], uv[k][1]);
            if (irand(g, 0, 3) == 0) c.d.x = nudge(c.d.x, irand(g, -1, 1));
            run_case(f, c);
        }
        fams.push_back(f);
    }
    {   // zero direction components (axis-parallel rays and rays in a coordinate plane)
        Fam f; f.name = "zero_direction_components";
        for (uint64_t i = 0; i < N; i++)
        {
            Case c;
            rand_tri(g, std::ldexp(1.0, -irand(g, 0, 6)), 3.0, c);
            if (irand(g, 0, 1))
            {   // the triangle in front of the ray along the zeroed axes
                const int ax = irand(g, 0, 2);
                if (ax == 0) c.v0.x = c.o.x; else if (ax == 1) c.v0.y = c.o.y; else c.v0.z = c.o.z;
            }
            c.d = dir_to(c, uni(g, -0.2, 1.2), uni(g, -0.2, 1.2));
            const int z = irand(g, 1, 6);
            if (z & 1) c.d.x = irand(g, 0, 1) ? 0.0f : -0.0f;
            if (z & 2) c.d.y = irand(g, 0, 1) ? 0.0f : -0.0f;
            if ((z & 4) && (z & 3) != 3) c.d.z = 0.0f;
            c.d = normalize(c.d);
            run_case(f, c);
        }
        fams.push_back(f);
    }
    {   // T = 0 (the origin at v0) and an origin in the triangle's plane
        Fam f; f.name = "origin_in_plane";
        for (uint64_t i = 0; i < N; i++)
        {
            Case c;
            rand_tri(g, std::ldexp(1.0, -irand(g, 0, 6)), 3.0, c);
            if (irand(g, 0, 2) == 0) c.o = c.v0;
            else
            {
                const double a = uni(g, -1.0, 2.0), b = uni(g, -1.0, 2.0);
                c.o = mk(float(c.v0.x + a * (double(c.v1.x) - c.v0.x) + b * (double(c.v2.x) - c.v0.x)),
                         float(c.v0.y + a * (double(c.v1.y) - c.v0.y) + b * (double(c.v2.y) - c.v0.y)),
                         float(c.v0.z + a * (double(c.v1.z) - c.v0.z) + b * (double(c.v2.z) - c.v0.z)));
            }
            const V3 r = rand_v(g, 1.0);
            c.d = irand(g, 0, 1) ? dir_of(r.x, r.y, r.z)
                                 : dir_of(double(c.v1.x) - c.v0.x + 1e-3 * r.x, double(c.v1.y) - c.v0.y + 1e-3 * r.y,
                                          double(c.v1.z) - c.v0.z + 1e-3 * r.z);
            run_case(f, c);
        }
        fams.push_back(f);
    }
    {   // zero-area and repeated-vertex triangles
        Fam f; f.name = "degenerate_triangles";
        for (uint64_t i = 0; i < N; i++)
        {
            Case c;
            rand_tri(g, std::ldexp(1.0, -irand(g, 0, 6)), 3.0, c);
            switch (irand(g, 0, 4))
            {
            case 0: c.v1 = c.v0; break;
            case 1: c.v2 = c.v0; break;
            case 2: c.v2 = c.v1; break;
            case 3: c.v1 = c.v0; c.v2 = c.v0; break;
            default:    // collinear: v2 on the line v0 v1
            {
                const double w = uni(g, -2.0, 2.0);
                c.v2 = mk(float(c.v0.x + w * (double(c.v1.x) - c.v0.x)), float(c.v0.y + w * (double(c.v1.y) - c.v0.y)),
                          float(c.v0.z + w * (double(c.v1.z) - c.v0.z)));
            }
            }
            c.d = dir_to(c, uni(g, -0.2, 1.2), uni(g, -0.2, 1.2));
            run_case(f, c);
        }
        fams.push_back(f);
    }
    {   // uniform scales 2^-30 .. 2^39 of a unit-sized configuration (rays aimed at and around the triangle)
        Fam f; f.name = "uniform_scales";
        for (uint64_t i = 0; i < N; i++)
        {
            Case c;
            rand_tri(g, 1.0, 1.0, c);
            c.o = rand_v(g, 1.0);
            const float sc = std::ldexp(1.0f, irand(g, -30, 39));
            for (V3 *p : { &c.o, &c.v0, &c.v1, &c.v2 }) { p->x *= sc; p->y *= sc; p->z *= sc; }
            const int k = irand(g, 0, 3);
            c.d = dir_to(c, k == 0 ? 0.0 : (k == 1 ? 1.0 : uni(g, -0.5, 1.5)), uni(g, -0.5, 1.5));
            if (k < 2) c.d.x = nudge(c.d.x, irand(g, -2, 2));
            run_case(f, c);
        }
        fams.push_back(f);
    }
    {   // a component of e1, e2 or T above 2^40: E must be +inf, the record always tested
        Fam f; f.name = "components_above_2^40";
        for (uint64_t i = 0; i < N; i++)
        {
            Case c;
            rand_tri(g, 1.0, 1.0, c);
            const float big = std::ldexp(float(uni(g, 1.0001, 2.0)), irand(g, 40, 100)) * (irand(g, 0, 1) ? 1.0f : -1.0f);
            V3 *p = irand(g, 0, 2) == 0 ? &c.o : (irand(g, 0, 1) ? &c.v1 : &c.v2);
            const int ax = irand(g, 0, 2);
            (ax == 0 ? p->x : (ax == 1 ? p->y : p->z)) = big;
            const V3 r = rand_v(g, 1.0);
            c.d = irand(g, 0, 1) ? dir_of(r.x, r.y, r.z) : dir_to(c, uni(g, 0.0, 1.0), uni(g, 0.0, 1.0));
            run_case(f, c);
        }
        fams.push_back(f);
    }
    std::printf("{\"mode\": \"adversarial\", \"cam_bound\": %.17g, \"gate_ok\": %s, \"families\": {", bound,
                rtk::cam_gate_ok(bound) ? "true" : "false");
    for (size_t i = 0; i < fams.size(); i++)
        std::printf("%s\n  \"%s\": {\"cases\": %llu, \"ok1_true\": %llu, \"gate_rejects\": %llu, \"violations\": %llu, "
                    "\"e_finite\": %llu, \"e_inf\": %llu}", i ? "," : "", fams[i].name, (unsigned long long)fams[i].cases,
                    (unsigned long long)fams[i].ok1_true, (unsigned long long)fams[i].gate_rejects,
                    (unsigned long long)fams[i].violations, (unsigned long long)fams[i].e_finite,
                    (unsigned long long)fams[i].e_inf);
    std::printf("}}\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && std::string(argv[1]) == "scene") return scene_mode(argc, argv);
    if (argc >= 2 && std::string(argv[1]) == "adversarial") return adversarial_mode(argc, argv);
    if (argc == 11 && std::string(argv[1]) == "bound")
    {
        float m[9];
        for (int k = 0; k < 9; k++) m[k] = std::strtof(argv[2 + k], nullptr);
        const double b = rtk::cam_dir_bound(m);
        std::printf("{\"finite\": %s, \"cam_bound\": %.17g, \"gate_ok\": %s, \"fast_rcp_ok\": %s, \"gate_dmax\": %.17g, "
                    "\"rcp_max_dir\": %.17g}\n", std::isfinite(b) ? "true" : "false", std::isfinite(b) ? b : -1.0,
                    rtk::cam_gate_ok(b) ? "true" : "false", rtk::cam_fast_rcp_ok(b) ? "true" : "false", rtk::kGateDmax,
                    rtk::kCamRcpMaxDir);
        return 0;
    }
    std::fprintf(stderr, "usage: record_gate_check scene|adversarial|bound ...\n");
    return 2;
}
