// rt_tracer.hip -- the C ABI's basics (include/rt_tracer.h: version, last error, build hash, device count, the
// sample and AO tables), scene upload and teardown (rt_scene_create / rt_scene_destroy, scene info and sizes)
// and the rt_debug_* entry points of librt_tracer.so.  The rest of the host side:
//   rt_launch.hip   events and stream ordering, frame tables, the render launches (single frames, shards,
//                   batched steps, records, hit IDs), the timing getters and the host copy-back paths
//   rt_queries.hip  rt_trace_samples, the ray, occlusion and distance queries, primary rays, AO frames
//   rt_launch.h     what the three share
// The kernels: rt_kernels.hip (per-sample code in rt_item.h over rt_walk.h), rt_rays.hip, rt_occlusion.hip, rt_ao.hip,
// rt_distance.hip, rt_grid_build.hip; the heavy-first planner: rt_plan.hip; rt_kparams.h is what they share
// with the host files.
//
// Scene layout in HBM (built once by rt_scene_create):
//   cellw     u32[C]              packed cell word in GridIdx order (grid.h:41-42): non-empty
//                                 start << 11 | count, empty: L-inf distance to geometry << 11
//   cellwo    u32[8][C]           the same per ray octant: an empty cell holds the side of the
//                                 largest empty cube extending along the octant
//   cellwb    u32[24][C]          box-run words per octant x major axis (rt_box_words.h)
//   cell_off  u32[C+1]            CSR offsets (scenes whose lists do not fit the packed word)
//   refs      float4[3*R]         one 48-B record per CSR reference, in CSR order:
//                                 {v0.xyz, e1.x} {e1.yz, e2.xy} {e2.z, tri_idx bits, 0, 0}
//   frefs     float4[4*(R+pad)]   per camera origin (k_origin_pre), one 64-B record per CSR
//                                 reference: the origin-only terms of triangle.h:82-98; then
//                                 kFrefPad zero records (the uniform record loop's look-ahead)
//   gates     float4[2*(R+pad)]   beside each frefs buffer (k_origin_pre), one 32-B gate record per
//                                 CSR reference (rt_record_gate.h), the same zero pad
//   shade     float4[3*T]         per triangle the 3 vertex normals (shading of a hit)
//   face_n    float4[T]           face normal (IntersectRayTriBarycentric only)

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rt_tracer.h"
#include "rt_device.h"
#include "rt_internal.h"
#include "rt_box_words.h"
#include "rt_dist_tree.h"
#include "rt_launch.h"

using namespace rtk;

namespace {
thread_local std::string g_err;
} // namespace

int rt_internal_fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

void rtk::hammersley(uint32_t spp, std::vector<float>& xy)
{
    xy.resize(size_t(spp) * 2);
    for (uint32_t s = 0; s < spp; s++)
    {
        double val = 0.0, inv_i = 0.5;
        for (uint32_t n = s; n > 0; n /= 2)
        {
            val += (n % 2) * inv_i;
            inv_i *= 0.5;
        }
        xy[2 * s + 0] = float(double(s) / double(spp) - 0.5f);
        xy[2 * s + 1] = float(val - 0.5f);
    }
}

namespace {
// Dot (lin_alg.h:138-144), accumulating from T() = 0
float dot_ref(const float *a, const float *b)
{
    float r = 0.0f;
    r += a[0] * b[0];
    r += a[1] * b[1];
    r += a[2] * b[2];
    return r;
}

// Distance record of one triangle (layout: rtd::dist_point_tri); the position-independent
// terms of ComputeBarycentric / LineSegMinDistSq (triangle.h:140-150, 166-167)
void dist_record(const float *p0, const float *p1, const float *p2, float4 *r)
{
    const float e0[3] = { p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2] };
    const float e1[3] = { p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2] };
    const float e12[3] = { p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2] };
    const float d00 = dot_ref(e0, e0), d01 = dot_ref(e0, e1), d11 = dot_ref(e1, e1);
    const float inv_denom = 1 / (d00 * d11 - d01 * d01);
    r[0] = make_float4(p0[0], p0[1], p0[2], p1[0]);
    r[1] = make_float4(p1[1], p1[2], p2[0], p2[1]);
    r[2] = make_float4(p2[2], e0[0], e0[1], e0[2]);
    r[3] = make_float4(e1[0], e1[1], e1[2], e12[0]);
    r[4] = make_float4(e12[1], e12[2], d00, d01);
    r[5] = make_float4(d11, inv_denom, dot_ref(e12, e12), 0.0f);
}

// One scheduling tunable from the environment, read by rt_scene_create alone: the launch path never calls getenv
uint32_t env_tunable(const char *name, uint32_t dflt)
{
    const char *e = std::getenv(name);
    return e && *e ? uint32_t(std::strtoul(e, nullptr, 0)) : dflt;
}
} // namespace

int rt_internal_use_device(int device, int *num_cus)
{
    int ndev = 0;
    RT_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(RT_E_NODEVICE, "device index out of range / no GPU");
    hipDeviceProp_t prop;
    RT_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RT_E_NODEVICE, std::string("librt_tracer is built for gfx950, device is ") + prop.gcnArchName);
    RT_HIP(hipSetDevice(device));
    if (num_cus) *num_cus = prop.multiProcessorCount;
    return RT_OK;
}

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_last_error(char *buf, size_t len)
{
    if (!buf || len == 0) return RT_E_INVALID;
    std::snprintf(buf, len, "%s", g_err.c_str());
    return RT_OK;
}

int rt_get_device_count(int *count)
{
    if (!count) return fail(RT_E_INVALID, "count is NULL");
    *count = 0;
    RT_HIP(hipGetDeviceCount(count));
    return RT_OK;
}

#ifndef RT_SRC_HASH
#define RT_SRC_HASH "unknown"
#endif

int rt_build_hash(char *buf, size_t len)
{
    if (!buf || len == 0) return fail(RT_E_INVALID, "bad arguments");
    std::snprintf(buf, len, "%s", RT_SRC_HASH);
    return RT_OK;
}

int rt_scene_info_get(rt_scene *s, rt_scene_info *out)
{
    if (!s || !out) return fail(RT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    std::memset(out, 0, sizeof(*out));
    out->octant_words = s->octant_words;
    out->box_words = s->box_words;
    out->packed_cells = s->d_cellw != nullptr;
    out->rcp_safe = s->rcp_safe;
    out->pack_ok = s->pack_ok;
    out->max_cell_refs = s->max_cell_refs;
    out->hf_floor = s->hf_floor;
    out->hf_min_blocks = s->hf_min_blocks;
    out->wh_floor = s->wh_floor;
    out->wh_alpha16 = s->wh_alpha16;
    out->wh_alpha16_n2 = s->wh_alpha16_n2;
    out->wh_lds = s->wh_lds;
    out->wh_auto_refs = s->wh_auto_refs;
    out->wh_fused = 1;
    out->hf_contexts = kHfCtxs;
    out->hf_evictions = s->hf_evictions;
    out->batch_launches = s->batch_launches;
    out->batch_fallbacks = s->batch_fallbacks;
    out->device_bytes = s->device_bytes;
    return RT_OK;
}

int rt_sample_table(uint32_t spp, float *out_xy)
{
    if (!out_xy || spp == 0) return fail(RT_E_INVALID, "bad arguments");
    std::vector<float> t;
    hammersley(spp, t);
    std::memcpy(out_xy, t.data(), t.size() * sizeof(float));
    return RT_OK;
}

// The built-in AO directions (include/rt_tracer.h): cosine-weighted over the Hammersley points (i + 0.5) / K and
// the base-2 radical inverse of i (hammersley's), in double, rounded once to float.
int rt_ao_table(uint32_t K, float *out_xyz)
{
    if (!out_xyz || K == 0 || K > rtk::kAoMaxDirs) return fail(RT_E_INVALID, "rt_ao_table: K must be in [1, 64]");
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t i = 0; i < K; i++)
    {
        double val = 0.0, inv_i = 0.5;
        for (uint32_t n = i; n > 0; n /= 2)
        {
            val += (n % 2) * inv_i;
            inv_i *= 0.5;
        }
        const double u = (double(i) + 0.5) / double(K), r = std::sqrt(u);
        out_xyz[3 * i + 0] = float(r * std::cos(two_pi * val));
        out_xyz[3 * i + 1] = float(r * std::sin(two_pi * val));
        out_xyz[3 * i + 2] = float(std::sqrt(1.0 - u));
    }
    return RT_OK;
}

// RT_AO_ROTATE's 16 (cos, sin) pairs: angles 2 pi (j + 0.5) / 16, in double, rounded once to float
int rt_ao_rotations(float *out_cs)
{
    if (!out_cs) return fail(RT_E_INVALID, "rt_ao_rotations: NULL argument");
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t j = 0; j < 16; j++)
    {
        const double a = two_pi * (double(j) + 0.5) / 16.0;
        out_cs[2 * j + 0] = float(std::cos(a));
        out_cs[2 * j + 1] = float(std::sin(a));
    }
    return RT_OK;
}

// Cap on the 8 octant copies of the cell words (device and host): 64 M cells at most.
constexpr uint64_t kOctWordsMaxBytes = 256ull << 20;
// ... and on the 24 box-run copies
constexpr uint64_t kBoxWordsMaxBytes = 384ull << 20;

int rt_scene_create(const rt_scene_desc *d, int device, rt_scene **out)
{
    if (!d || !out) return fail(RT_E_INVALID, "desc/out is NULL");
    *out = nullptr;
    const rt_grid_desc& g = d->grid;
    if (d->num_triangles == 0 || d->num_vertices == 0 || !d->vertices || !d->triangles)
        return fail(RT_E_INVALID, "empty mesh");
    if (!g.cell_offsets || g.dims[0] == 0 || g.dims[1] == 0 || g.dims[2] == 0)
        return fail(RT_E_INVALID, "empty grid");
    const uint64_t nc64 = uint64_t(g.dims[0]) * g.dims[1] * g.dims[2];
    if (nc64 >= 0x7FFFFFFFull) return fail(RT_E_INVALID, "grid too large");
    const uint32_t nc = uint32_t(nc64);
    if (g.cell_offsets[0] != 0) return fail(RT_E_INVALID, "cell_offsets[0] != 0");
    for (uint32_t c = 0; c < nc; c++)
        if (g.cell_offsets[c + 1] < g.cell_offsets[c]) return fail(RT_E_INVALID, "cell_offsets not monotonic");
    const uint32_t nr = g.cell_offsets[nc];
    if (nr && !g.cell_tris) return fail(RT_E_INVALID, "cell_tris is NULL");
    for (uint32_t k = 0; k < nr; k++)
        if (g.cell_tris[k] >= d->num_triangles) return fail(RT_E_INVALID, "cell_tris index out of range");
    for (uint32_t i = 0; i < d->num_triangles; i++)
    {
        const rt_triangle& t = d->triangles[i];
        if (t.v0 >= d->num_vertices || t.v1 >= d->num_vertices || t.v2 >= d->num_vertices)
            return fail(RT_E_INVALID, "triangle vertex index out of range");
    }
    int ncus = 0;
    if (int rc = rt_internal_use_device(device, &ncus)) return rc;

    std::unique_ptr<rt_scene> s(new rt_scene());
    s->device = device;
    s->compact_wgs = 8u * uint32_t(std::max(1, ncus));
    // scheduling tunables: read once here, never per launch (A/B sweeps set them per scene)
    s->hf_floor = env_tunable("RT_HF_FLOOR", s->hf_floor);
    s->hf_min_blocks = env_tunable("RT_HF_MIN_BLOCKS", s->hf_min_blocks);
    s->wg64_min_blocks = env_tunable("RT_WG64_MIN_BLOCKS", s->wg64_min_blocks);   // (tests: small frames on k_render_lanes_w64)
    s->hf_shift = std::min(env_tunable("RT_HF_SHIFT", s->hf_shift), 8u);
    s->hf_pos16 = std::min(env_tunable("RT_HF_POS16", s->hf_pos16), 64u);
    s->wg64 = env_tunable("RT_WG64", s->wg64);
    s->wh_floor = env_tunable("RT_WH_FLOOR", s->wh_floor);
    s->wh_alpha16 = env_tunable("RT_WH_ALPHA16", s->wh_alpha16);
    s->wh_alpha16_n2 = env_tunable("RT_WH_ALPHA16_N2", s->wh_alpha16_n2);
    s->wh_alpha16_n4 = env_tunable("RT_WH_ALPHA16_N4", s->wh_alpha16_n4);
    s->wh_alpha16_n8 = env_tunable("RT_WH_ALPHA16_N8", s->wh_alpha16_n8);
    s->wh_auto_refs = env_tunable("RT_WH_AUTO_REFS", s->wh_auto_refs);
    s->wg64_max_refs = env_tunable("RT_WG64_MAX_REFS", s->wg64_max_refs);
    s->wg64_wide = env_tunable("RT_WG64_WIDE", s->wg64_wide);
    s->wg64_o8 = env_tunable("RT_WG64_O8", s->wg64_o8);
    s->wh_lds = env_tunable("RT_WH_LDS", s->wh_lds);
    s->wh_beta16 = env_tunable("RT_WH_BETA16", s->wh_beta16);
    s->hf_follow = env_tunable("RT_HF_FOLLOW", s->hf_follow);
    s->rec_gate = env_tunable("RT_REC_GATE", 1u) != 0u;         // 0: no record gate (the A/B arm)
    s->miss_skip = env_tunable("RT_MISS_SKIP", 1u) != 0u;       // 0: no miss masks (the A/B arm)
    for (int a = 0; a < 3; a++)
    {
        s->dims[a] = g.dims[a];
        s->bmin[a] = g.aabb_min[a];
        s->bmax[a] = g.aabb_max[a];
    }
    s->cw = g.cell_wdh;
    s->icw = g.inv_cell_wdh;
    s->ncells = nc;
    s->nrefs = nr;
    s->ntris = d->num_triangles;

    // Per-reference triangle records in CSR order (see file header)
    std::vector<float4> refs(size_t(std::max(nr, 1u)) * 3);
    double det_bound = 0.0;
    for (uint32_t k = 0; k < nr; k++)
    {
        const uint32_t ti = g.cell_tris[k];
        const rt_triangle& t = d->triangles[ti];
        const float *p0 = d->vertices[t.v0].p, *p1 = d->vertices[t.v1].p, *p2 = d->vertices[t.v2].p;
        const float e1[3] = { p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2] };  // triangle.h:41
        const float e2[3] = { p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2] };  // triangle.h:42
        float idf;
        std::memcpy(&idf, &ti, 4);
        refs[3 * size_t(k) + 0] = make_float4(p0[0], p0[1], p0[2], e1[0]);
        refs[3 * size_t(k) + 1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
        refs[3 * size_t(k) + 2] = make_float4(e2[2], idf, 0.0f, 0.0f);
        // |det| = |e1 . (d x e2)| <= |e1|_1 |e2|_1 for |d| ~ 1 (FAST_RCP range, rcp_nr)
        const double b = (std::fabs(double(e1[0])) + std::fabs(double(e1[1])) + std::fabs(double(e1[2]))) *
                         (std::fabs(double(e2[0])) + std::fabs(double(e2[1])) + std::fabs(double(e2[2])));
        det_bound = (b > det_bound || b != b) ? b : det_bound;
    }
    s->rcp_safe = det_bound == det_bound && det_bound < 0x1p120;
    s->pack_ok = g.dims[0] <= 512 && g.dims[1] <= 512 && g.dims[2] <= 512;
    std::vector<float4> shade(size_t(d->num_triangles) * 3), facen(d->num_triangles);
    std::vector<float4> trimt(size_t(d->num_triangles) * 3), tridist(size_t(d->num_triangles) * 6);
    for (uint32_t i = 0; i < d->num_triangles; i++)
    {
        const rt_triangle& t = d->triangles[i];
        const float *p0 = d->vertices[t.v0].p, *p1 = d->vertices[t.v1].p, *p2 = d->vertices[t.v2].p;
        {
            // brute force: {v0, e1 = v1 - v0, e2 = v2 - v0} (triangle.h:41-42) in triangle order
            const float e1[3] = { p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2] };
            const float e2[3] = { p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2] };
            trimt[3 * size_t(i) + 0] = make_float4(p0[0], p0[1], p0[2], e1[0]);
            trimt[3 * size_t(i) + 1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
            trimt[3 * size_t(i) + 2] = make_float4(e2[2], 0.0f, 0.0f, 0.0f);
        }
        const float *n0 = d->vertices[t.v0].n, *n1 = d->vertices[t.v1].n, *n2 = d->vertices[t.v2].n;
        shade[3 * size_t(i) + 0] = make_float4(n0[0], n0[1], n0[2], n1[0]);
        shade[3 * size_t(i) + 1] = make_float4(n1[1], n1[2], n2[0], n2[1]);
        shade[3 * size_t(i) + 2] = make_float4(n2[2], 0.0f, 0.0f, 0.0f);
        facen[i] = make_float4(t.n[0], t.n[1], t.n[2], 0.0f);
    }
    // Packed cell ranges: start < 2^21 and count < 2^11 for every cell -> one load per DDA step
    std::vector<uint32_t> cellw, cellwo, cellwb;
    bool packable = nr < (1u << 21);
    for (uint32_t c = 0; c < nc && packable; c++) packable = g.cell_offsets[c + 1] - g.cell_offsets[c] < 2048u;
    if (packable)
    {
        // Empty cells carry their Chebyshev (L-inf) distance to the nearest non-empty cell in
        // the start field: a DDA step moves to a face neighbour, so the next dist-1 cells of
        // any walk leaving this cell are empty and need no lookup.  BFS over 26-neighbours
        // from all non-empty cells gives exactly the L-inf distance.
        const uint32_t dxs = g.dims[0], dys = g.dims[1], dzs = g.dims[2];
        std::vector<uint32_t> dist(nc, 0xFFFFFFFFu), frontier, next;
        for (uint32_t c = 0; c < nc; c++)
            if (g.cell_offsets[c + 1] != g.cell_offsets[c]) { dist[c] = 0; frontier.push_back(c); }
        for (uint32_t d = 1; !frontier.empty(); d++)
        {
            next.clear();
            for (uint32_t c : frontier)
            {
                const uint32_t x = c % dxs, z = (c / dxs) % dzs, y = c / (dxs * dzs);   // grid.h:41-42
                for (int oy = -1; oy <= 1; oy++)
                    for (int oz = -1; oz <= 1; oz++)
                        for (int ox = -1; ox <= 1; ox++)
                        {
                            const int nx = int(x) + ox, ny = int(y) + oy, nz = int(z) + oz;
                            if (nx < 0 || ny < 0 || nz < 0 || nx >= int(dxs) || ny >= int(dys) || nz >= int(dzs))
                                continue;
                            const uint32_t n = uint32_t(nx) + uint32_t(nz) * dxs + uint32_t(ny) * dxs * dzs;
                            if (dist[n] == 0xFFFFFFFFu) { dist[n] = d; next.push_back(n); }
                        }
            }
            frontier.swap(next);
        }
        cellw.resize(nc);
        for (uint32_t c = 0; c < nc; c++)
        {
            const uint32_t cnt = g.cell_offsets[c + 1] - g.cell_offsets[c];
            cellw[c] = cnt ? ((g.cell_offsets[c] << 11) | cnt)
                           : (std::min<uint32_t>(dist[c] == 0xFFFFFFFFu ? 0x1FFFFFu : dist[c], 0x1FFFFFu) << 11);
        }
        // Per ray octant (sign of dx, dy, dz) a directional bound: D(c) = the side of the largest
        // empty cube with corner c that extends along the octant's signs (cells outside the grid
        // count as empty).  j steps of a walk in that octant move each coordinate by 0..j in the
        // octant's direction, so the next D-1 cells are empty -- the same contract as the L-inf
        // word, and D >= the L-inf distance.  D(c) = 1 + min of D over the 7 forward neighbours
        // (the 3-D largest-square recurrence).  A grid whose 8 copies would pass kOctWordsMaxBytes keeps
        // the L-inf words (they measured ~2 % slower, profiles/r02x_ab_octant_dist.json).
        if (uint64_t(nc) * 8u * 4u <= kOctWordsMaxBytes)
        {
            s->octant_words = true;
            constexpr uint32_t kInf = 0x1FFFFFu;
            cellwo.resize(size_t(8) * nc);
            std::vector<uint32_t> D(nc);
            for (uint32_t o = 0; o < 8; o++)
            {
                const int sx = (o & 1) ? -1 : 1, sy = (o & 2) ? -1 : 1, sz = (o & 4) ? -1 : 1;
                auto at = [&](int x, int y, int z) -> uint32_t {
                    if (x < 0 || y < 0 || z < 0 || x >= int(dxs) || y >= int(dys) || z >= int(dzs)) return kInf;
                    return D[uint32_t(x) + uint32_t(z) * dxs + uint32_t(y) * dxs * dzs];
                };
                for (int iy = 0; iy < int(dys); iy++)
                    for (int iz = 0; iz < int(dzs); iz++)
                        for (int ix = 0; ix < int(dxs); ix++)
                        {
                            // visit forward neighbours first: against the octant's direction
                            const int x = sx > 0 ? int(dxs) - 1 - ix : ix;
                            const int y = sy > 0 ? int(dys) - 1 - iy : iy;
                            const int z = sz > 0 ? int(dzs) - 1 - iz : iz;
                            const uint32_t c = uint32_t(x) + uint32_t(z) * dxs + uint32_t(y) * dxs * dzs;
                            if (g.cell_offsets[c + 1] != g.cell_offsets[c]) { D[c] = 0; continue; }
                            uint32_t m = kInf;
                            for (int n = 1; n < 8; n++)
                                m = std::min(m, at(x + ((n & 1) ? sx : 0), y + ((n & 2) ? sy : 0), z + ((n & 4) ? sz : 0)));
                            D[c] = std::min(kInf, m + 1);
                        }
                for (uint32_t c = 0; c < nc; c++)
                    cellwo[size_t(o) * nc + c] = (cellw[c] & 2047u) ? cellw[c] : (D[c] << 11);
            }
        }
        // AUTO's box-run words (build_box_words): the non-empty words keep start < 2^20
        if (nr < (1u << 20) && uint64_t(nc) * 24u * 4u <= kBoxWordsMaxBytes)
        {
            s->box_words = rtbox::build_box_words(g.cell_offsets, g.dims, cellwb);
            if (!s->box_words) cellwb.clear();          // out of host memory: AUTO walks without them
        }
    }
    for (uint32_t c = 0; c < nc; c++)
        s->max_cell_refs = std::max(s->max_cell_refs, g.cell_offsets[c + 1] - g.cell_offsets[c]);

    // the per-origin record buffers end in kFrefPad zero records (rt_kparams.h): zeroed once here,
    // k_origin_pre writes only the nr records in front of them (the blocking copies below follow the
    // memsets on the null stream, so the pad is zero before any launch can read it)
    const size_t nfrefs = rtk::fref_buffer_bytes(nr) / sizeof(float4);
    RT_HIP(hipMalloc(&s->d_off, sizeof(uint32_t) * (nc + 1)));
    RT_HIP(hipMalloc(&s->d_refs, sizeof(float4) * refs.size()));
    RT_HIP(hipMalloc(&s->d_frefs[0], sizeof(float4) * nfrefs));
    RT_HIP(hipMalloc(&s->d_frefs[1], sizeof(float4) * nfrefs));
    RT_HIP(hipMemset(s->d_frefs[0], 0, sizeof(float4) * nfrefs));
    RT_HIP(hipMemset(s->d_frefs[1], 0, sizeof(float4) * nfrefs));
    // their gate arrays (rt_record_gate.h), zeroed the same way: a zero gate record rejects nothing
    // (the gated loop addresses a record by a 32-bit byte offset: no gate for a buffer of 4 GiB or more)
    if (rtk::fref_buffer_bytes(nr) > 0xFFFFFFFFull) s->rec_gate = false;
    const size_t ngates = rtk::gate_buffer_bytes(nr) / sizeof(float4);
    for (int b = 0; b < 2; b++)
    {
        RT_HIP(hipMalloc(&s->d_gates[b], sizeof(float4) * ngates));
        RT_HIP(hipMemset(s->d_gates[b], 0, sizeof(float4) * ngates));
    }
    RT_HIP(hipMalloc(&s->d_shade, sizeof(float4) * shade.size()));
    RT_HIP(hipMalloc(&s->d_facen, sizeof(float4) * facen.size()));
    RT_HIP(hipMemcpy(s->d_off, g.cell_offsets, sizeof(uint32_t) * (nc + 1), hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(s->d_refs, refs.data(), sizeof(float4) * refs.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(s->d_shade, shade.data(), sizeof(float4) * shade.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(s->d_facen, facen.data(), sizeof(float4) * facen.size(), hipMemcpyHostToDevice));
    // Distance records in Morton order of the triangle centroids, blocks of kDistBlock with their
    // exact float AABB (the ray march's block cull, see ray_march), and over the blocks the distance
    // queries' box hierarchy, mesh indices and block keys (rt_dist_tree.h)
    std::vector<float4> distblk;
    DistTree dtree;
    {
        static_assert(sizeof(rt_vertex) == 24 && sizeof(rt_triangle) == 24, "dist_tree_build's strides");
        static_assert(kDistTreeBlock == kDistBlock && kDistMaxLevels == kDistLevels, "rt_dist_tree.h / rt_kparams.h");
        const uint32_t nt = d->num_triangles;
        dist_tree_build(nt || d->num_vertices ? d->vertices[0].p : nullptr, 6, d->num_vertices,
                        nt ? &d->triangles[0].v0 : nullptr, 6, nt, dtree);
        s->ndist_blk = dtree.nblk;
        distblk.resize(size_t(s->ndist_blk) * 2);
        if (!distblk.empty()) std::memcpy(distblk.data(), dtree.blk.data(), sizeof(float4) * distblk.size());
        for (uint32_t k = 0; k < nt; k++)
        {
            const rt_triangle& t = d->triangles[dtree.order[k]];
            dist_record(d->vertices[t.v0].p, d->vertices[t.v1].p, d->vertices[t.v2].p, &tridist[6 * size_t(k)]);
        }
        s->scene_scale = dtree.scale;
        for (int a = 0; a < 3; a++)
        {
            s->vmin[a] = dtree.vmin[a];
            s->vmax[a] = dtree.vmax[a];
        }
        s->dist_levels = dtree.nlevels;
        for (uint32_t l = 0; l < kDistLevels; l++)
        {
            s->dist_lvl_off[l] = dtree.lvl_off[l];
            s->dist_lvl_n[l] = dtree.lvl_n[l];
        }
    }
    RT_HIP(hipMalloc(&s->d_distidx, sizeof(uint32_t) * std::max<size_t>(1, dtree.order.size())));
    RT_HIP(hipMemcpy(s->d_distidx, dtree.order.data(), sizeof(uint32_t) * dtree.order.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMalloc(&s->d_distkey, sizeof(uint32_t) * std::max<size_t>(1, dtree.blk_key.size())));
    RT_HIP(hipMemcpy(s->d_distkey, dtree.blk_key.data(), sizeof(uint32_t) * dtree.blk_key.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMalloc(&s->d_distnodes, sizeof(float) * std::max<size_t>(8, dtree.nodes.size())));
    RT_HIP(hipMemcpy(s->d_distnodes, dtree.nodes.data(), sizeof(float) * dtree.nodes.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMalloc(&s->d_distblk, sizeof(float4) * std::max<size_t>(1, distblk.size())));
    RT_HIP(hipMemcpy(s->d_distblk, distblk.data(), sizeof(float4) * distblk.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMalloc(&s->d_trimt, sizeof(float4) * trimt.size()));
    RT_HIP(hipMalloc(&s->d_tridist, sizeof(float4) * tridist.size()));
    RT_HIP(hipMemcpy(s->d_trimt, trimt.data(), sizeof(float4) * trimt.size(), hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(s->d_tridist, tridist.data(), sizeof(float4) * tridist.size(), hipMemcpyHostToDevice));
    if (packable)
    {
        RT_HIP(hipMalloc(&s->d_cellw, sizeof(uint32_t) * nc));
        RT_HIP(hipMemcpy(s->d_cellw, cellw.data(), sizeof(uint32_t) * nc, hipMemcpyHostToDevice));
        if (!cellwo.empty())
        {
            RT_HIP(hipMalloc(&s->d_cellwo, sizeof(uint32_t) * cellwo.size()));
            RT_HIP(hipMemcpy(s->d_cellwo, cellwo.data(), sizeof(uint32_t) * cellwo.size(), hipMemcpyHostToDevice));
            s->oct_stride = nc;
        }
        if (!cellwb.empty())
        {
            RT_HIP(hipMalloc(&s->d_cellwb, sizeof(uint32_t) * cellwb.size()));
            RT_HIP(hipMemcpy(s->d_cellwb, cellwb.data(), sizeof(uint32_t) * cellwb.size(), hipMemcpyHostToDevice));
            s->box_stride = nc;
        }
    }
    s->device_bytes = sizeof(uint32_t) * (nc + 1) +
                      sizeof(float4) * (refs.size() + 2 * nfrefs + 2 * ngates + shade.size() + facen.size() + trimt.size() +
                                        tridist.size() + distblk.size()) +
                      sizeof(uint32_t) * (cellw.size() + cellwo.size() + cellwb.size()) +
                      sizeof(uint32_t) * (dtree.order.size() + dtree.blk_key.size()) + sizeof(float) * dtree.nodes.size();
    RT_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    if (int rc = new_event(s->ev_own, s->ev_order_flags)) return rc;
    for (rtk::EvRef& e : s->ev_done)                                    // dispatches' stop events
        if (int rc = new_event(e, s->ev_time_flags)) return rc;
    s->ev_last = s->ev_own;
    // the plan stream (launch_plans) and the first timed launch's events: created here, not by a
    // frame (a stream's creation took ~0.33 ms of the second frame's call, profiles/r05p_host_trace.log)
    RT_HIP(hipStreamCreateWithFlags(&s->plan_st, hipStreamNonBlocking));
    RT_HIP(hipEventCreateWithFlags(&s->kt0[0], s->ev_time_flags));
    if (int rc = new_event(s->kt1[0], s->ev_time_flags)) return rc;
    // the heavy-first contexts' host-mapped counters, and the frame tables at a 4K x 16 spp capacity:
    // allocated here so a new launch shape's first frame waits for no allocation call
    RT_HIP(hipHostMalloc(&s->h_wh_cnt, sizeof(uint32_t) * 2 * kHfCtxs, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(s->h_wh_cnt, 0, sizeof(uint32_t) * 2 * kHfCtxs);
    {
        void *dev = nullptr;
        RT_HIP(hipHostGetDevicePointer(&dev, s->h_wh_cnt, 0));
        s->d_wh_cnt = static_cast<uint32_t *>(dev);
    }
    // the miss masks' flagged counts, one host-mapped word per buffer (k_miss_mask's last workgroup writes it)
    RT_HIP(hipHostMalloc(&s->h_miss_cnt, sizeof(uint32_t) * 2, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(s->h_miss_cnt, 0, sizeof(uint32_t) * 2);
    {
        void *dev = nullptr;
        RT_HIP(hipHostGetDevicePointer(&dev, s->h_miss_cnt, 0));
        s->d_miss_cnt = static_cast<uint32_t *>(dev);
    }
    s->ndc_cap = size_t(4096 + 4096) * 16u;
    RT_HIP(hipMalloc(&s->d_ndc, s->ndc_cap * sizeof(float)));
    s->smp_cap = 64u;
    RT_HIP(hipMalloc(&s->d_smp, sizeof(float2) * s->smp_cap));
    RT_HIP(hipHostMalloc(&s->h_smp_pinned, sizeof(float2) * s->smp_cap));
    // and the first heavy-first context's state (a new shape's first frame took ~25 us of host time
    // in hf_prepare's hipMalloc: RT_HOST_TRACE, profiles/r05at_host_trace.log)
    if (int rc = hf_alloc(&s->hf[0], kHfPreBlocks)) return rc;

    *out = s.release();
    return RT_OK;
}

int rt_scene_destroy(rt_scene *s)
{
    if (!s) return RT_OK;
    {
        std::lock_guard<std::mutex> lk(s->mtx);
        (void)hipSetDevice(s->device);
        if (s->stream) (void)hipStreamSynchronize(s->stream);
        if (s->last_stream && s->ev_recorded) (void)hipEventSynchronize(s->ev_last->ev);
        if (s->ev_prev) (void)hipEventSynchronize(s->ev_prev->ev);
        if (s->plan_st) (void)hipStreamSynchronize(s->plan_st);
        if (s->side) (void)hipStreamSynchronize(s->side);
        (void)hipFree(s->d_off);
        (void)hipFree(s->d_refs);
        (void)hipFree(s->d_frefs[0]);
        (void)hipFree(s->d_frefs[1]);
        (void)hipFree(s->d_gates[0]);
        (void)hipFree(s->d_gates[1]);
        (void)hipFree(s->d_shade);
        (void)hipFree(s->d_facen);
        (void)hipFree(s->d_cellw);
        (void)hipFree(s->d_cellwo);
        (void)hipFree(s->d_cellwb);
        (void)hipFree(s->d_trimt);
        (void)hipFree(s->d_tridist);
        (void)hipFree(s->d_distblk);
        (void)hipFree(s->d_distidx);
        (void)hipFree(s->d_distkey);
        (void)hipFree(s->d_distnodes);
        (void)hipFree(s->d_clk);
        for (HfCtx& h : s->hf)
        {
            (void)hipFree(h.mem);
            if (h.pend_ev) (void)hipEventDestroy(h.pend_ev);
            if (h.fence_ev) (void)hipEventDestroy(h.fence_ev);
        }
        if (s->h_wh_cnt) (void)hipHostFree(s->h_wh_cnt);
        for (rtk::MissSlot& m : s->miss)
        {
            (void)hipFree(m.d);
            if (m.wr_ev) (void)hipEventDestroy(m.wr_ev);
        }
        if (s->h_miss_cnt) (void)hipHostFree(s->h_miss_cnt);
        if (s->rays_ev_recorded) (void)hipEventSynchronize(s->rays_ev);
        rt_internal_sort_free(s->rays_sort);
        if (s->rays_ev) (void)hipEventDestroy(s->rays_ev);
        if (s->side) (void)hipStreamDestroy(s->side);
        if (s->plan_st) (void)hipStreamDestroy(s->plan_st);
        if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
        if (s->ev_join) (void)hipEventDestroy(s->ev_join);
        (void)hipFree(s->d_smp);
        (void)hipFree(s->d_ndc);
        (void)hipFree(s->d_frame);
        if (s->h_smp_pinned) (void)hipHostFree(s->h_smp_pinned);
        if (s->h_frame) (void)hipHostFree(s->h_frame);
        s->ev_own.reset();             // shared events: destroyed with their last reference
        for (rtk::EvRef& e : s->ev_done) e.reset();
        s->ev_last.reset();
        s->ev_prev.reset();
        for (hipEvent_t e : s->band_ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : s->kt0) if (e) (void)hipEventDestroy(e);
        for (rtk::EvRef& e : s->kt1) e.reset();
        for (hipEvent_t e : s->tile_ev) if (e) (void)hipEventDestroy(e);
        if (s->stream) (void)hipStreamDestroy(s->stream);
        if (s->stream2) (void)hipStreamDestroy(s->stream2);
        if (s->ev_t_fork) (void)hipEventDestroy(s->ev_t_fork);
        if (s->ev_t_join) (void)hipEventDestroy(s->ev_t_join);

    }
    delete s;
    return RT_OK;
}

int rt_fref_buffer_bytes(uint32_t nrefs, uint64_t *bytes)
{
    if (!bytes) return fail(RT_E_INVALID, "NULL argument");
    *bytes = rtk::fref_buffer_bytes(nrefs);
    return RT_OK;
}

int rt_scene_device_bytes(const rt_scene *s, uint64_t *bytes)
{
    if (!s || !bytes) return fail(RT_E_INVALID, "NULL argument");
    *bytes = s->device_bytes;
    return RT_OK;
}

int rt_debug_wave_clocks(rt_scene *s, uint64_t *out, uint32_t max_items, uint32_t *n_items)
{
    if (!s || !n_items) return fail(RT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = ensure_device(s))) return rc;
    *n_items = s->clk_items;
    if (!out || !s->d_clk) return RT_OK;
    RT_HIP(hipDeviceSynchronize());
    RT_HIP(hipMemcpy(out, s->d_clk, sizeof(uint64_t) * 4 * std::min(max_items, s->clk_items), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_debug_heavy_first(rt_scene *s, uint32_t *front, uint32_t *listed, uint32_t *epoch)
{
    if (!s || !front || !listed || !epoch) return fail(RT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = ensure_device(s))) return rc;
    *front = *listed = *epoch = 0;
    const HfCtx *c = nullptr;
    for (const HfCtx& h : s->hf)
        if (h.frames && (!c || h.used > c->used)) c = &h;
    if (!c) return RT_OK;
    RT_HIP(hipDeviceSynchronize());
    HfPlan pl;
    const uint32_t nv = c->pend ? c->pend : c->ver;        // the newest plan launched
    RT_HIP(hipMemcpy(&pl, c->plans + (nv & 1u), sizeof(pl), hipMemcpyDeviceToHost));
    *front = c->front;
    *listed = nv ? std::min(pl.cnt_hi + pl.cnt_lo, c->front) : 0u;
    *epoch = c->frames;
    return RT_OK;
}

int rt_debug_set_plan_delay(rt_scene *s, uint32_t us)
{
    if (!s) return fail(RT_E_INVALID, "NULL scene");
    if (us > 100000u) return fail(RT_E_INVALID, "plan delay must be <= 100000 us");
    std::lock_guard<std::mutex> lk(s->mtx);
    s->plan_delay = us * 100u;          // s_memrealtime ticks (100 MHz)
    return RT_OK;
}

int rt_debug_wide_items(rt_scene *s, uint32_t *count)
{
    if (!s || !count) return fail(RT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    const HfCtx *c = nullptr;
    for (const HfCtx& h : s->hf)
        if (h.wh_cnt && (!c || h.used > c->used)) c = &h;
    if (c) RT_HIP(hipDeviceSynchronize());
    *count = c ? c->wh_cnt[0] + kWavesPerWG * c->wh_cnt[1] : 0u;
    return RT_OK;
}

int rt_debug_wide_tiers(rt_scene *s, uint32_t *listed, uint32_t *lds)
{
    if (!s || !listed || !lds) return fail(RT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = ensure_device(s))) return rc;
    *listed = *lds = 0u;
    const HfCtx *c = nullptr;
    for (const HfCtx& h : s->hf)
        if (h.wh_cnt && (!c || h.used > c->used)) c = &h;
    const uint32_t nv = c ? (c->pend ? c->pend : c->ver) : 0u;     // the newest plan launched
    if (!nv) return RT_OK;
    RT_HIP(hipDeviceSynchronize());
    HfPlan pl;
    RT_HIP(hipMemcpy(&pl, c->plans + (nv & 1u), sizeof(pl), hipMemcpyDeviceToHost));
    *listed = std::min(pl.cnt_w, kWhMax);
    *lds = std::min(pl.cnt_l, kWhMax);
    return RT_OK;
}

int rt_debug_miss_mask(rt_scene *s, uint32_t *flagged, uint32_t *computed)
{
    if (!s || !flagged || !computed) return fail(RT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = ensure_device(s))) return rc;
    RT_HIP(hipDeviceSynchronize());
    const int b = s->miss_frame_slot;
    *flagged = b >= 0 ? (*static_cast<volatile uint32_t *>(s->h_miss_cnt + b) & 0x00FFFFFFu) : 0u;
    *computed = s->miss_computed;
    return RT_OK;
}

int rt_debug_lane_launches(rt_scene *s, uint64_t *launches, uint64_t *one_wave)
{
    if (!s || !launches || !one_wave) return fail(RT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    *launches = s->lane_launches;
    *one_wave = s->w64_launches;
    return RT_OK;
}

int rt_debug_rcp_check(uint64_t *bad_by_exponent, int device)
{
    if (!bad_by_exponent) return fail(RT_E_INVALID, "NULL argument");
    RT_HIP(hipSetDevice(device));
    unsigned long long *d_bad = nullptr;
    RT_HIP(hipMalloc(&d_bad, 256 * sizeof(unsigned long long)));
    hipError_t e = hipMemset(d_bad, 0, 256 * sizeof(unsigned long long));
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(rcp_check_kernel(), dim3(8192), dim3(kWG), 0, nullptr, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(bad_by_exponent, d_bad, 256 * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_debug_rcp_check: ") + hipGetErrorString(e));
    return RT_OK;
}

int rt_debug_gamma_check(uint64_t *mismatches, int device)
{
    if (!mismatches) return fail(RT_E_INVALID, "NULL argument");
    RT_HIP(hipSetDevice(device));
    unsigned long long *d_bad = nullptr;
    RT_HIP(hipMalloc(&d_bad, sizeof(unsigned long long)));
    hipError_t e = hipMemset(d_bad, 0, sizeof(unsigned long long));
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(gamma_check_kernel(), dim3(8192), dim3(kWG), 0, nullptr, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(mismatches, d_bad, sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_debug_gamma_check: ") + hipGetErrorString(e));
    return RT_OK;
}

int rt_debug_primitives(int kind, const float *in, uint32_t n, float *out, int device)
{
    // kind 7 (DistancePointTri) reaches the device as pos + pad + the 24-float scene record
    // kind 8: (n, d) -> {dda_setup's quotient, n / d, 1 when the wave took the reciprocal form} (rt_setup_div.h)
    static const uint32_t in_w[9] = { 18, 12, 23, 3, 11, 18, 18, 28, 2 }, out_w[9] = { 8, 4, 6, 4, 3, 8, 8, 1, 3 };
    if (kind < 0 || kind > 8 || !in || !out) return fail(RT_E_INVALID, "bad arguments");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(device));
    std::vector<float> host_in;
    if (kind == 7)
    {
        host_in.resize(size_t(28) * n);
        for (uint32_t i = 0; i < n; i++)
        {
            const float *a = in + 12 * size_t(i);
            float *o = &host_in[28 * size_t(i)];
            o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = 0.0f;
            dist_record(a + 3, a + 6, a + 9, reinterpret_cast<float4 *>(o + 4));
        }
    }
    else
        host_in.assign(in, in + size_t(in_w[kind]) * n);
    if (kind == 2)   // camera.h:41-42 fov_xs is a host-side constant (double ::tan, hazard H5)
        for (uint32_t i = 0; i < n; i++)
        {
            const float hfov = host_in[23 * size_t(i) + 22] * float(0.0174532925);
            host_in[23 * size_t(i) + 22] = float(::tan(double(hfov / 2.0f)));
        }
    in = host_in.data();
    float *d_in = nullptr, *d_out = nullptr;
    RT_HIP(hipMalloc(&d_in, sizeof(float) * in_w[kind] * n));
    RT_HIP(hipMalloc(&d_out, sizeof(float) * out_w[kind] * n));
    hipError_t e = hipMemcpy(d_in, in, sizeof(float) * in_w[kind] * n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(primitives_kernel(), dim3((n + kWG - 1) / kWG), dim3(kWG), 0, nullptr, kind, d_in, n, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(float) * out_w[kind] * n, hipMemcpyDeviceToHost);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_debug_primitives: ") + hipGetErrorString(e));
    return RT_OK;
}

} // extern "C"
