// rt_item.h -- the frame item layer of the render kernels (rt_kernels.hip only): the
// reference's GenerateRay -> intersect -> shading -> resolve path, one wave-sized work item at a time.
// trace_sample* picks the intersector (rt_walk.h's grid walk, or rt_frame_isect.h's two), process_item
// runs an item from its head to its stored pixels, store_record* and process_record write the records.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_frame_isect.h"
#include "rt_item_coord.h"
#include "rt_walk.h"

namespace rtk {
namespace {

// What a product walk leaves for rt_render_records_device: hit, t, u, v, the CSR reference of the hit
// and the walk's end cell (raw: a box-run miss's cell still in its box-word copy).
struct SampleOut { bool hit; float t, u, v; uint32_t voxel, csr; };

// The cell whose CSR list holds reference k: off[c] <= k < off[c + 1] (records of a hit: the walk
// accepts a hit only inside the cell being tested, grid.cpp:258-271, so this is that cell).
__device__ __forceinline__ uint32_t cell_of_ref(const KParams& P, uint32_t k)
{
    uint32_t lo = 0u, hi = uint32_t(P.dim[0]) * uint32_t(P.dim[1]) * uint32_t(P.dim[2]);   // off[hi] = R > k
    while (hi - lo > 1u)
    {
        const uint32_t mid = (lo + hi) >> 1;
        if (P.off[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The colour words of a record (the wide section stores them after its resolve).
__device__ __forceinline__ void store_record_colour(const KParams& Q, uint32_t px, uint32_t py, uint32_t s, float r,
                                                    float g, float b)
{
    const uint32_t rx = px - Q.rec_x0, ry = py - Q.rec_y0;
    if (rx >= Q.rec_w || ry >= Q.rec_h) return;
    volatile uint32_t *o = reinterpret_cast<volatile uint32_t *>(Q.recs + (size_t(ry) * Q.rec_w + rx) * Q.spp + s);
    o[8] = __float_as_uint(r);
    o[9] = __float_as_uint(g);
    o[10] = __float_as_uint(b);
}

// One per-sample record (rt_sample_rec) of a product kernel, for samples inside the requested
// rectangle: rec[((y - y0) * w + (x - x0)) * spp + s], in RAW form -- what the walk leaves, with no
// extra lookups in the product kernels (their register budget decides their occupancy): a hit's CSR
// reference (tri word), a miss's end cell as the walk holds it (voxel word, still inside its copy of
// the cell words).  k_record_fixup then maps the reference to Grid::Intersect's tri_idx and the cell
// it lies in, and moves a raw end cell out of its copy (kRecRaw* in the pad word).  DDA steps and
// tests are not counted by the product walks (0xFFFFFFFF; k_trace_records pins them).
constexpr uint32_t kRecMagic = 0xF1A90000u;     // pad word of a raw record (a -1-filled word is not)
constexpr uint32_t kRecRawCsr = 1u;             // tri word = CSR reference of the hit
constexpr uint32_t kRecRawBox = 2u;             // voxel word = end cell in the ray's box-word copy
constexpr uint32_t kRecRawOct = 4u;             // voxel word = end cell in the ray's octant copy
__device__ __forceinline__ void store_record(const KParams& Q, uint32_t px, uint32_t py, uint32_t s, bool hit,
                                             uint32_t tri, uint32_t voxel, float t, float u, float v, uint32_t raw)
{
    const uint32_t rx = px - Q.rec_x0, ry = py - Q.rec_y0;
    if (rx >= Q.rec_w || ry >= Q.rec_h) return;
    // word by word (volatile: no dwordx4 merging, which needs consecutive VGPRs)
    volatile uint32_t *o = reinterpret_cast<volatile uint32_t *>(Q.recs + (size_t(ry) * Q.rec_w + rx) * Q.spp + s);
    o[0] = hit ? 1u : 0u;
    o[1] = hit ? tri : rtd::kNoTri;
    o[2] = hit ? rtd::kNoTri : voxel;
    o[3] = 0xFFFFFFFFu;
    o[4] = 0xFFFFFFFFu;
    o[5] = hit ? __float_as_uint(t) : 0u;
    o[6] = hit ? __float_as_uint(u) : 0u;
    o[7] = hit ? __float_as_uint(v) : 0u;
    o[11] = kRecMagic | (hit ? (raw & kRecRawCsr) : (raw & ~kRecRawCsr));
}

// renderer.cpp:88-122: one sample -> its colour contribution; hit_tri = the hit triangle
// (Grid::Intersect's tri_idx, renderer.cpp:105) or kNoTri
// (trace_sample_at: from the sample's camera-space x, y -- KParams::ndcx / ndcy entries the caller has loaded)
template <bool STATS, int TRI, int VAR>
__device__ __forceinline__ void trace_sample_at(const KParams& P, float cam_x, float cam_y, uint32_t py, float& cr,
                                                float& cg, float& cb, uint32_t& hit_tri, rt_sample_rec *rec,
                                                uint32_t off = 0u, SampleOut *so = nullptr)
{
    float dx, dy, dz;
    rtd::dir_from_xy(P.m, cam_x, cam_y, dx, dy, dz);                                       // camera.h:8-47
    float t = 0.0f, u = 0.0f, v = 0.0f;
    uint32_t tri = rtd::kNoTri, voxel = rtd::kNoTri, steps = 0, tests = 0;
    bool hit;
    if constexpr ((VAR & kVarMarch) != 0)
        hit = ray_march<STATS, (VAR & kVarExhaustive) != 0>(P, P.org[0], P.org[1], P.org[2], dx, dy, dz, t, steps,
                                                             tests);
    else if constexpr ((VAR & kVarBrute) != 0)
        hit = brute_intersect<STATS>(P, P.org[0], P.org[1], P.org[2], dx, dy, dz, t, u, v, tri, tests);
    else
        hit = grid_intersect<STATS, TRI, VAR>(P, P.org[0], P.org[1], P.org[2], dx, dy, dz, t, u, v, tri, voxel,
                                              steps, tests);
    const KParams& Q = late_params(P, off);
    constexpr bool CSR_TRI = (VAR & (kVarMarch | kVarBrute)) == 0 && (VAR & kVarOriginPre) && TRI == RT_TRI_MOLLER_TRUMBORE;
    if (so)                     // the walk's outcome for a record (process_item stores it)
    {
        so->hit = hit;
        so->t = t;
        so->u = u;
        so->v = v;
        so->voxel = voxel;
        so->csr = CSR_TRI ? tri : rtd::kNoTri;
    }
    if constexpr (CSR_TRI)
        if (hit) tri = __float_as_uint(Q.refs[3 * size_t(tri) + 2].y);     // CSR reference -> triangle id
    if constexpr ((VAR & kVarMarch) != 0)
    {
        // The reference's RayMarch leaves u, v, tri_idx unset (renderer.cpp:103), so the
        // march is shaded by depth: the reference's own alternative at renderer.cpp:118.
        if (hit) cr = cg = cb = t / 3.0f;
        else cr = cg = cb = float(py) / float(Q.H);
    }
    else if (hit)
    {
        const float4 a = Q.shade[3 * tri + 0], b = Q.shade[3 * tri + 1], c = Q.shade[3 * tri + 2];
        rtd::shade_hit(u, v, a, b, c, cr, cg, cb);
    }
    else
    {
        cr = cg = cb = miss_colour(py, Q.H);                     // renderer.cpp:121
    }
    hit_tri = hit ? tri : rtd::kNoTri;
    if (STATS)
    {
        rec->hit = hit;
        rec->tri = hit ? tri : rtd::kNoTri;
        rec->voxel = voxel;
        rec->steps = steps;
        rec->tests = tests;
        rec->t = hit ? t : 0.0f;
        rec->u = hit ? u : 0.0f;
        rec->v = hit ? v : 0.0f;
        rec->r = cr; rec->g = cg; rec->b = cb;
        rec->pad = 0;
    }
}

template <bool STATS, int TRI, int VAR>
__device__ __forceinline__ void trace_sample(const KParams& P, uint32_t px, uint32_t py, uint32_t s, float& cr,
                                             float& cg, float& cb, uint32_t& hit_tri, rt_sample_rec *rec,
                                             uint32_t off = 0u, SampleOut *so = nullptr)
{
    trace_sample_at<STATS, TRI, VAR>(P, P.ndcx[px * P.spp + s], P.ndcy[py * P.spp + s], py, cr, cg, cb, hit_tri, rec,
                                     off, so);
}

// The record of one sample of AUTO's walk (rt_render_records_device), raw (store_record): a box-run
// miss's end cell is still in its box-word copy.
template <int VAR>
__device__ __forceinline__ void process_record(const KParams& Q, const ItemCoord& ic, const SampleOut& so, float cr,
                                               float cg, float cb)
{
    constexpr uint32_t box = ((VAR & kVarSkipRun) && (VAR & kVarPackedRem)) ? kRecRawBox : 0u;
    store_record(Q, ic.x, ic.y, ic.s, so.hit, so.csr, so.voxel, so.t, so.u, so.v,
                 (so.csr != rtd::kNoTri ? kRecRawCsr : 0u) | (so.voxel < kVoxelUnknown ? box : 0u));
    store_record_colour(Q, ic.x, ic.y, ic.s, cr, cg, cb);
}

// One wave-sized work item = 64 consecutive sample slots of a 16x16 tile in Morton order
// (a 2^k x 2^k pixel block x spp samples).  Traces the lane's sample, sums the pixel's
// samples across its adjacent lanes in sample order (renderer.cpp:87-122, hazard H10) and
// stores the packed pixel (renderer.cpp:124-133).
//
// The item's head (item_head) is everything its prologue reads from memory, sent out as ONE group:
// the plan mark of the item's block (block_of_launch; the caller tests it) and the miss-mask word -- wave-uniform:
// scalar loads -- and the lane's two camera-space table entries.  None of the four addresses depends on another's
// value, so all are issued before the first test that reads one and waited for once.  A load with nothing to fetch
// reads a spare word (no mark, no mask) or entry 0 of its table (a lane outside the region), so every address is in
// bounds for every launched block; the tests then read what has arrived, in the order they always had.
struct ItemHead { ItemCoord ic; uint32_t mark_w, mask_w, flag; float cam_x, cam_y; };

// the miss skip (AUTO's lane kernels on the grid walk; the host passes a mask only to frames without hit
// IDs or records): a flagged item's pixels take the row's all-miss word, and no ray is generated
template <int TRI, int VAR>
constexpr bool kItemMissSkip = TRI == RT_TRI_MOLLER_TRUMBORE && (VAR & kVarAutoCore) == kVarAutoCore &&
                               (VAR & (kVarWaveClock | kVarLdsSplit | kVarMarch | kVarBrute | kVarRays)) == 0;

// item: wave-uniform (readfirstlane'd by the caller); mark: the block's plan mark, or null
template <int TRI, int VAR>
__device__ __forceinline__ ItemHead item_head(const KParams& P, uint32_t item, const uint32_t *mark = nullptr)
{
    ItemHead h;
    h.ic = item_coord_pre(P, item, threadIdx.x & 63u);
    const ItemCoord& ic = h.ic;
    h.flag = kItemMissSkip<TRI, VAR> ? item_flag_index(P, item, ic.c.k) : 0u;
    h.mark_w = uniform_word(mark ? mark : spare_word());
    h.mask_w = kItemMissSkip<TRI, VAR> ? uniform_word(P.miss_mask ? P.miss_mask + (h.flag >> 5) : spare_word()) : 0u;
    h.cam_x = P.ndcx[ic.valid ? ic.x * P.spp + ic.s : 0u];
    h.cam_y = P.ndcy[ic.valid ? ic.y * P.spp + ic.s : 0u];
    asm volatile("" : "+s"(h.mark_w), "+s"(h.mask_w), "+v"(h.cam_x), "+v"(h.cam_y));     // the group's one wait
    return h;
}

template <int TRI, int VAR>
__device__ __forceinline__ void process_item(const KParams& P, uint32_t item, uint32_t off, const ItemHead& h)
{
    const uint32_t lane = threadIdx.x & 63u;
    float cr = 0.0f, cg = 0.0f, cb = 0.0f;
    uint32_t hit_tri = rtd::kNoTri;
    SampleOut so{false, 0.0f, 0.0f, 0.0f, rtd::kNoTri, rtd::kNoTri};
    uint32_t origin;
    {
        const ItemCoord& ic = h.ic;
        if constexpr (kItemMissSkip<TRI, VAR>)
            if (P.miss_mask && ((h.mask_w >> (h.flag & 31u)) & 1u) != 0u)
            {
                if (ic.valid && ic.s == 0) store_pixel(P, ic.c, ic.p, ic.x, ic.y, P.rowmiss[ic.y]);
                return;
            }
        origin = tile_origin_word(ic);
        if (ic.valid)
            trace_sample_at<false, TRI, VAR>(P, h.cam_x, h.cam_y, ic.y, cr, cg, cb, hit_tri, nullptr, off, &so);
    }
    const KParams& Q = late_params(P, off);
    const ItemCoord ic = item_coord_post(Q, item, lane, origin);
    // kVarLdsSplit: the workgroup's four waves traced the same samples; wave 0 stores them
    const bool owner = (VAR & kVarLdsSplit) == 0 || threadIdx.x < 64u;
    // rt_render_hits_device only: the sample's hit triangle, after the walk (a scalar test of a
    // kernel parameter; the walk above is the same code whatever the pointer holds)
    if (Q.hits && ic.valid && owner) Q.hits[(size_t(ic.y) * Q.W + ic.x) * Q.spp + ic.s] = hit_tri;
    // rt_render_records_device only, likewise: the sample's record (process_record)
    if (Q.recs && ic.valid && owner) process_record<VAR>(Q, ic, so, cr, cg, cb);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    if (Q.spp == 4u)
    {
        // the bench's 4 spp: a pixel's samples are one quad of lanes, so each sample's colour is
        // a quad broadcast (DPP, one VALU) instead of an LDS permute; same values, same order.
        // renderer.cpp:87-122 starts the sum at 0.0f; 0.0f + x == x for every colour (>= +0:
        // (n + 1) * 0.5 of a normalised component, py / H, t / 3 -- never -0), so the sum
        // starts at the first sample
        sr = quad_bcast<0>(cr) + quad_bcast<1>(cr) + quad_bcast<2>(cr) + quad_bcast<3>(cr);
        sg = quad_bcast<0>(cg) + quad_bcast<1>(cg) + quad_bcast<2>(cg) + quad_bcast<3>(cg);
        sb = quad_bcast<0>(cb) + quad_bcast<1>(cb) + quad_bcast<2>(cb) + quad_bcast<3>(cb);
        // ... and the quad's lanes 0, 1, 2 resolve one channel each (b, g, r: the byte at their
        // position in pack_bgra8's word; lane 3 contributes the zero alpha byte), so the correctly
        // rounded square root and the packing run once per wave instead of three times; the
        // bytes meet in the pixel's lane by quad broadcasts (same per-channel arithmetic)
        const uint32_t j = lane & 3u;
        const float c = j == 0u ? sb : (j == 1u ? sg : sr);
        uint32_t v = resolve_channel4(c) << (8u * j);            // renderer.cpp:124, exact
        v = j == 3u ? 0u : v;
        const uint32_t word = quad_bcast_u<0>(v) | quad_bcast_u<1>(v) | quad_bcast_u<2>(v);
        if (ic.valid && ic.s == 0 && owner) store_pixel(Q, ic.c, ic.p, ic.x, ic.y, word);
        return;
    }
    else
    {
        const uint32_t base = lane & ~(Q.spp - 1u);
        for (uint32_t k = 0; k < Q.spp; k++)
        {
            sr += __shfl(cr, int(base + k), 64);
            sg += __shfl(cg, int(base + k), 64);
            sb += __shfl(cb, int(base + k), 64);
        }
    }
    if (ic.valid && ic.s == 0 && owner)
    {
        store_pixel(Q, ic.c, ic.p, ic.x, ic.y, resolve_word(Q, sr, sg, sb));
    }
}

// an item with no plan mark to test (the wide section's LDS tier)
template <int TRI, int VAR>
__device__ __forceinline__ void process_item(const KParams& P, uint32_t item, uint32_t off = 0u)
{
    item = __builtin_amdgcn_readfirstlane(item);
    process_item<TRI, VAR>(P, item, off, item_head<TRI, VAR>(P, item));
}

} // namespace
} // namespace rtk
