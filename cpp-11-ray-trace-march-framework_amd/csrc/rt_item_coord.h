// rt_item_coord.h -- where a frame's work item lies and what its pixels become: tile and
// item coordinates, the miss-mask bit of an item, the pixel store, the resolve of a pixel's sums and the
// all-miss word of a row.  No ray is traced here: the planner (rt_plan.hip) includes this header alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_device.h"
#include "rt_kparams.h"
#include "rt_wave.h"

namespace rtk {
namespace {

// renderer.cpp:121: the colour of a sample that hits nothing (trace_sample; row_miss_word)
__device__ __forceinline__ float miss_colour(uint32_t py, uint32_t H) { return float(py) / float(H); }

// Tile bookkeeping: block -> (local tile k, sub-block)
struct TileCoord { uint32_t k, sub, tx0, ty0; };

__device__ __forceinline__ TileCoord tile_of_block(const KParams& P)
{
    TileCoord c;
    c.k = blockIdx.x / P.wg_per_tile;
    c.sub = blockIdx.x - c.k * P.wg_per_tile;
    uint32_t tx, ty;
    shard_tile_xy(c.k, P.rank, P.nranks, P.tiles_x, tx, ty);
    c.tx0 = P.rx0 + tx * kTile;
    c.ty0 = P.ry0 + ty * kTile;
    return c;
}

__device__ __forceinline__ void store_pixel(const KParams& P, const TileCoord& c, uint32_t p, uint32_t x,
                                            uint32_t y, uint32_t word)
{
    if (P.shard_mode == 2u)
    {
        // the Framebuffer's tile buffers back to back in tile order c + r * fb_tx: tile (c, r) starts
        // at y0 * W + th_r * x0 (the tiles above it, then the row's tiles left of it, all th_r tall),
        // pixel (x, y) at buf[(x - x0) + (y - y0) * tw_c] (renderer.cpp:133).  x, y < 2^16 and the
        // tile sizes < 2^16, so the mul_hi quotients are exact.
        const uint32_t c = P.fb_tw ? min(__umulhi(x, P.fb_mtw), P.fb_tx - 1u) : P.fb_tx - 1u;
        const uint32_t r = P.fb_th ? min(__umulhi(y, P.fb_mth), P.fb_ty - 1u) : P.fb_ty - 1u;
        const uint32_t x0 = c * P.fb_tw, y0 = r * P.fb_th;
        const uint32_t tw = c == P.fb_tx - 1u ? P.W - x0 : P.fb_tw;
        const uint32_t th = r == P.fb_ty - 1u ? P.H - y0 : P.fb_th;
        P.out[size_t(y0) * P.W + size_t(th) * x0 + (y - y0) * tw + (x - x0)] = word;
    }
    else if (P.shard_mode)
        P.out[size_t(c.k) * kTilePix + compact_bits(p >> 1) * kTile + compact_bits(p)] = word;
    else
        P.out[size_t(y - P.ry0) * P.pitch + (x - P.rx0)] = word;     // renderer.cpp:133
}

// renderer.cpp:124 col / float(spp); exact as a multiply when spp is a power of two
__device__ __forceinline__ float average(const KParams& P, float sum)
{
    return P.inv_spp != 0.0f ? sum * P.inv_spp : sum / float(P.spp);
}

struct ItemCoord { TileCoord c; uint32_t p, s, x, y; bool valid; };

// Sample slot `slot` (pixel-major, Morton pixel order) of local tile k.
__device__ __forceinline__ ItemCoord tile_slot_coord(const KParams& P, uint32_t k, uint32_t slot)
{
    ItemCoord ic;
    ic.c.k = k;
    uint32_t tx, ty;
    shard_tile_xy(k, P.rank, P.nranks, P.tiles_x, tx, ty);
    ic.c.tx0 = P.rx0 + tx * kTile;
    ic.c.ty0 = P.ry0 + ty * kTile;
    ic.p = slot >> P.spp_shift;                               // pixel index in the tile (Morton)
    ic.s = slot & (P.spp - 1u);
    ic.x = ic.c.tx0 + compact_bits(ic.p);
    ic.y = ic.c.ty0 + compact_bits(ic.p >> 1);
    ic.valid = ic.x < P.rx0 + P.rw && ic.y < P.ry0 + P.rh;
    return ic;
}

// Pixel/sample of this lane in work item `item` (wave-uniform): the compact kernel's and the wide
// section's form, for any tile size (process_item has its own, item_coord_pre / item_coord_post).
__device__ __forceinline__ ItemCoord item_coord(const KParams& P, uint32_t item, uint32_t lane)
{
    const uint32_t items_per_tile = P.wg_per_tile * kWavesPerWG;
    const uint32_t kseq = item / items_per_tile;              // position in the launch's tile order
    const uint32_t slot = (item - kseq * items_per_tile) * 64u + lane;
    return tile_slot_coord(P, P.tile_order ? P.tile_order[kseq] : kseq, slot);   // local tile k
}

// process_item's form of item_coord.  Before the walk (item_coord_pre): the same coordinates with the
// two u32 divisions replaced -- the work items per tile are a power of two in every lane kernel
// (P.ipt_shift), and the shard deal divides by P.tiles_x through its magic (shard_tile_xy_m).  The
// item's TILE ORIGIN then crosses the walk in ONE packed VGPR (tile_origin_word: tx0 | ty0 << 16 --
// every launched tile holds a pixel of the region, so tx0 < rx0 + rw <= 65536 and ty0 likewise:
// validate_frame; wave-uniform, but kept in a VGPR: the kernel has no SGPR to spare across the walk),
// and item_coord_post rebuilds the whole ItemCoord from it in full 32-bit arithmetic, so a lane of a
// tile that overhangs the region (x or y up to 15 past it, past 2^16 too) is invalid exactly as
// item_coord finds it: the Morton offsets come from the lane, the sample is the lane's low bits,
// validity the same two compares.
// (slot_coord_m: sample slot `slot` of local tile k, tile_slot_coord with the shard deal's magic division; k_miss_mask
// takes the corner lanes of an item in the launch's natural order from it)
__device__ __forceinline__ ItemCoord slot_coord_m(const KParams& P, uint32_t k, uint32_t slot)
{
    ItemCoord ic;
    ic.c.k = k;
    uint32_t tx, ty;
    shard_tile_xy_m(ic.c.k, P.rank, P.nranks, P.tiles_x, P.tiles_x_m, tx, ty);
    ic.c.tx0 = P.rx0 + tx * kTile;
    ic.c.ty0 = P.ry0 + ty * kTile;
    ic.p = slot >> P.spp_shift;
    ic.s = slot & (P.spp - 1u);
    ic.x = ic.c.tx0 + compact_bits(ic.p);
    ic.y = ic.c.ty0 + compact_bits(ic.p >> 1);
    ic.valid = ic.x < P.rx0 + P.rw && ic.y < P.ry0 + P.rh;
    return ic;
}

__device__ __forceinline__ ItemCoord item_coord_pre(const KParams& P, uint32_t item, uint32_t lane)
{
    const uint32_t kseq = item >> P.ipt_shift;                // position in the launch's tile order
    const uint32_t slot = ((item - (kseq << P.ipt_shift)) << 6) + lane;
    return slot_coord_m(P, P.tile_order ? P.tile_order[kseq] : kseq, slot);    // local tile k
}

// The miss skip: bit `local tile k * items per tile + item in tile` of KParams::miss_mask -- the
// launch's NATURAL item order, whatever tile_order says -- is set when k_miss_mask proved that every sample of
// the item misses the grid box (rt_miss_mask.h).  Wave-uniform: one scalar load (process_item issues it beside the
// item's other prologue words) and a bit test.
__device__ __forceinline__ uint32_t item_flag_index(const KParams& P, uint32_t item, uint32_t k)
{
    return (k << P.ipt_shift) + (item & ((1u << P.ipt_shift) - 1u));
}

// The resolve of one pixel (renderer.cpp:124-133), shared by process_item and k_miss_mask's row table.
// resolve_channel4: one channel of the spp-4 quad form, from the sum of its four samples (c * 0.25f is exact);
// resolve_word: the generic form, from the three sums.
__device__ __forceinline__ uint32_t resolve_channel4(float c) { return rtd::pack_channel(rtd::gamma_half(c * 0.25f)); }
__device__ __forceinline__ uint32_t resolve_word(const KParams& Q, float sr, float sg, float sb)
{
    return rtd::pack_bgra8(rtd::gamma_half(average(Q, sr)), rtd::gamma_half(average(Q, sg)), rtd::gamma_half(average(Q, sb)));
}

// The packed BGRA word of a pixel of row y whose samples all miss (KParams::rowmiss[y]): process_item's own
// sums and resolve on spp copies of the miss colour -- the quad form at spp 4 (the sum starts at the first
// sample), the generic form otherwise (the sum starts at 0.0f).
__device__ __forceinline__ uint32_t row_miss_word(const KParams& P, uint32_t y)
{
    const float c = miss_colour(y, P.H);
    if (P.spp == 4u)
    {
        const uint32_t v = resolve_channel4(c + c + c + c);
        return v | (v << 8) | (v << 16);
    }
    float sum = 0.0f;
    for (uint32_t k = 0; k < P.spp; k++) sum += c;
    return resolve_word(P, sum, sum, sum);
}

// The tile origin of an ItemCoord as one word held in a VGPR (the empty asm keeps the compiler from
// carrying the wave-uniform value in an SGPR across the walk).
__device__ __forceinline__ uint32_t tile_origin_word(const ItemCoord& ic)
{
    uint32_t w = ic.c.tx0 | (ic.c.ty0 << 16);
    asm volatile("" : "+v"(w));
    return w;
}

__device__ __forceinline__ ItemCoord item_coord_post(const KParams& Q, uint32_t item, uint32_t lane, uint32_t origin)
{
    const uint32_t kseq = item >> Q.ipt_shift;
    const uint32_t o = __builtin_amdgcn_readfirstlane(origin);
    ItemCoord ic;
    ic.c.k = Q.tile_order ? Q.tile_order[kseq] : kseq;
    ic.c.tx0 = o & 0xFFFFu;
    ic.c.ty0 = o >> 16;
    ic.p = (((item - (kseq << Q.ipt_shift)) << 6) + lane) >> Q.spp_shift;
    ic.s = lane & (Q.spp - 1u);
    ic.x = ic.c.tx0 + compact_bits(ic.p);
    ic.y = ic.c.ty0 + compact_bits(ic.p >> 1);
    ic.valid = ic.x < Q.rx0 + Q.rw && ic.y < Q.ry0 + Q.rh;
    return ic;
}

} // namespace
} // namespace rtk
