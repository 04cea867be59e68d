// rt_dist_sweep.h -- what the kernels over the distance hierarchy (rt_dist_tree.h) share: the update of one evaluated
// triangle, the wave's vote on a node box, a block's evaluation, the top-down sweep and the Morton code of a point.
// Included by rt_distance.hip (k_distance_points: one point per lane) and rt_march.hip (k_march_rays: one ray per
// lane, this per step).  DESIGN.md §4.31, §4.35.
//
// The wave sweeps the box hierarchy top down, in index order.  A node is entered iff SOME active lane still needs
// it: !(lb(node box) - margin > the lane's minimum), with margin = 1e-5 (|p|_inf + scene_scale), the ray march's
// error model (rt_frame_isect.h, ray_march).  A NaN bound never culls, and neither does a bound whose squares overflowed.
// Node boxes, triangle records and mesh indices of the sweep are read through wave-uniform addresses (scalar
// loads); every active lane of the wave evaluates every triangle of an entered block.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_device.h"
#include "rt_kparams.h"

namespace rtk {
namespace {

constexpr uint32_t kFan = 32;           // children per node (kDistFan, rt_dist_tree.h)

// the update of one evaluated triangle: std::min's strict '<' (a NaN or infinite d is never selected), and among
// equal distances the lowest mesh index
__device__ __forceinline__ void take(float d, uint32_t mi, uint32_t k, float& dist, uint32_t& tri, uint32_t& bk)
{
    if ((d < dist) || (d == dist && mi < tri))
    {
        dist = d;
        tri = mi;
        bk = k;
    }
}

// true when some active lane cannot rule the box out
__device__ __forceinline__ bool node_needed(const float4 mn, const float4 mx, float px, float py, float pz,
                                            float margin, float dist)
{
    const float ex = fmaxf(fmaxf(mn.x - px, px - mx.x), 0.0f);
    const float ey = fmaxf(fmaxf(mn.y - py, py - mx.y), 0.0f);
    const float ez = fmaxf(fmaxf(mn.z - pz, pz - mx.z), 0.0f);
    const float s = ex * ex + ey * ey + ez * ez;
    const float lb = __builtin_sqrtf(s) - margin;
    return __any(!(lb > dist) || !(s <= rtd::kFltMax));
}

// block b's records for every lane of the wave (b is wave-uniform)
__device__ __forceinline__ void eval_block(const KDist& P, uint32_t b, float px, float py, float pz, float& dist,
                                           uint32_t& tri, uint32_t& bk)
{
    const uint32_t k0 = b * kDistBlock, k1 = min(k0 + kDistBlock, P.ntris);
    for (uint32_t k = k0; k < k1; k++)
    {
        const float4 *r = P.tri_dist + 6 * size_t(k);
        const float d = rtd::dist_point_tri(px, py, pz, r[0], r[1], r[2], r[3], r[4], r[5]);
        take(d, P.tri_idx[k], k, dist, tri, bk);
    }
}

// Nodes [i0, i1) of level L (0: the blocks; j: upper level j), in index order
template <int L>
__device__ __forceinline__ void sweep(const KDist& P, uint32_t i0, uint32_t i1, float px, float py, float pz,
                                      float margin, float& dist, uint32_t& tri, uint32_t& bk)
{
    const float4 *box;
    if constexpr (L == 0) box = P.blk;
    else box = P.nodes + 2 * size_t(P.lvl_off[L - 1]);
    for (uint32_t i = i0; i < i1; i++)
    {
        if (!node_needed(box[2 * size_t(i)], box[2 * size_t(i) + 1], px, py, pz, margin, dist)) continue;
        if constexpr (L == 0) eval_block(P, i, px, py, pz, dist, tri, bk);
        else
        {
            uint32_t nchild;
            if constexpr (L == 1) nchild = P.nblk;
            else nchild = P.lvl_n[L - 2];
            sweep<L - 1>(P, i * kFan, min(i * kFan + kFan, nchild), px, py, pz, margin, dist, tri, bk);
        }
    }
}

__device__ __forceinline__ uint32_t spread10(uint32_t v)     // 10 bits -> every third bit
{
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// Morton code of the point clamped into the vertex box (rt_dist_tree.h dist_morton's bit order).  Any value is a
// valid code: it picks the seed block and the sort position, never a result.  A NaN coordinate (and inf on a flat
// axis, inf * 0) counts as the box's min: fmaxf drops the NaN.
__device__ __forceinline__ uint32_t point_code(const KDist& P, float px, float py, float pz)
{
    const float p[3] = { px, py, pz };
    uint32_t q[3];
    // (clamping the scaled offset to [0, 1023] is clamping the point into the box: the map is monotone)
    for (int a = 0; a < 3; a++) q[a] = uint32_t(fminf(fmaxf((p[a] - P.vmin[a]) * P.vinv[a], 0.0f), 1023.0f));
    return (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
}

} // namespace
} // namespace rtk
