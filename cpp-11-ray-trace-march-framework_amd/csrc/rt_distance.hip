// rt_distance.hip -- the distance-query kernels of librt_tracer.so for gfx950 (MI355X): Renderer::DistanceBruteForce
// (renderer.cpp:138-155) over DistancePointTri (triangle.h:174-198) for points the caller supplies
// (rt_distance_points_device).  DESIGN.md §4.31.
//
// One point per lane; a wave takes 64 consecutive points (of the input, or of the sorted order) and the tail wave
// masks its extra lanes.  Per point the result is the minimum over ALL triangles of the computed distance, with the
// lowest mesh index among equal distances: a value that does not depend on the order the triangles are taken in,
// nor on which of them are taken twice.  So:
//   * each lane seeds its minimum from the block of 32 records whose Morton range holds the lane's own code
//     (a binary search of the blocks' first codes, then a per-lane gather of the block's records);
//   * the wave then sweeps the box hierarchy (rt_dist_tree.h) top down, in index order.  A node is entered iff
//     SOME lane still needs it: !(lb(node box) - margin > the lane's minimum), with margin = 1e-5 (|p|_inf +
//     scene_scale), the ray march's error model (rt_frame_isect.h, ray_march).  A NaN bound never culls, and neither does a
//     bound whose squares overflowed.  Node boxes, triangle records and mesh indices of the sweep are read through
//     wave-uniform addresses (scalar loads); every lane of the wave evaluates every triangle of an entered block.
//     (take, node_needed, eval_block, sweep and point_code: rt_dist_sweep.h, shared with rt_march.hip.)
// Everything here reads only arrays rt_scene_create wrote once: no ordering against any other launch of the scene.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_device.h"
#include "rt_dist_sweep.h"
#include "rt_kparams.h"

namespace rtk {
namespace {

// LineSegMinDistSq (triangle.h:163-172) as rtd::seg_dist_sq forms it, and its proj
__device__ __forceinline__ float seg_closest(float ax, float ay, float az, float abx, float aby, float abz, float len_sq,
                                             float px, float py, float pz, float& qx, float& qy, float& qz)
{
    float t = rtd::dot3(px - ax, py - ay, pz - az, abx, aby, abz) / len_sq;
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
    qx = ax + t * abx;
    qy = ay + t * aby;
    qz = az + t * abz;
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return rtd::dot3(dx, dy, dz, dx, dy, dz);
}

// The point DistancePointTri measured to, by rtd::dist_point_tri's own operations on the same record: the inside
// branch's BarycentricInterpolate (triangle.h:189), else the proj of the segment std::min(l01, std::min(l02, l12))
// returns (l01 wins over the inner minimum, l02 over l12: std::min keeps its first argument on a tie)
__device__ __forceinline__ void closest_on_tri(float px, float py, float pz, const float4& r0, const float4& r1,
                                               const float4& r2, const float4& r3, const float4& r4, const float4& r5,
                                               float& qx, float& qy, float& qz)
{
    const float v0x = r0.x, v0y = r0.y, v0z = r0.z, v1x = r0.w, v1y = r1.x, v1z = r1.y;
    const float v2x = r1.z, v2y = r1.w, v2z = r2.x;
    const float wx = px - v0x, wy = py - v0y, wz = pz - v0z;
    const float dot02 = rtd::dot3(r2.y, r2.z, r2.w, wx, wy, wz);
    const float dot12 = rtd::dot3(r3.x, r3.y, r3.z, wx, wy, wz);
    const float dot00 = r4.z, dot01 = r4.w, dot11 = r5.x, inv_denom = r5.y;
    const float u = (dot00 * dot12 - dot01 * dot02) * inv_denom;
    const float v = (dot11 * dot02 - dot01 * dot12) * inv_denom;
    if ((u >= 0.0f) && (v >= 0.0f) && (u + v < 1.0f))
    {
        const float w = 1.0f - u - v;
        qx = v1x * u + v2x * v + v0x * w;
        qy = v1y * u + v2y * v + v0y * w;
        qz = v1z * u + v2z * v + v0z * w;
        return;
    }
    float ax, ay, az, bx, by, bz, cx, cy, cz;
    const float l01 = seg_closest(v0x, v0y, v0z, r3.x, r3.y, r3.z, dot11, px, py, pz, ax, ay, az);
    const float l02 = seg_closest(v0x, v0y, v0z, r2.y, r2.z, r2.w, dot00, px, py, pz, bx, by, bz);
    const float l12 = seg_closest(v1x, v1y, v1z, r3.w, r4.x, r4.y, r5.z, px, py, pz, cx, cy, cz);
    const bool in12 = l12 < l02;                                  // std::min(l02, l12)
    const float inner = in12 ? l12 : l02;
    const bool in = inner < l01;                                  // std::min(l01, inner)
    qx = in ? (in12 ? cx : bx) : ax;
    qy = in ? (in12 ? cy : by) : ay;
    qz = in ? (in12 ? cz : bz) : az;
}

// EXHAUSTIVE: every record for every point, no seed and no cull (the A/B and parity arm)
template <bool EXHAUSTIVE>
__global__ void __launch_bounds__(kWG) k_distance_points(KDist P)
{
    const uint32_t k = blockIdx.x * kWG + threadIdx.x;
    if (k >= P.n) return;
    const uint32_t i = P.order ? uint32_t(P.order[k] >> 32) : k;
    if (i >= P.n) return;           // (never, for a permutation: no sort word may index past the arrays)
    const float *pp = P.points + size_t(i) * 3u;
    const float px = pp[0], py = pp[1], pz = pp[2];
    float dist = rtd::kFltMax;
    uint32_t tri = rtd::kNoTri, bk = 0;
    if constexpr (EXHAUSTIVE)
    {
        for (uint32_t j = 0; j < P.ntris; j++)
        {
            const float4 *r = P.tri_dist + 6 * size_t(j);
            const float d = rtd::dist_point_tri(px, py, pz, r[0], r[1], r[2], r[3], r[4], r[5]);
            take(d, P.tri_idx[j], j, dist, tri, bk);
        }
    }
    else if (P.nblk != 0)
    {
        // the seed: the last block whose first code is <= the point's (block 0 below every code)
        const uint32_t code = point_code(P, px, py, pz);
        uint32_t lo = 0, hi = P.nblk;
        while (hi - lo > 1)
        {
            const uint32_t mid = (lo + hi) >> 1;
            if (P.blk_key[mid] <= code) lo = mid;
            else hi = mid;
        }
        const uint32_t k1 = min(lo * kDistBlock + kDistBlock, P.ntris);
        for (uint32_t j = lo * kDistBlock; j < k1; j++)
        {
            const float4 *r = P.tri_dist + 6 * size_t(j);
            const float d = rtd::dist_point_tri(px, py, pz, r[0], r[1], r[2], r[3], r[4], r[5]);
            take(d, P.tri_idx[j], j, dist, tri, bk);
        }
        const float margin = 1e-5f * (fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)) + P.scene_scale);
        switch (P.nlevels)
        {
        case 0: sweep<0>(P, 0, P.nblk, px, py, pz, margin, dist, tri, bk); break;
        case 1: sweep<1>(P, 0, P.lvl_n[0], px, py, pz, margin, dist, tri, bk); break;
        case 2: sweep<2>(P, 0, P.lvl_n[1], px, py, pz, margin, dist, tri, bk); break;
        case 3: sweep<3>(P, 0, P.lvl_n[2], px, py, pz, margin, dist, tri, bk); break;
        case 4: sweep<4>(P, 0, P.lvl_n[3], px, py, pz, margin, dist, tri, bk); break;
        default: sweep<5>(P, 0, P.lvl_n[4], px, py, pz, margin, dist, tri, bk); break;
        }
    }
    P.out[i] = make_uint2(__float_as_uint(dist), tri);
    if (P.closest)
    {
        float qx = 0.0f, qy = 0.0f, qz = 0.0f;
        if (tri != rtd::kNoTri)
        {
            const float4 *r = P.tri_dist + 6 * size_t(bk);
            closest_on_tri(px, py, pz, r[0], r[1], r[2], r[3], r[4], r[5], qx, qy, qz);
        }
        float *q = P.closest + size_t(i) * 3u;
        q[0] = qx;
        q[1] = qy;
        q[2] = qz;
    }
}

// RT_DIST_SORT: the sort word of every point, index << 32 | its Morton code (sorted by the low 32 bits)
__global__ void __launch_bounds__(kWG) k_point_keys(KDist P, unsigned long long *keys)
{
    const uint32_t i = blockIdx.x * kWG + threadIdx.x;
    if (i >= P.n) return;
    const float *pp = P.points + size_t(i) * 3u;
    keys[i] = ((unsigned long long)i << 32) | point_code(P, pp[0], pp[1], pp[2]);
}

} // namespace

dist_fn distance_points_kernel(bool exhaustive)
{
    return exhaustive ? k_distance_points<true> : k_distance_points<false>;
}

point_keys_fn point_keys_kernel() { return k_point_keys; }

} // namespace rtk
