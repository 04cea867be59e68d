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
//     scene_scale), the ray march's error model (rt_walk.h, ray_march).  A NaN bound never culls, and neither does a
//     bound whose squares overflowed.  Node boxes, triangle records and mesh indices of the sweep are read through
//     wave-uniform addresses (scalar loads); every lane of the wave evaluates every triangle of an entered block.
// Everything here reads only arrays rt_scene_create wrote once: no ordering against any other launch of the scene.
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
