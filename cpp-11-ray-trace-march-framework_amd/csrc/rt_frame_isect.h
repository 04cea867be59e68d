// rt_frame_isect.h -- the frame-only intersectors, beside the grid walk of rt_walk.h:
// brute_intersect (RT_ISECT_BRUTE_FORCE) and ray_march (RT_ISECT_RAY_MARCH) of a rendered frame.  Only
// rt_item.h's trace_sample_at calls them; the march QUERY has its own kernel (rt_march.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_device.h"
#include "rt_kparams.h"

namespace rtk {
namespace {

// Renderer::IntersectBruteForce (renderer.cpp:157-197): every triangle in index order, the
// closest accepted hit wins, ties keep the lower index (strict '<', :187).  All lanes of a wave
// walk the same triangle sequence, so the records arrive through wave-uniform (scalar) loads
// and the wave-gated test skips a triangle's second half when no lane can still hit it.
template <bool STATS>
__device__ __forceinline__ bool brute_intersect(const KParams& P, float ox, float oy, float oz, float dx, float dy,
                                                float dz, float& t, float& u, float& v, uint32_t& tri,
                                                uint32_t& tests)
{
    t = rtd::kFltMax;
    for (uint32_t i = 0; i < P.ntris; i++)
    {
        const float4 a = P.tri_mt[3 * i + 0], b = P.tri_mt[3 * i + 1], c = P.tri_mt[3 * i + 2];
        float ct = 0.0f, cu = 0.0f, cv = 0.0f;
        const bool h = rtd::ray_tri_mt_gated(ox, oy, oz, dx, dy, dz, a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x,
                                             ct, cu, cv);
        if (h && ct < t)
        {
            t = ct;
            u = cu;
            v = cv;
            tri = i;
        }
    }
    if (STATS) tests = P.ntris;
    return t != rtd::kFltMax;
}

// Renderer::RayMarch (renderer.cpp:24-41) over Renderer::DistanceBruteForce (:138-155):
// sphere tracing from the camera, at most 128 steps, hit when a step's distance < 0.001.
//
// DistanceBruteForce is a minimum, and the minimum of a set does not depend on the order it
// is taken in ((d < dist) ? d : dist never selects a NaN, ties have equal values), so any
// triangle whose computed distance is provably above the minimum can be skipped, and any member
// may seed it, without changing a bit.  The records are Morton-sorted into blocks of kDistBlock
// triangles with an exact float AABB.  Error model: every computed DistancePointTri is the
// distance to a point of the triangle (the inside branch's convex combination or a clamped
// segment point) up to ~10 ulp of (|p| + |v|); float box distances are off by a few ulp of the
// same scale.  margin = 1e-5 * (|p|_inf + scene_scale) (>= 166 ulp) therefore gives
//   lb(block) - margin <= every computed distance of the block's triangles.
// Per step and lane: the minimum is seeded with the computed distance to the lane's previous
// nearest triangle, blocks are swept outward from that triangle's block (lane 0's), and a block
// is skipped when lb - margin > running minimum for every active lane (wave-uniform branch).
//
// Miss early-out: once p is outside the vertex AABB with box distance Db, receding from it at a
// rate r = dir . (p - clamp(p)) / Db >= 2e-5, and Db > 1.00001 * (margin + 0.001), every later
// point p' = p + s * dir has Db' >= Db + r s and margin' <= margin + 1e-5 s (|dir| <= 1), so
// every later computed distance exceeds 0.001: the reference marches to its 128-step limit
// without a hit (renderer.cpp:30-40).  The march stops there and reports exactly that.
__device__ __forceinline__ void march_eval_block(const KParams& P, uint32_t b, float px, float py, float pz,
                                                 float& dist, uint32_t& best_k)
{
    const uint32_t k0 = b * kDistBlock, k1 = min(k0 + kDistBlock, P.ntris);
    for (uint32_t k = k0; k < k1; k++)
    {
        const float4 *r = P.tri_dist + 6 * size_t(k);
        const float d = rtd::dist_point_tri(px, py, pz, r[0], r[1], r[2], r[3], r[4], r[5]);
        if (d < dist)
        {
            dist = d;
            best_k = k;
        }
    }
}

// true when block b can still lower some active lane's minimum
__device__ __forceinline__ bool march_block_needed(const KParams& P, uint32_t b, float px, float py, float pz,
                                                   float margin, float dist)
{
    const float4 mn = P.dist_blk[2 * b], mx = P.dist_blk[2 * b + 1];
    const float ex = fmaxf(fmaxf(mn.x - px, px - mx.x), 0.0f);
    const float ey = fmaxf(fmaxf(mn.y - py, py - mx.y), 0.0f);
    const float ez = fmaxf(fmaxf(mn.z - pz, pz - mx.z), 0.0f);
    const float lb = __builtin_sqrtf(ex * ex + ey * ey + ez * ez) - margin;
    return __any(!(lb > dist));
}

template <bool STATS, bool EXHAUSTIVE>
__device__ __forceinline__ bool ray_march(const KParams& P, float ox, float oy, float oz, float dx, float dy,
                                          float dz, float& t, uint32_t& steps, uint32_t& tests)
{
    t = 0.0f;
    uint32_t best_k = 0;                 // sorted index of the previous step's nearest triangle
    for (uint32_t s = 0; s < kMarchSteps; s++)
    {
        const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
        float dist = rtd::kFltMax;
        if (EXHAUSTIVE)
        {
            for (uint32_t i = 0; i < P.ntris; i++)
            {
                const float4 *r = P.tri_dist + 6 * size_t(i);
                const float d = rtd::dist_point_tri(px, py, pz, r[0], r[1], r[2], r[3], r[4], r[5]);
                dist = (d < dist) ? d : dist;                        // std::min(dist, d)
            }
            if (STATS) tests += P.ntris;
        }
        else
        {
            const float margin = 1e-5f * (fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)) + P.scene_scale);
            {
                const float wx = px - fminf(fmaxf(px, P.smin[0]), P.smax[0]);
                const float wy = py - fminf(fmaxf(py, P.smin[1]), P.smax[1]);
                const float wz = pz - fminf(fmaxf(pz, P.smin[2]), P.smax[2]);
                const float db = __builtin_sqrtf(wx * wx + wy * wy + wz * wz);
                const float rate = dx * wx + dy * wy + dz * wz;
                if (db > 1.00001f * (margin + 0.001f) && rate >= 2e-5f * db)
                {
                    if (STATS) steps = kMarchSteps;
                    return false;
                }
            }
            {
                // the seed enters as any other member does: (d < dist) never selects a NaN (a triangle with
                // coinciding vertices), which as a plain assignment would keep every later d < dist false
                const float4 *r = P.tri_dist + 6 * size_t(best_k);
                const float d = rtd::dist_point_tri(px, py, pz, r[0], r[1], r[2], r[3], r[4], r[5]);
                dist = (d < dist) ? d : dist;
            }
            uint32_t evals = 1;
            const uint32_t start = __builtin_amdgcn_readfirstlane(best_k / kDistBlock);
            for (uint32_t b = start; b < P.ndist_blk; b++)
            {
                if (!march_block_needed(P, b, px, py, pz, margin, dist)) continue;
                march_eval_block(P, b, px, py, pz, dist, best_k);
                evals += min(b * kDistBlock + kDistBlock, P.ntris) - b * kDistBlock;
            }
            for (uint32_t b = start; b-- > 0;)
            {
                if (!march_block_needed(P, b, px, py, pz, margin, dist)) continue;
                march_eval_block(P, b, px, py, pz, dist, best_k);
                evals += min(b * kDistBlock + kDistBlock, P.ntris) - b * kDistBlock;
            }
            if (STATS) tests += evals;
        }
        t += dist;
        if (STATS) steps = s + 1;
        if (dist < 0.001f) return true;
    }
    return false;
}

} // namespace
} // namespace rtk
