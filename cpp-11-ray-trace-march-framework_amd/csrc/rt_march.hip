// rt_march.hip -- the march-query kernel of librt_tracer.so for gfx950 (MI355X): Renderer::RayMarch (renderer.cpp:24-41)
// over Renderer::DistanceBruteForce (:138-155) for rays the caller supplies (rt_march_rays_device).  DESIGN.md §4.35.
//
// One ray per lane; a wave takes 64 consecutive rays (of the input, or of the sorted order) and the tail wave masks
// its extra lanes.  The contract's loop, every float operation one f32 rounding:
//     t = 0;  for (s = 0; s < max_steps; s++) { pos = o + t * d;  dist = DistanceBruteForce(pos);  t += dist;
//                                               if (dist < min_dist) HIT at step s + 1; }   MISS
// A lane leaves the step loop when it hits (or provably misses, below), so the loop runs while any lane of the wave
// is still marching, and every vote of the sweep (node_needed, rt_dist_sweep.h) is taken over the marching lanes
// alone: a finished lane keeps no node alive for the others, and its record is frozen.
//
// A step is what k_distance_points does for a point (rt_distance.hip): a seed block gathered per lane, then the sweep
// of the box hierarchy under lb - margin > dist.  The seed is the block of the previous step's nearest record (step 0:
// the block whose Morton range holds the origin's code) -- RT_MARCH_SEED 0 builds the other arm, the Morton search of
// every step's position.  Either is exact: the minimum, and the lowest index among equal distances, do not depend on
// the order of evaluation nor on what is evaluated twice.
//
// The receding-miss stop (RT_MARCH_STOP 0 builds the arm without it; never in the exhaustive kernel).  Notation:
// B the vertex box, p the step's computed position, w = p - clamp(p, B), Db = |w|, L1 = |dx| + |dy| + |dz|,
// margin = 1e-5 (|p|_inf + scene_scale), E = 2.5e-7 (|o|_inf + 2 |p|_inf), u = 2^-24.  The lane stops as a MISS when
//     Db > 1.00001 (margin + min_dist + E)   and   d . w >= 2e-5 L1 Db   (all of them finite, 2e-5 L1 Db normal).
// Proof that the contract's loop then never hits.  Later steps have t' >= t (dist >= 0, never NaN).  A computed
// position is off the real line o + t d by at most u (|o_i| + 2 |p_i|) (1 + 2u) per component (one rounding of the
// product, one of the sum), so p' = p + s d + e with s = t' - t >= 0 and, in the 2-norm, |e| <= E + 3.6 u s L1.
// The distance to a convex box is convex along a line and its slope at p is d . w / Db, which the second condition
// bounds below by 1.9e-5 L1 (the float dot product is within 3 u L1 Db of the real one).  Hence
//     dist(p', B) >= Db + 1.9e-5 s L1 - E - 3.6 u s L1,   margin' <= margin + 1e-5 (s L1 + E + 3.6 u s L1),
// and dist(p', B) - margin' >= Db - margin - 1.00001 E + s L1 (1.9e-5 - 1e-5 - 5 u) > min_dist.  Every computed
// DistancePointTri at p' is at least dist(p', B) - margin' (the cull's error model, DESIGN §4.3, for the box of the
// whole mesh; the factor 1.00001 pays for the float box distance), so no later step -- nor this one, s = 0 -- is
// below min_dist.  A later position that is no longer finite, or whose squares overflow, has dist = FLT_MAX, which
// is not below a finite min_dist either.  Rays that fail a premise (a non-finite component, an overflow, a
// direction whose products underflow) do not take the stop: they march on.  min_dist <= 0 never hits (dist >= 0):
// those calls write their misses at once.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_device.h"
#include "rt_dist_sweep.h"
#include "rt_kparams.h"

#ifndef RT_MARCH_SEED       // (tools/build_variant.sh -DRT_MARCH_SEED=0: the A/B arm, the Morton search per step)
#define RT_MARCH_SEED 1
#endif
#ifndef RT_MARCH_STOP       // (tools/build_variant.sh -DRT_MARCH_STOP=0: the A/B arm without the receding-miss stop)
#define RT_MARCH_STOP 1
#endif

namespace rtk {
namespace {

constexpr float kFltMin = 1.17549435e-38f;     // std::numeric_limits<float>::min()

// the block whose Morton range holds the point's code: the last block whose first code is <= it (block 0 below
// every code), as k_distance_points' seed
__device__ __forceinline__ uint32_t morton_block(const KDist& P, float px, float py, float pz)
{
    const uint32_t code = point_code(P, px, py, pz);
    uint32_t lo = 0, hi = P.nblk;
    while (hi - lo > 1)
    {
        const uint32_t mid = (lo + hi) >> 1;
        if (P.blk_key[mid] <= code) lo = mid;
        else hi = mid;
    }
    return lo;
}

// every record for every lane of the wave, through wave-uniform addresses
__device__ __forceinline__ void eval_all(const KDist& P, float px, float py, float pz, float& dist, uint32_t& tri,
                                         uint32_t& bk)
{
    for (uint32_t j = 0; j < P.ntris; j++)
    {
        const float4 *r = P.tri_dist + 6 * size_t(j);
        const float d = rtd::dist_point_tri(px, py, pz, r[0], r[1], r[2], r[3], r[4], r[5]);
        take(d, P.tri_idx[j], j, dist, tri, bk);
    }
}

// EXHAUSTIVE: every record at every step, no seed, no cull and no early stop (the A/B and parity arm).  The default
// arm on a mesh of at most kDistSmallBlocks blocks evaluates every record too -- the seed alone would be half or all
// of such a mesh (rt_distance_points_device's rule) -- and keeps the early stop.
// (amdgpu_num_sgpr(96): the sweep's five levels and the step loop want 106 scalar registers, one 16-register granule
// past 8 waves per SIMD; capped, 18 of them live in the lanes of one vector register instead)
template <bool EXHAUSTIVE>
__global__ void __launch_bounds__(kWG) __attribute__((amdgpu_num_sgpr(96))) k_march_rays(KMarch M)
{
    const KDist& P = M.d;
    const uint32_t k = blockIdx.x * kWG + threadIdx.x;
    if (k >= P.n) return;
    const uint32_t i = P.order ? uint32_t(P.order[k] >> 32) : k;
    if (i >= P.n) return;           // (never, for a permutation: no sort word may index past the arrays)
    const float2 *rp = M.rays + size_t(i) * 3u;
    const float2 r0 = rp[0], r1 = rp[1], r2 = rp[2];
    const float ox = r0.x, oy = r0.y, oz = r1.x, dx = r1.y, dy = r2.x, dz = r2.y;
    float t = 0.0f, dist = 0.0f;
    uint32_t tri = rtd::kNoTri, steps = 0, bk = 0;
    bool marching = true;
    if constexpr (!EXHAUSTIVE)
    {
        if (!(M.min_dist > 0.0f)) marching = false;             // dist < min_dist is never true
        else if (P.nblk > kDistSmallBlocks) bk = morton_block(P, ox, oy, oz) * kDistBlock;
    }
    // (per lane: the wave runs the loop while any lane is in it, the lanes that left masked off)
    for (uint32_t s = 0; marching && s < M.max_steps; s++)
    {
        const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
        dist = rtd::kFltMax;
        tri = rtd::kNoTri;
        if constexpr (EXHAUSTIVE) eval_all(P, px, py, pz, dist, tri, bk);
        else
        {
            const float pmax = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
            const float margin = 1e-5f * (pmax + P.scene_scale);
#if RT_MARCH_STOP
            {
                const float wx = px - fminf(fmaxf(px, P.vmin[0]), M.vmax[0]);
                const float wy = py - fminf(fmaxf(py, P.vmin[1]), M.vmax[1]);
                const float wz = pz - fminf(fmaxf(pz, P.vmin[2]), M.vmax[2]);
                const float db = __builtin_sqrtf(wx * wx + wy * wy + wz * wz);
                const float rate = dx * wx + dy * wy + dz * wz;
                const float thr = (2e-5f * (fabsf(dx) + fabsf(dy) + fabsf(dz))) * db;
                const float err = 2.5e-7f * (fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz)) + 2.0f * pmax);
                if (db > 1.00001f * ((margin + M.min_dist) + err) && db <= rtd::kFltMax && rate >= thr &&
                    rate <= rtd::kFltMax && thr >= kFltMin)
                    break;                                          // a proven MISS
            }
#endif
            if (P.nblk <= kDistSmallBlocks) eval_all(P, px, py, pz, dist, tri, bk);
            else
            {
#if RT_MARCH_SEED
                const uint32_t sb = bk / kDistBlock;
#else
                const uint32_t sb = morton_block(P, px, py, pz);
#endif
                const uint32_t k1 = min(sb * kDistBlock + kDistBlock, P.ntris);
                for (uint32_t j = sb * kDistBlock; j < k1; j++)
                {
                    const float4 *r = P.tri_dist + 6 * size_t(j);
                    const float d = rtd::dist_point_tri(px, py, pz, r[0], r[1], r[2], r[3], r[4], r[5]);
                    take(d, P.tri_idx[j], j, dist, tri, bk);
                }
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
        }
        t += dist;
        if (dist < M.min_dist)
        {
            steps = s + 1;
            break;
        }
    }
    // a MISS is t = 0, dist = 0, tri = 0xFFFFFFFF, steps = 0
    const bool hit = steps != 0;
    uint2 *o = M.out + 2 * size_t(i);                          // (d_out is 8-byte aligned: two stores)
    o[0] = make_uint2(__float_as_uint(hit ? t : 0.0f), __float_as_uint(hit ? dist : 0.0f));
    o[1] = make_uint2(hit ? tri : rtd::kNoTri, steps);
}

} // namespace

march_fn march_rays_kernel(bool exhaustive)
{
    return exhaustive ? k_march_rays<true> : k_march_rays<false>;
}

} // namespace rtk
