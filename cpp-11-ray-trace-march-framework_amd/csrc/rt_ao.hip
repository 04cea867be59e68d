// rt_ao.hip -- the ambient-occlusion frame kernel of librt_tracer.so for gfx950 (MI355X): rt_render_ao_device
// (include/rt_tracer.h states the contract op by op).  One launch forms the camera ray of every
// sample (k_primary_rays' bits), finds its closest hit (k_trace_rays' walk), forms K AO rays at the hit and sends
// each through the any-hit walk (k_occluded_rays'), and resolves the pixel as the render kernels do -- no ray and
// no hit goes through memory.
//
// One lane per sample; a wave takes 64 consecutive sample slots of a 16x16 tile in Morton order (process_item's
// work item), so a pixel's samples sit in adjacent lanes and the wave is spatially compact.  The AO loop is
// wave-uniform: every lane uses local direction k at the same time, which arrives by scalar loads from the
// kernel arguments.  Lanes whose camera ray missed idle through the loop; a wave with no hit lane skips it.
// Every float operation below is one f32 rounding (-ffp-contract=off, no fast-math: csrc/Makefile).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

// (the AO walks keep the guarded add chains of a per-lane run: tests/test_ao_cpu.py pins k_render_ao's registers to the
// SGPR, and the lean chains change that count -- 94 to 91 -- in the variant every shipped scene takes; rt_walk.h)
#define RT_WALK_LEAN_CHAINS false
#include "rt_item_coord.h"
#include "rt_ray_common.h"

namespace rtk {
namespace {

constexpr uint32_t kAoMiss = 0xFFu;         // the count byte of a sample whose camera ray hits nothing

// The kernel's one argument re-read from the kernarg segment (late_params' round trip through a VGPR): what the
// AO loop and the resolve read is loaded where it is used, not held in SGPRs across the walks.
__device__ __forceinline__ const KAo& late_ao()
{
    const uint64_t a = uint64_t(__builtin_amdgcn_kernarg_segment_ptr());
    uint32_t lo = uint32_t(a), hi = uint32_t(a >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    return *(const KAo *)(const __attribute__((address_space(4))) KAo *)((uint64_t(hi) << 32) | lo);
}

// Step 6 of the contract: k_occluded_rays' body for one ray -- 0 without a walk for a non-finite ray, else the
// any-hit walk, the wave voting between the Newton reciprocal and the division (same bits either way).
template <int VAR>
__device__ __forceinline__ bool ao_ray(const KParams& P, float ox, float oy, float oz, float dx, float dy, float dz,
                                       float tmin, float tmax)
{
    bool hit = false;
    if (RT_FINITE_RAY(ox, oy, oz, dx, dy, dz))
        hit = rcp_vote<VAR>(dx, dy, dz, [&](auto v) {
            return occlusion_walk<decltype(v)::value>(P, ox, oy, oz, dx, dy, dz, tmin, tmax);
        });
    return hit;
}

template <int VAR>
__global__ void __launch_bounds__(kWG) k_render_ao(KAo G)
{
    static_assert((VAR & kVarRays) != 0 && (VAR & kVarAnyHit) == 0, "the closest-hit variant; the AO rays add kVarAnyHit");
    const KParams& P = G.p;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerWG + (threadIdx.x >> 6));
    // what crosses the AO walks: the hit point (the AO rays' origin, which the walk holds anyway), the flipped
    // normal, the count and the rotation index in one word, and the tile origin (process_item's packed word)
    float px = 0.0f, py = 0.0f, pz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    uint32_t cnt = kAoMiss;                 // bits 0-7: the count (kAoMiss: no hit); bits 8-11: the rotation index j
    uint32_t origin;
    {
        const ItemCoord ic = item_coord_pre(P, item, lane);
        origin = tile_origin_word(ic);
        if (ic.valid)
        {
            // 1. the camera ray (k_primary_rays)
            float dx, dy, dz;
            rtd::dir_from_xy(P.m, P.ndcx[ic.x * P.spp + ic.s], P.ndcy[ic.y * P.spp + ic.s], dx, dy, dz);
            const float ox = P.org[0], oy = P.org[1], oz = P.org[2];
            // 2. its closest hit (k_trace_rays' fast arm)
            float t = 0.0f, u = 0.0f, v = 0.0f;
            uint32_t tri = rtd::kNoTri;
            bool hit = false;
            if (RT_FINITE_RAY(ox, oy, oz, dx, dy, dz))
                hit = rcp_vote<VAR>(dx, dy, dz, [&](auto w) {
                    return rays_walk<decltype(w)::value>(P, ox, oy, oz, dx, dy, dz, t, u, v, tri);
                });
            if (hit)
            {
                // 4. g = e1 x e2 from the triangle's {v0, e1, e2} record, n = g / |g| turned against d, p = o + t d
                const float4 a = P.tri_mt[3 * size_t(tri) + 0], b = P.tri_mt[3 * size_t(tri) + 1],
                             c = P.tri_mt[3 * size_t(tri) + 2];
                const float e1x = a.w, e1y = b.x, e1z = b.y, e2x = b.z, e2y = b.w, e2z = c.x;
                const float gx = e1y * e2z - e1z * e2y;
                const float gy = e1z * e2x - e1x * e2z;
                const float gz = e1x * e2y - e1y * e2x;
                const float len = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz);
                nx = gx / len;
                ny = gy / len;
                nz = gz / len;
                if ((nx * dx + ny * dy) + nz * dz > 0.0f)
                {
                    nx = -nx;
                    ny = -ny;
                    nz = -nz;
                }
                px = ox + t * dx;
                py = oy + t * dy;
                pz = oz + t * dz;
                cnt = (((ic.x & 3u) | ((ic.y & 3u) << 2)) ^ (ic.s & 15u)) << 8;
            }
        }
    }
    if (__builtin_amdgcn_ballot_w64((cnt & 0xFFu) != kAoMiss) != 0ull)
    {
        const AoParams& A = late_ao().a;
        const bool hitl = (cnt & 0xFFu) != kAoMiss;
        const uint32_t K = A.num_dirs;
        const bool rotate = (A.flags & RT_AO_ROTATE) != 0u;
        const float tmin = A.tmin, tmax = A.tmax;
        for (uint32_t k = 0; k < K; k++)
        {
            // (the frame below is recomputed per direction: held across the walk it is six more registers)
            asm volatile("" : "+v"(nx), "+v"(ny), "+v"(nz));
            // 5. local direction k, rotated about the normal by the sample's angle
            float lx = A.dirs[3u * k + 0u], ly = A.dirs[3u * k + 1u];
            const float lz = A.dirs[3u * k + 2u];
            if (rotate)
            {
                const uint32_t j = (cnt >> 8) & 15u;
                const float rc = A.rot[2u * j + 0u], rs = A.rot[2u * j + 1u];
                const float rx = rc * lx - rs * ly;
                const float ry = rs * lx + rc * ly;
                lx = rx;
                ly = ry;
            }
            // 4. the tangent frame of n (Duff et al. 2017, "Building an Orthonormal Basis, Revisited")
            const float sg = __builtin_copysignf(1.0f, nz);
            const float fa = -1.0f / (sg + nz);
            const float fb = (nx * ny) * fa;
            const float t1x = 1.0f + (sg * (nx * nx)) * fa, t1y = sg * fb, t1z = -(sg * nx);
            const float t2x = fb, t2y = sg + (ny * ny) * fa, t2z = -ny;
            const float wx = (lx * t1x + ly * t2x) + lz * nx;
            const float wy = (lx * t1y + ly * t2y) + lz * ny;
            const float wz = (lx * t1z + ly * t2z) + lz * nz;
            // 6. the any-hit walk of (p, w) over (tmin, tmax)
            bool occ = false;
            if (hitl) occ = ao_ray<VAR | kVarAnyHit>(P, px, py, pz, wx, wy, wz, tmin, tmax);
            cnt += occ ? 1u : 0u;
        }
    }
    const KAo& L = late_ao();
    const KParams& Q = L.p;
    const ItemCoord ic = item_coord_post(Q, item, lane, origin);
    cnt &= 0xFFu;
    // 3. / 7. the sample's colour: the background of a miss (renderer.cpp:121), else the open share of K
    const float col = cnt == kAoMiss ? float(ic.y) / float(Q.H) : float(L.a.num_dirs - cnt) / float(L.a.num_dirs);
    if (L.a.counts && ic.valid) L.a.counts[(size_t(ic.y) * Q.W + ic.x) * Q.spp + ic.s] = uint8_t(cnt);
    // 8. process_item's resolve: the pixel's samples summed in sample order across its adjacent lanes
    float sum = 0.0f;
    if (Q.spp == 4u)
        sum = quad_bcast<0>(col) + quad_bcast<1>(col) + quad_bcast<2>(col) + quad_bcast<3>(col);
    else
    {
        const uint32_t base = lane & ~(Q.spp - 1u);
        for (uint32_t k = 0; k < Q.spp; k++) sum += __shfl(col, int(base + k), 64);
    }
    if (ic.valid && ic.s == 0)
    {
        const float g = rtd::gamma_half(average(Q, sum));
        store_pixel(Q, ic.c, ic.p, ic.x, ic.y, rtd::pack_bgra8(g, g, g));
    }
}

} // namespace

ao_fn render_ao_kernel(int var)
{
    return ray_variant<0>(var, [](auto v) -> ao_fn { return k_render_ao<decltype(v)::value>; });
}

} // namespace rtk
