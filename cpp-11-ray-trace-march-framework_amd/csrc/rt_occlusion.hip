// rt_occlusion.hip -- the occlusion-query kernels of librt_tracer.so for gfx950 (MI355X): the any-hit walk of
// rt_occluded_rays_device (include/rt_tracer.h) -- Grid::Intersect (grid.cpp:159-281) over a
// per-ray interval (tmin, tmax) that ends at the first test that counts.
//
// One ray per lane, as rt_rays.hip's k_trace_rays, with the same variants chosen the same way (the scene's
// traversal bits, and the wave's vote between the Newton reciprocal and the division at |d|_inf <= 8); the
// walk is rt_walk.h's grid_intersect with kVarAnyHit, which says what the bit changes.  One byte per ray goes
// out.  Everything here reads only arrays rt_scene_create wrote once.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_ray_common.h"

namespace rtk {
namespace {

// rays, order: as k_trace_rays.  tminmax: (tmin, tmax) per ray, or null = (-inf, +inf).  occluded[i] = 1 / 0.
template <int VAR>
__global__ void __launch_bounds__(kWG) k_occluded_rays(KParams P, const float2 *rays, const float2 *tminmax,
                                                       const unsigned long long *order, uint32_t n, uint8_t *occluded)
{
    static_assert((VAR & kVarAnyHit) != 0 && (VAR & kVarRays) != 0, "the any-hit walk of caller-supplied rays");
    const uint32_t k = blockIdx.x * kWG + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = order ? uint32_t(order[k] >> kKeyBits) : k;
    if (i >= n) return;             // (never, for a permutation: no sort word may index past the arrays)
    const float2 *rp = rays + size_t(i) * 3u;
    const float2 a = rp[0], b = rp[1], c = rp[2];
    const float ox = a.x, oy = a.y, oz = b.x, dx = b.y, dy = c.x, dz = c.y;
    float tmin = -__builtin_inff(), tmax = __builtin_inff();
    if (tminmax)
    {
        const float2 m = tminmax[i];
        tmin = m.x;
        tmax = m.y;
    }
    bool hit = false;
    // 0 without a walk: a non-finite ray (as rt_trace_rays_device), a NaN bound, an empty interval -- the one
    // compare tmin < tmax is false for all of the last two
    if (finite_f32(ox) && finite_f32(oy) && finite_f32(oz) && finite_f32(dx) && finite_f32(dy) && finite_f32(dz) &&
        tmin < tmax)
    {
        if constexpr ((VAR & kVarFastRcp) != 0)
        {
            const float dm = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
            if (wave_all(dm <= kRcpMaxDir))
                hit = occlusion_walk<VAR>(P, ox, oy, oz, dx, dy, dz, tmin, tmax);
            else
                hit = occlusion_walk<VAR & ~kVarFastRcp>(P, ox, oy, oz, dx, dy, dz, tmin, tmax);
        }
        else
            hit = occlusion_walk<VAR>(P, ox, oy, oz, dx, dy, dz, tmin, tmax);
    }
    occluded[i] = hit ? uint8_t(1) : uint8_t(0);
}

} // namespace

occluded_fn occluded_rays_kernel(int var)
{
    switch (var)
    {
    case kVarAnyHit | kRaysBase | kVarFastRcp | kRaysBox: return k_occluded_rays<kVarAnyHit | kRaysBase | kVarFastRcp | kRaysBox>;
    case kVarAnyHit | kRaysBase | kRaysBox: return k_occluded_rays<kVarAnyHit | kRaysBase | kRaysBox>;
    case kVarAnyHit | kRaysBase | kVarFastRcp: return k_occluded_rays<kVarAnyHit | kRaysBase | kVarFastRcp>;
    case kVarAnyHit | kRaysBase: return k_occluded_rays<kVarAnyHit | kRaysBase>;
    default: return nullptr;
    }
}

} // namespace rtk
