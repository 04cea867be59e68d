// rt_crossings.hip -- the crossing-query kernels of librt_tracer.so for gfx950 (MI355X): the counting walk of
// rt_crossing_rays_device (include/rt_tracer.h) -- Grid::Intersect (grid.cpp:159-281) over a
// per-ray interval (tmin, tmax) that ends at no hit: every test that lies in its own cell's interval of the walk
// counts, once, with the sign of its det.
//
// One ray per lane, as rt_occlusion.hip's k_occluded_rays, with the same variants chosen the same way (the scene's
// traversal bits, and the wave's vote between the Newton reciprocal and the division at |d|_inf <= 8); the
// walk is rt_walk.h's grid_intersect with kVarCross, which says what the bit changes.  One 8-byte record per ray
// goes out.  Everything here reads only arrays rt_scene_create wrote once.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_ray_common.h"

namespace rtk {
namespace {

// rays, order, tminmax: as k_occluded_rays.  out[i] = {count, front} (rt_ray_cross).
template <int VAR>
__global__ void __launch_bounds__(kWG) k_cross_rays(KParams P, const float2 *rays, const float2 *tminmax,
                                                    const unsigned long long *order, uint32_t n, uint2 *out)
{
    static_assert((VAR & kVarCross) != 0 && (VAR & kVarRays) != 0 && (VAR & kVarAnyHit) == 0,
                  "the counting walk of caller-supplied rays");
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
    uint32_t count = 0u, front = 0u;
    // {0, 0} without a walk: a non-finite ray, a NaN bound, an empty interval (k_occluded_rays' one compare); a ray
    // that misses the grid box leaves the walk before its first cell
    if (finite_f32(ox) && finite_f32(oy) && finite_f32(oz) && finite_f32(dx) && finite_f32(dy) && finite_f32(dz) &&
        tmin < tmax)
    {
        if constexpr ((VAR & kVarFastRcp) != 0)
        {
            const float dm = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
            if (wave_all(dm <= kRcpMaxDir))
                crossing_walk<VAR>(P, ox, oy, oz, dx, dy, dz, tmin, tmax, count, front);
            else
                crossing_walk<VAR & ~kVarFastRcp>(P, ox, oy, oz, dx, dy, dz, tmin, tmax, count, front);
        }
        else
            crossing_walk<VAR>(P, ox, oy, oz, dx, dy, dz, tmin, tmax, count, front);
    }
    out[i] = make_uint2(count, front);
}

} // namespace

cross_fn cross_rays_kernel(int var)
{
    switch (var)
    {
    case kVarCross | kRaysBase | kVarFastRcp | kRaysBox: return k_cross_rays<kVarCross | kRaysBase | kVarFastRcp | kRaysBox>;
    case kVarCross | kRaysBase | kRaysBox: return k_cross_rays<kVarCross | kRaysBase | kRaysBox>;
    case kVarCross | kRaysBase | kVarFastRcp: return k_cross_rays<kVarCross | kRaysBase | kVarFastRcp>;
    case kVarCross | kRaysBase: return k_cross_rays<kVarCross | kRaysBase>;
    default: return nullptr;
    }
}

} // namespace rtk
