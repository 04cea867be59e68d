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

// rays, order, tminmax: rt_ray_common.h (ray_slot, load_ray, load_interval).  occluded[i] = 1 / 0.
template <int VAR>
__global__ void __launch_bounds__(kWG) k_occluded_rays(KParams P, const float2 *rays, const float2 *tminmax,
                                                       const unsigned long long *order, uint32_t n, uint8_t *occluded)
{
    static_assert((VAR & kVarAnyHit) != 0 && (VAR & kVarRays) != 0, "the any-hit walk of caller-supplied rays");
    uint32_t i;
    if (!ray_slot(order, n, i)) return;
    float ox, oy, oz, dx, dy, dz, tmin, tmax;
    load_ray(rays, i, ox, oy, oz, dx, dy, dz);
    load_interval(tminmax, i, tmin, tmax);
    bool hit = false;
    // 0 without a walk: a non-finite ray (as rt_trace_rays_device), a NaN bound, an empty interval -- the one
    // compare tmin < tmax is false for all of the last two
    if (RT_FINITE_RAY(ox, oy, oz, dx, dy, dz) && tmin < tmax)
        hit = rcp_vote<VAR>(dx, dy, dz, [&](auto v) {
            return occlusion_walk<decltype(v)::value>(P, ox, oy, oz, dx, dy, dz, tmin, tmax);
        });
    occluded[i] = hit ? uint8_t(1) : uint8_t(0);
}

} // namespace

occluded_fn occluded_rays_kernel(int var)
{
    return ray_variant<kVarAnyHit>(var, [](auto v) -> occluded_fn { return k_occluded_rays<decltype(v)::value>; });
}

} // namespace rtk
