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
    uint32_t i;
    if (!ray_slot(order, n, i)) return;
    float ox, oy, oz, dx, dy, dz, tmin, tmax;
    load_ray(rays, i, ox, oy, oz, dx, dy, dz);
    load_interval(tminmax, i, tmin, tmax);
    uint32_t count = 0u, front = 0u;
    // {0, 0} without a walk: a non-finite ray, a NaN bound, an empty interval (k_occluded_rays' one compare); a ray
    // that misses the grid box leaves the walk before its first cell
    if (RT_FINITE_RAY(ox, oy, oz, dx, dy, dz) && tmin < tmax)
        rcp_vote<VAR>(dx, dy, dz, [&](auto v) {
            crossing_walk<decltype(v)::value>(P, ox, oy, oz, dx, dy, dz, tmin, tmax, count, front);
        });
    out[i] = make_uint2(count, front);
}

} // namespace

cross_fn cross_rays_kernel(int var)
{
    return ray_variant<kVarCross>(var, [](auto v) -> cross_fn { return k_cross_rays<decltype(v)::value>; });
}

} // namespace rtk
