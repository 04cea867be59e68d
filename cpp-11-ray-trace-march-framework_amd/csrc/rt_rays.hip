// rt_rays.hip -- the ray-query kernels of librt_tracer.so for gfx950 (MI355X): Grid::Intersect
// (grid.cpp:159-281) for rays the caller supplies (rt_trace_rays_device), and the camera's own rays
// written out as such (rt_primary_rays_device).  DESIGN.md §4.27.
//
// One ray per lane; a wave takes 64 consecutive rays of the input and the tail wave masks its extra
// lanes.  The walk is rt_walk.h's grid_intersect, the code the render kernels run, with two
// differences that follow from rays that share neither an origin nor their cells:
//   * no per-camera-origin records (frefs, kVarOriginPre) and no wave-uniform list loop
//     (kVarUniform): the record test reads the scene's 48-byte reference records and forms tvec and
//     qvec per ray (triangle.h:82, 90) -- rtd::ray_tri_mt_gated, wave-gated on its det / u half;
//   * kVarRays: the box-run walk stays in its per-lane phase (see the loop in grid_intersect, where
//     the "no input can hang the GPU" argument is written down for it).
// Everything here reads only arrays rt_scene_create wrote once: the launches need no ordering against
// the scene's render launches.  (RT_RAYS_SORT alone has state: its sort words live in scratch kept on the
// scene, which rt_trace_rays_device orders between sorted calls.)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_ray_common.h"

namespace rtk {
namespace {

// RT_RAYS_SORT: a ray's sort word is index << kKeyBits | key, sorted by its low kKeyBits bits (stable: equal
// keys keep input order).  key = direction octant << 27 | Morton code of the clamped entry cell (9 bits an
// axis; a longer axis drops its low bits, `shift`); a ray that misses the grid box, or is not finite, gets
// the largest key (kMissKey: above every octant's).  Any key is a valid one: the order only decides which
// rays share a wave.  The key field is 32 bits -- four WHOLE 8-bit digits of the radix sort, which reads
// whole digits: no bit of the index is ever part of a digit -- and the index (n < 2^31) sits above it.
constexpr uint32_t kMissKey = 0x7FFFFFFFu;

__device__ __forceinline__ uint32_t spread3(uint32_t v)      // 9 bits -> every third bit
{
    v &= 0x1FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// rays, order: rt_ray_common.h (ray_slot, load_ray).
// COUNT: the counting walk of k_trace_records with its full record; else the fast arm (VAR).
template <int VAR, bool COUNT>
__global__ void __launch_bounds__(kWG) k_trace_rays(KParams P, const float2 *rays, const unsigned long long *order,
                                                    uint32_t n, rt_ray_hit *hits, rt_sample_rec *recs)
{
    uint32_t i;
    if (!ray_slot(order, n, i)) return;
    float ox, oy, oz, dx, dy, dz;
    load_ray(rays, i, ox, oy, oz, dx, dy, dz);
    float t = 0.0f, u = 0.0f, v = 0.0f;
    uint32_t tri = rtd::kNoTri, voxel = rtd::kNoTri, steps = 0, tests = 0;
    bool hit = false;
    if (RT_FINITE_RAY(ox, oy, oz, dx, dy, dz))
    {
        if constexpr (COUNT)
            hit = grid_intersect<true, RT_TRI_MOLLER_TRUMBORE, kVarWaveGate | kVarDistSkip>(P, ox, oy, oz, dx, dy, dz, t, u,
                                                                                           v, tri, voxel, steps, tests);
        else
            hit = rcp_vote<VAR>(dx, dy, dz, [&](auto w) {
                return rays_walk<decltype(w)::value>(P, ox, oy, oz, dx, dy, dz, t, u, v, tri);
            });
    }
    if (hits)
    {
        float4 o;
        o.x = __uint_as_float(hit ? tri : rtd::kNoTri);
        o.y = hit ? t : 0.0f;
        o.z = hit ? u : 0.0f;
        o.w = hit ? v : 0.0f;
        // two 8-byte stores: the ABI asks for 8-byte, not 16-byte, alignment
        float2 *hp = reinterpret_cast<float2 *>(hits + i);
        hp[0] = make_float2(o.x, o.y);
        hp[1] = make_float2(o.z, o.w);
    }
    if constexpr (COUNT)
    {
        // rt_sample_rec word by word: hit, tri | voxel, steps | tests, t | u, v | r, g | b, pad (8-byte
        // stores, as above)
        uint2 *dst = reinterpret_cast<uint2 *>(recs + i);
        dst[0] = make_uint2(hit ? 1u : 0u, hit ? tri : rtd::kNoTri);
        dst[1] = make_uint2(voxel, steps);
        dst[2] = make_uint2(tests, hit ? __float_as_uint(t) : 0u);
        dst[3] = make_uint2(hit ? __float_as_uint(u) : 0u, hit ? __float_as_uint(v) : 0u);
        dst[4] = make_uint2(0u, 0u);
        dst[5] = make_uint2(0u, 0u);
    }
}

// RT_RAYS_SORT: the sort word of every ray (above); the entry cell is dda_setup's, the walk's own start
__global__ void __launch_bounds__(kWG) k_ray_keys(KParams P, const float2 *rays, uint32_t n, uint32_t shift,
                                                  unsigned long long *keys)
{
    const uint32_t i = blockIdx.x * kWG + threadIdx.x;
    if (i >= n) return;
    float ox, oy, oz, dx, dy, dz;
    load_ray(rays, i, ox, oy, oz, dx, dy, dz);
    uint32_t key = kMissKey;
    if (RT_FINITE_RAY(ox, oy, oz, dx, dy, dz))
    {
        float nct0, nct1, nct2, dt0, dt1, dt2;
        int rem0, rem1, rem2, cs0, cs1, cs2, cell;
        if (dda_setup(P, ox, oy, oz, dx, dy, dz, nct0, nct1, nct2, dt0, dt1, dt2, rem0, rem1, rem2, cs0, cs1, cs2, cell))
        {
            // GridIdx = x + z * dims[0] + y * dims[0] * dims[2] (grid.h:41-42)
            const uint32_t uc = uint32_t(cell), y = uc / uint32_t(P.dxdz), r = uc - y * uint32_t(P.dxdz);
            const uint32_t z = r / uint32_t(P.dim[0]), x = r - z * uint32_t(P.dim[0]);
            const uint32_t o = uint32_t(dx < 0.0f) | (uint32_t(dy < 0.0f) << 1) | (uint32_t(dz < 0.0f) << 2);
            key = (o << 27) | spread3(x >> shift) | (spread3(y >> shift) << 1) | (spread3(z >> shift) << 2);
        }
    }
    keys[i] = ((unsigned long long)i << kKeyBits) | key;
}

// rt_primary_rays_device: ray i = (y, x, sample) of the frame, origin P.org and the direction the render
// kernels form (trace_sample: rtd::dir_from_xy over the frame's tables)
__global__ void __launch_bounds__(kWG) k_primary_rays(KParams P, float2 *rays, uint32_t n)
{
    const uint32_t i = blockIdx.x * kWG + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = i % P.spp, pix = i / P.spp;
    const uint32_t x = pix % P.W, y = pix / P.W;
    float dx, dy, dz;
    rtd::dir_from_xy(P.m, P.ndcx[x * P.spp + s], P.ndcy[y * P.spp + s], dx, dy, dz);
    float2 *rp = rays + size_t(i) * 3u;
    rp[0] = make_float2(P.org[0], P.org[1]);
    rp[1] = make_float2(P.org[2], dx);
    rp[2] = make_float2(dy, dz);
}

} // namespace

rays_fn trace_rays_kernel(int var, bool count)
{
    if (count) return k_trace_rays<0, true>;
    return ray_variant<0>(var, [](auto v) -> rays_fn { return k_trace_rays<decltype(v)::value, false>; });
}

primary_fn primary_rays_kernel() { return k_primary_rays; }
ray_keys_fn ray_keys_kernel() { return k_ray_keys; }
uint32_t ray_key_bits() { return kKeyBits; }

} // namespace rtk
