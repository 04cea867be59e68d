// rt_ray_common.h -- the one lane skeleton of the ray-query translation units (rt_rays.hip: rt_trace_rays_device;
// rt_occlusion.hip: rt_occluded_rays_device; rt_crossings.hip: rt_crossing_rays_device; rt_ao.hip:
// rt_render_ao_device) beside rt_walk.h's walk.  DESIGN.md §4.37.  A ray-query kernel is
//     ray_slot -> load_ray [-> load_interval] -> RT_FINITE_RAY -> rcp_vote<VAR>(its walk) -> its own store
// and its `*_kernel(int var)` lookup is ray_variant<its extra bit>(var, its kernel template).  What a kernel writes
// itself is its payload: the walk it calls and the record it stores.
#pragma once
#include <type_traits>

#include "rt_cam_bound.h"
#include "rt_walk.h"

namespace rtk {
namespace {

// One class test per component: anything but NaN and +-inf (v_cmp_class_f32; mask bits 3-8: the
// normal, subnormal and zero classes of either sign).
__device__ __forceinline__ bool finite_f32(float x)
{
    return __builtin_amdgcn_classf(x, 0x1F8);
}

// kVarFastRcp for rays: rt_scene::rcp_safe bounds |e1|_1 |e2|_1 below 2^120, which keeps
// |det| = |e1 . (d x e2)| <= 2 |d|_inf |e1|_1 |e2|_1 inside rcp_nr's exact range (< 2^126) for a
// direction of |d|_inf <= kRcpMaxDir with a factor of 4 to spare for the roundings.  d is used as the caller
// passes it, so a wave that holds a longer direction takes the same walk with the correctly rounded division
// instead (a wave-uniform choice: same bits).
// The render kernels take no such vote.  Their directions are the frame's camera rays, whose length is whatever
// rt_frame.cam's 3x3 makes it (the direction is normalised before the matrix, rtd::dir_from_xy): an
// orthonormal camera's are far inside, and for any other the host bounds |d|_inf per frame from the matrix
// (rt_cam_bound.h) and launches the instantiation without kVarFastRcp when the bound exceeds kRcpMaxDir
// (rt_launch.hip, frame_traversal_bits).
constexpr float kRcpMaxDir = 8.0f;
static_assert(double(kRcpMaxDir) == kCamRcpMaxDir, "rt_cam_bound.h bounds camera directions against kRcpMaxDir");

// RT_RAYS_SORT: a ray's sort word is index << kKeyBits | key (rt_rays.hip, k_ray_keys)
constexpr uint32_t kKeyBits = 32;

// the ray kernels' variants: kRaysBase [| kVarFastRcp] [| kRaysBox] (rt_launch.hip scene_traversal_bits)
constexpr int kRaysBase = kVarRays | kVarWaveGate | kVarDistSkip;
constexpr int kRaysBox = kVarPackedRem | kVarSkipRun;

// The slot of a lane: lane k of the launch takes ray k, or with RT_RAYS_SORT's sorted words ray order[k] >> kKeyBits,
// and writes that ray's outputs, so the results land in input order whatever the order they are traced in.  False
// for the tail wave's extra lanes and for a sort word that indexes past the arrays (never, for a permutation).
__device__ __forceinline__ bool ray_slot(const unsigned long long *order, uint32_t n, uint32_t& i)
{
    const uint32_t k = blockIdx.x * kWG + threadIdx.x;
    if (k >= n) return false;
    i = order ? uint32_t(order[k] >> kKeyBits) : k;
    return i < n;
}

// rays: rt_ray as three 8-byte words ({ox, oy} {oz, dx} {dy, dz}: the ABI asks for 8-byte alignment)
__device__ __forceinline__ void load_ray(const float2 *rays, uint32_t i, float& ox, float& oy, float& oz, float& dx,
                                         float& dy, float& dz)
{
    const float2 *rp = rays + size_t(i) * 3u;
    const float2 a = rp[0], b = rp[1], c = rp[2];
    ox = a.x, oy = a.y, oz = b.x, dx = b.y, dy = c.x, dz = c.y;
}

// tminmax: (tmin, tmax) per ray, or null = (-inf, +inf)
__device__ __forceinline__ void load_interval(const float2 *tminmax, uint32_t i, float& tmin, float& tmax)
{
    tmin = -__builtin_inff(), tmax = __builtin_inff();
    if (tminmax)
    {
        const float2 m = tminmax[i];
        tmin = m.x;
        tmax = m.y;
    }
}

// A non-finite ray is a miss without a walk (include/rt_tracer.h).  A macro, so that the six tests stand in the
// kernel's own condition: as a function they are simplified on their own first, into one and-chain, and the kernel
// that inlines it branches and allocates its registers otherwise than the one that spells them out (§4.37).
#define RT_FINITE_RAY(ox, oy, oz, dx, dy, dz) \
    (finite_f32(ox) && finite_f32(oy) && finite_f32(oz) && finite_f32(dx) && finite_f32(dy) && finite_f32(dz))

// a variant word as a compile-time tag: what rcp_vote and ray_variant hand their callable
template <int VAR>
using VarTag = std::integral_constant<int, VAR>;

// The wave's vote between the Newton reciprocal and the division (kRcpMaxDir above): walk(VarTag<V>) runs the
// caller's walk<V> and RETURNS its result, V = VAR while every lane's |d|_inf is in range, else VAR without
// kVarFastRcp.  (A walk whose result the callable assigns through a by-reference capture instead compiles to
// other code; crossing_walk, whose two counters are reference arguments to begin with, returns nothing: §4.37.)
template <int VAR, class Walk>
__device__ __forceinline__ auto rcp_vote(float dx, float dy, float dz, Walk walk)
{
    if constexpr ((VAR & kVarFastRcp) != 0)
    {
        const float dm = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
        if (wave_all(dm <= kRcpMaxDir))
            return walk(VarTag<VAR>{});
        else
            return walk(VarTag<VAR & ~kVarFastRcp>{});
    }
    else
        return walk(VarTag<VAR>{});
}

// The variant table of a ray kernel: the four words the host forms (kRaysBase | scene_traversal_bits, plus the
// kernel's own EXTRA bit) to pick(VarTag<word>) = that instantiation; null for any other word.
template <int EXTRA, class Pick>
auto ray_variant(int var, Pick pick) -> decltype(pick(VarTag<EXTRA | kRaysBase>{}))
{
    switch (var)
    {
    case EXTRA | kRaysBase | kVarFastRcp | kRaysBox: return pick(VarTag<EXTRA | kRaysBase | kVarFastRcp | kRaysBox>{});
    case EXTRA | kRaysBase | kRaysBox: return pick(VarTag<EXTRA | kRaysBase | kRaysBox>{});
    case EXTRA | kRaysBase | kVarFastRcp: return pick(VarTag<EXTRA | kRaysBase | kVarFastRcp>{});
    case EXTRA | kRaysBase: return pick(VarTag<EXTRA | kRaysBase>{});
    default: return nullptr;
    }
}

// The closest-hit walk of one caller-supplied ray (k_trace_rays' fast arm; k_render_ao's camera ray): the stateless
// walk over the scene's 48-byte reference records
template <int VAR>
__device__ __forceinline__ bool rays_walk(const KParams& P, float ox, float oy, float oz, float dx, float dy, float dz,
                                          float& t, float& u, float& v, uint32_t& tri)
{
    uint32_t voxel = rtd::kNoTri, steps = 0, tests = 0;
    return grid_intersect<false, RT_TRI_MOLLER_TRUMBORE, VAR>(P, ox, oy, oz, dx, dy, dz, t, u, v, tri, voxel, steps, tests);
}

// The any-hit walk of one ray over (tmin, tmax) (k_occluded_rays; k_render_ao's AO rays): VAR carries kVarAnyHit
template <int VAR>
__device__ __forceinline__ bool occlusion_walk(const KParams& P, float ox, float oy, float oz, float dx, float dy, float dz,
                                               float tmin, float tmax)
{
    float t = tmax, u = 0.0f, v = 0.0f;            // t carries tmax into the walk (grid_intersect)
    uint32_t tri = rtd::kNoTri, voxel = rtd::kNoTri, steps = 0, tests = 0;
    return grid_intersect<false, RT_TRI_MOLLER_TRUMBORE, VAR>(P, ox, oy, oz, dx, dy, dz, t, u, v, tri, voxel, steps, tests,
                                                              tmin);
}

// The counting walk of one ray over (tmin, tmax) (k_cross_rays): VAR carries kVarCross; count and front enter as 0
template <int VAR>
__device__ __forceinline__ void crossing_walk(const KParams& P, float ox, float oy, float oz, float dx, float dy, float dz,
                                              float tmin, float tmax, uint32_t& count, uint32_t& front)
{
    float t = tmax, u = 0.0f, v = 0.0f;            // t carries tmax into the walk (grid_intersect)
    uint32_t voxel = rtd::kNoTri, steps = 0;
    (void)grid_intersect<false, RT_TRI_MOLLER_TRUMBORE, VAR>(P, ox, oy, oz, dx, dy, dz, t, u, v, count, voxel, steps, front,
                                                             tmin);
}

} // namespace
} // namespace rtk
