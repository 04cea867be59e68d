// rt_ray_common.h -- what the ray-query translation units share (rt_rays.hip: rt_trace_rays_device;
// rt_occlusion.hip: rt_occluded_rays_device; rt_crossings.hip: rt_crossing_rays_device; rt_ao.hip:
// rt_render_ao_device) beside rt_walk.h's walk.
#pragma once
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
