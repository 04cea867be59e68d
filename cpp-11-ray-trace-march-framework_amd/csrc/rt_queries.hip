// rt_queries.hip -- the query entry points of librt_tracer.so (include/rt_tracer.h): per-sample records of a frame
// rectangle (rt_trace_samples), caller-supplied rays (rt_trace_rays_device), occlusion (rt_occluded_rays_device),
// crossings (rt_crossing_rays_device), point distances (rt_distance_points_device), marches (rt_march_rays_device), a
// frame's primary rays (rt_primary_rays_device) and AO frames (rt_render_ao_device).  Kernels: rt_kernels.hip,
// rt_rays.hip, rt_occlusion.hip, rt_crossings.hip, rt_distance.hip, rt_march.hip, rt_ao.hip.
// What they share with the render launches (rt_launch.hip) is declared in rt_launch.h.

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/rt_tracer.h"
#include "rt_device.h"
#include "rt_launch.h"

using namespace rtk;

namespace {
// The parameters of a query: the scene's arrays and grid constants as rt_scene_create wrote them -- with a frame
// (AO), the frame's too -- and no per-camera-origin state, which is not these paths'
void query_params(const rt_scene *s, KParams& P, const rt_frame *f = nullptr)
{
    if (f)
        frame_params(s, f, P);
    else
    {
        std::memset(&P, 0, sizeof(P));
        scene_params(s, P);
    }
    P.frefs = nullptr;
    P.gates = nullptr;
}

// One lane of a query per input element
inline dim3 lane_grid(uint32_t n) { return dim3((n + kWG - 1) / kWG); }

// The ray queries' sort words (RT_RAYS_SORT, RT_MARCH_SORT): k_ray_keys' on st, to be sorted by ray_key_bits() bits
int fill_ray_keys(const rt_scene *s, const KParams& P, const float2 *rays, uint32_t n, hipStream_t st,
                  unsigned long long *keys)
{
    // cells per axis beyond 512 drop their low bits from the key (9 bits an axis)
    uint32_t shift = 0;
    while ((std::max(std::max(s->dims[0], s->dims[1]), s->dims[2]) - 1u) >> shift >= 512u) shift++;
    hipLaunchKernelGGL(ray_keys_kernel(), lane_grid(n), dim3(kWG), 0, st, P, rays, n, shift, keys);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// The sort scratch's last use: the event a later sorted call on another stream waits for
int rays_sorted_done(rt_scene *s, hipStream_t st)
{
    RT_HIP(hipEventRecord(s->rays_ev, st));
    s->rays_stream = st;
    s->rays_ev_recorded = true;
    return RT_OK;
}

// The launch of every query over n caller-supplied elements, after its entry point has checked its arguments, called
// ensure_device and filled its parameters.  launch(order) launches the query kernel on st reading its input through
// `order` (null: in input order).
//
// Unsorted: that launch and nothing else -- no lock, no event: the kernel reads only what rt_scene_create wrote, so it
// is ordered against nothing but its own stream.
//
// Sorted (RT_RAYS_SORT / RT_DIST_SORT / RT_MARCH_SORT), under the scene's mutex: fill_keys(keys) launches the kernel
// that writes the n sort words on st, the grid build's radix sort orders them by their low key_bits bits, and
// launch(sorted) reads the input through them.  The scratch is the scene's and is the one piece of state the queries
// have: sorted calls are serialised by the scene's mutex, and one on another stream than the last waits for it
// (rays_ev).  It grows -- a free and an allocation, which wait for the device -- only when n exceeds every earlier
// sorted n.  rays_sorted_done, after the kernel's launch, marks the scratch's last use.
template <class Keys, class Launch>
int launch_query(rt_scene *s, hipStream_t st, uint32_t n, bool sort, uint32_t key_bits, Keys fill_keys, Launch launch)
{
    if (!sort)
    {
        launch(static_cast<const unsigned long long *>(nullptr));
        RT_HIP(hipGetLastError());
        return RT_OK;
    }
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->rays_ev) RT_HIP(hipEventCreateWithFlags(&s->rays_ev, s->ev_order_flags));
    if (s->rays_ev_recorded && st != s->rays_stream) RT_HIP(hipStreamWaitEvent(st, s->rays_ev, 0));
    unsigned long long *keys = nullptr, *sorted = nullptr;
    if (int rc = rt_internal_sort_reserve(&s->rays_sort, n, &keys)) return rc;
    if (int rc = fill_keys(keys)) return rc;
    if (int rc = rt_internal_sort_run(s->rays_sort, st, n, key_bits, &sorted)) return rc;
    launch(static_cast<const unsigned long long *>(sorted));
    RT_HIP(hipGetLastError());
    return rays_sorted_done(s, st);
}

// The scene's distance arrays (rt_dist_tree.h) as rt_scene_create wrote them: what the distance and march kernels share
void dist_params(const rt_scene *s, KDist& D)
{
    std::memset(&D, 0, sizeof(D));
    D.tri_dist = s->d_tridist;
    D.tri_idx = s->d_distidx;
    D.blk = s->d_distblk;
    D.blk_key = s->d_distkey;
    D.nodes = s->d_distnodes;
    D.ntris = s->ntris;
    D.nblk = s->ndist_blk;
    D.nlevels = s->dist_levels;
    for (uint32_t l = 0; l < kDistLevels; l++)
    {
        D.lvl_off[l] = s->dist_lvl_off[l];
        D.lvl_n[l] = s->dist_lvl_n[l];
    }
    D.scene_scale = s->scene_scale;
    for (int a = 0; a < 3; a++)
    {
        const float ext = s->vmax[a] - s->vmin[a];
        D.vmin[a] = s->vmin[a];
        D.vinv[a] = ext > 0.0f && 1024.0f / ext <= rtd::kFltMax ? 1024.0f / ext : 0.0f;
    }
}
} // namespace

extern "C" {

int rt_trace_samples(rt_scene *s, const rt_frame *f, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                     rt_sample_rec *out)
{
    if (!s || !out) return fail(RT_E_INVALID, "NULL argument");
    int rc = validate_frame(f);
    if (rc) return rc;
    if (w == 0 || h == 0 || x0 + w > f->width || y0 + h > f->height)
        return fail(RT_E_INVALID, "rectangle outside the frame");
    std::lock_guard<std::mutex> lk(s->mtx);
    if ((rc = ensure_device(s))) return rc;
    const uint32_t spp = std::max(1u, f->spp);
    if ((rc = prepare_samples(s, f, spp))) return rc;
    const uint64_t n64 = uint64_t(w) * h * spp;
    if (n64 > (1ull << 28)) return fail(RT_E_INVALID, "too many samples for one record call");
    const uint32_t n = uint32_t(n64);
    rt_sample_rec *d_rec = nullptr;
    RT_HIP(hipMalloc(&d_rec, sizeof(rt_sample_rec) * n));
    KParams P;
    frame_params(s, f, P);
    set_records(P, RecOut{ d_rec, x0, y0, w, h });
    if (P.isect == RT_ISECT_RAY_MARCH && (f->kernel & RT_KERNEL_FLAG_EXHAUSTIVE)) P.isect += 0x100;
    if ((rc = flush_tables(s, s->stream)))
    {
        (void)hipFree(d_rec);
        return rc;
    }
    hipLaunchKernelGGL(trace_records_kernel(), dim3((n + kWG - 1) / kWG), dim3(kWG), 0, s->stream, P, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_rec, sizeof(rt_sample_rec) * n, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    (void)hipFree(d_rec);
    if (e != hipSuccess) return fail(RT_E_HIP, std::string("rt_trace_samples: ") + hipGetErrorString(e));
    return RT_OK;
}

// Every argument is checked before the scene is touched.  Without RT_RAYS_SORT no lock and no events: the
// launch reads only what rt_scene_create wrote (scene_params), so it is ordered against nothing but its
// own stream.
int rt_trace_rays_device(rt_scene *s, const rt_ray *d_rays, uint32_t n, uint32_t flags, rt_ray_hit *d_hits,
                         rt_sample_rec *d_recs, void *hip_stream)
{
    if (!s) return fail(RT_E_INVALID, "scene is NULL");
    if (flags & ~uint32_t(RT_RAYS_COUNT | RT_RAYS_SORT)) return fail(RT_E_INVALID, "unknown rt_rays_flags bit");
    const bool count = (flags & RT_RAYS_COUNT) != 0u, sort = (flags & RT_RAYS_SORT) != 0u;
    if (count && !d_recs) return fail(RT_E_INVALID, "RT_RAYS_COUNT needs d_recs");
    if (!count && d_recs) return fail(RT_E_INVALID, "d_recs without RT_RAYS_COUNT");
    if (n >= 0x80000000u) return fail(RT_E_INVALID, "n must be below 2^31");
    if (n == 0) return RT_OK;
    if (!d_rays) return fail(RT_E_INVALID, "d_rays is NULL");
    if (!count && !d_hits) return fail(RT_E_INVALID, "d_hits is NULL");
    if ((uintptr_t(d_rays) | uintptr_t(d_hits) | uintptr_t(d_recs)) & 7u)
        return fail(RT_E_INVALID, "d_rays, d_hits and d_recs must be 8-byte aligned");
    if (int rc = ensure_device(s)) return rc;
    KParams P;
    query_params(s, P);
    // the fast arm's walk: the box runs where the scene has them, else the octant distance skip (a scene
    // without packed cell words walks the plain CSR ranges: grid_intersect tests P.cellw)
    const int var = kVarRays | kVarWaveGate | kVarDistSkip | scene_traversal_bits(s);
    const rays_fn fn = trace_rays_kernel(var, count);
    if (!fn) return fail(RT_E_INVALID, "kernel variant not built: " + std::to_string(var));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const float2 *rays = reinterpret_cast<const float2 *>(d_rays);
    return launch_query(
        s, st, n, sort, ray_key_bits(), [&](unsigned long long *keys) { return fill_ray_keys(s, P, rays, n, st, keys); },
        [&](const unsigned long long *order) {
            hipLaunchKernelGGL(fn, lane_grid(n), dim3(kWG), 0, st, P, rays, order, n, d_hits, d_recs);
        });
}

// Ray i is occluded iff the any-hit walk over (tmin, tmax) finds a test that counts (include/rt_tracer.h).  The
// argument rules, the variant table, the sort path and the absence of state without RT_RAYS_SORT are
// rt_trace_rays_device's.
int rt_occluded_rays_device(rt_scene *s, const rt_ray *d_rays, const float *d_tminmax, uint32_t n, uint32_t flags,
                            uint8_t *d_occluded, void *hip_stream)
{
    if (!s) return fail(RT_E_INVALID, "scene is NULL");
    if (flags & RT_RAYS_COUNT) return fail(RT_E_INVALID, "RT_RAYS_COUNT: the occlusion walk has no counting arm");
    if (flags & ~uint32_t(RT_RAYS_SORT)) return fail(RT_E_INVALID, "unknown rt_rays_flags bit");
    const bool sort = (flags & RT_RAYS_SORT) != 0u;
    if (n >= 0x80000000u) return fail(RT_E_INVALID, "n must be below 2^31");
    if (n == 0) return RT_OK;
    if (!d_rays) return fail(RT_E_INVALID, "d_rays is NULL");
    if (!d_occluded) return fail(RT_E_INVALID, "d_occluded is NULL");
    if ((uintptr_t(d_rays) | uintptr_t(d_tminmax)) & 7u)
        return fail(RT_E_INVALID, "d_rays and d_tminmax must be 8-byte aligned");
    if (int rc = ensure_device(s)) return rc;
    KParams P;
    query_params(s, P);
    const int var = kVarAnyHit | kVarRays | kVarWaveGate | kVarDistSkip | scene_traversal_bits(s);
    const occluded_fn fn = occluded_rays_kernel(var);
    if (!fn) return fail(RT_E_INVALID, "kernel variant not built: " + std::to_string(var));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const float2 *rays = reinterpret_cast<const float2 *>(d_rays);
    const float2 *tmm = reinterpret_cast<const float2 *>(d_tminmax);
    return launch_query(
        s, st, n, sort, ray_key_bits(), [&](unsigned long long *keys) { return fill_ray_keys(s, P, rays, n, st, keys); },
        [&](const unsigned long long *order) {
            hipLaunchKernelGGL(fn, lane_grid(n), dim3(kWG), 0, st, P, rays, tmm, order, n, d_occluded);
        });
}

// d_out[i] = what the counting walk over (tmin, tmax) leaves for ray i (include/rt_tracer.h; kernels:
// rt_crossings.hip).  Everything but the output record is rt_occluded_rays_device's.
int rt_crossing_rays_device(rt_scene *s, const rt_ray *d_rays, const float *d_tminmax, uint32_t n, uint32_t flags,
                            rt_ray_cross *d_out, void *hip_stream)
{
    if (!s) return fail(RT_E_INVALID, "scene is NULL");
    if (flags & RT_RAYS_COUNT) return fail(RT_E_INVALID, "RT_RAYS_COUNT: the crossing walk has no record arm");
    if (flags & ~uint32_t(RT_RAYS_SORT)) return fail(RT_E_INVALID, "unknown rt_rays_flags bit");
    const bool sort = (flags & RT_RAYS_SORT) != 0u;
    if (n >= 0x80000000u) return fail(RT_E_INVALID, "n must be below 2^31");
    if (n == 0) return RT_OK;
    if (!d_rays) return fail(RT_E_INVALID, "d_rays is NULL");
    if (!d_out) return fail(RT_E_INVALID, "d_out is NULL");
    if ((uintptr_t(d_rays) | uintptr_t(d_tminmax) | uintptr_t(d_out)) & 7u)
        return fail(RT_E_INVALID, "d_rays, d_tminmax and d_out must be 8-byte aligned");
    if (int rc = ensure_device(s)) return rc;
    KParams P;
    query_params(s, P);
    const int var = kVarCross | kVarRays | kVarWaveGate | kVarDistSkip | scene_traversal_bits(s);
    const cross_fn fn = cross_rays_kernel(var);
    if (!fn) return fail(RT_E_INVALID, "kernel variant not built: " + std::to_string(var));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const float2 *rays = reinterpret_cast<const float2 *>(d_rays);
    const float2 *tmm = reinterpret_cast<const float2 *>(d_tminmax);
    uint2 *out = reinterpret_cast<uint2 *>(d_out);
    return launch_query(
        s, st, n, sort, ray_key_bits(), [&](unsigned long long *keys) { return fill_ray_keys(s, P, rays, n, st, keys); },
        [&](const unsigned long long *order) {
            hipLaunchKernelGGL(fn, lane_grid(n), dim3(kWG), 0, st, P, rays, tmm, order, n, out);
        });
}

// DistanceBruteForce for caller-supplied points (include/rt_tracer.h; kernels: rt_distance.hip).  The argument rules,
// the sort path (the scene's sort scratch and its event, shared with the ray queries) and the absence of state
// without RT_DIST_SORT are rt_trace_rays_device's.
int rt_distance_points_device(rt_scene *s, const float *d_points, uint32_t n, uint32_t flags, rt_point_dist *d_out,
                              float *d_closest, void *hip_stream)
{
    if (!s) return fail(RT_E_INVALID, "scene is NULL");
    if (flags & ~uint32_t(RT_DIST_EXHAUSTIVE | RT_DIST_SORT)) return fail(RT_E_INVALID, "unknown rt_dist_flags bit");
    if (n >= 0x80000000u) return fail(RT_E_INVALID, "n must be below 2^31");
    if (n == 0) return RT_OK;
    if (!d_points) return fail(RT_E_INVALID, "d_points is NULL");
    if (!d_out) return fail(RT_E_INVALID, "d_out is NULL");
    if ((uintptr_t(d_points) | uintptr_t(d_closest)) & 3u)
        return fail(RT_E_INVALID, "d_points and d_closest must be 4-byte aligned");
    if (uintptr_t(d_out) & 7u) return fail(RT_E_INVALID, "d_out must be 8-byte aligned");
    if (int rc = ensure_device(s)) return rc;
    KDist D;
    dist_params(s, D);
    D.points = d_points;
    D.n = n;
    D.out = reinterpret_cast<uint2 *>(d_out);
    D.closest = d_closest;
    // A mesh of at most two blocks (64 triangles) takes the exhaustive kernel in the default arm too: the seed alone
    // is half or all of such a mesh, so the cull can only add its own cost (scene 1, 44 triangles: 0.35 ms against
    // 0.20 ms for 1.4 M points, profiles/distance_bench.json).  Same bytes either way.
    const dist_fn fn = distance_points_kernel((flags & RT_DIST_EXHAUSTIVE) != 0u || s->ndist_blk <= kDistSmallBlocks);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // RT_DIST_SORT: the same kernel reading its points through sort words of k_point_keys, all 32 key bits of them
    return launch_query(
        s, st, n, (flags & RT_DIST_SORT) != 0u, 32u,
        [&](unsigned long long *keys) {
            hipLaunchKernelGGL(point_keys_kernel(), lane_grid(n), dim3(kWG), 0, st, D, keys);
            RT_HIP(hipGetLastError());
            return int(RT_OK);
        },
        [&](const unsigned long long *order) {
            D.order = order;
            hipLaunchKernelGGL(fn, lane_grid(n), dim3(kWG), 0, st, D);
        });
}

// Renderer::RayMarch for caller-supplied rays (include/rt_tracer.h; kernel: rt_march.hip).  The argument rules, the
// sort path (RT_RAYS_SORT's own: k_ray_keys' words, the scene's sort scratch and its event) and the absence of state
// without RT_MARCH_SORT are rt_trace_rays_device's.
int rt_march_rays_device(rt_scene *s, const rt_ray *d_rays, uint32_t n, const rt_march_params *params, uint32_t flags,
                         rt_march_hit *d_out, void *hip_stream)
{
    if (!s) return fail(RT_E_INVALID, "scene is NULL");
    if (flags & ~uint32_t(RT_MARCH_EXHAUSTIVE | RT_MARCH_SORT)) return fail(RT_E_INVALID, "unknown rt_march_flags bit");
    const rt_march_params mp = params ? *params : rt_march_params{ kMarchSteps, 0.001f };
    if (mp.max_steps == 0 || mp.max_steps > kMarchMaxSteps) return fail(RT_E_INVALID, "max_steps must be in [1, 4096]");
    if (std::isnan(mp.min_dist)) return fail(RT_E_INVALID, "min_dist is NaN");
    if (n >= 0x80000000u) return fail(RT_E_INVALID, "n must be below 2^31");
    if (n == 0) return RT_OK;
    if (!d_rays) return fail(RT_E_INVALID, "d_rays is NULL");
    if (!d_out) return fail(RT_E_INVALID, "d_out is NULL");
    if ((uintptr_t(d_rays) | uintptr_t(d_out)) & 7u) return fail(RT_E_INVALID, "d_rays and d_out must be 8-byte aligned");
    if (int rc = ensure_device(s)) return rc;
    KMarch M;
    dist_params(s, M.d);
    M.d.n = n;
    M.rays = reinterpret_cast<const float2 *>(d_rays);
    M.out = reinterpret_cast<uint2 *>(d_out);
    M.max_steps = mp.max_steps;
    M.min_dist = mp.min_dist;
    for (int a = 0; a < 3; a++) M.vmax[a] = s->vmax[a];
    const march_fn fn = march_rays_kernel((flags & RT_MARCH_EXHAUSTIVE) != 0u);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // RT_MARCH_SORT: RT_RAYS_SORT's order, whose keys need the grid's parameters -- built on that path alone
    return launch_query(
        s, st, n, (flags & RT_MARCH_SORT) != 0u, ray_key_bits(),
        [&](unsigned long long *keys) {
            KParams P;
            query_params(s, P);
            return fill_ray_keys(s, P, M.rays, n, st, keys);
        },
        [&](const unsigned long long *order) {
            M.d.order = order;
            hipLaunchKernelGGL(fn, lane_grid(n), dim3(kWG), 0, st, M);
        });
}

int rt_primary_rays_device(rt_scene *s, const rt_frame *f, rt_ray *d_rays, void *hip_stream)
{
    if (!s || !d_rays) return fail(RT_E_INVALID, "NULL argument");
    if (uintptr_t(d_rays) & 7u) return fail(RT_E_INVALID, "d_rays must be 8-byte aligned");
    int rc = validate_frame(f);
    if (rc) return rc;
    const uint32_t spp = std::max(1u, f->spp);
    const uint64_t n64 = uint64_t(f->width) * f->height * spp;
    if (n64 >= 0x80000000ull) return fail(RT_E_INVALID, "more than 2^31 - 1 rays");
    std::lock_guard<std::mutex> lk(s->mtx);
    if ((rc = ensure_device(s))) return rc;
    if ((rc = prepare_samples(s, f, spp))) return rc;
    KParams P;
    frame_params(s, f, P);
    // a launch of the scene that reads its frame tables: after every launch that may still read the old
    // ones, and itself the scene's last launch (as launch_render's plain arms)
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if ((rc = begin_table_launch(s, st))) return rc;
    const uint32_t n = uint32_t(n64);
    hipLaunchKernelGGL(primary_rays_kernel(), dim3((n + kWG - 1) / kWG), dim3(kWG), 0, st, P,
                       reinterpret_cast<float2 *>(d_rays), n);
    RT_HIP(hipGetLastError());
    return mark_own(s, st);
}

// An AO frame in one launch of k_render_ao (rt_ao.hip; include/rt_tracer.h has the contract).  Every argument is
// checked before the scene is touched.  The launch is rt_primary_rays_device's kind (begin_table_launch): one of
// the scene that reads its frame tables and no per-origin records.  The directions and rotations are kernel arguments.
int rt_render_ao_device(rt_scene *s, const rt_frame *f, const rt_ao_params *ao, uint32_t *d_bgra, uint8_t *d_counts,
                        void *hip_stream)
{
    if (!s) return fail(RT_E_INVALID, "scene is NULL");
    if (!f) return fail(RT_E_INVALID, "frame is NULL");
    if (!ao) return fail(RT_E_INVALID, "ao is NULL");
    if (!d_bgra) return fail(RT_E_INVALID, "d_bgra is NULL");
    int rc = validate_frame(f);
    if (rc) return rc;
    if (ao->num_dirs == 0 || ao->num_dirs > rtk::kAoMaxDirs) return fail(RT_E_INVALID, "num_dirs must be in [1, 64]");
    if (std::isnan(ao->tmin) || std::isnan(ao->tmax)) return fail(RT_E_INVALID, "tmin / tmax is NaN");
    if (!(ao->tmin < ao->tmax)) return fail(RT_E_INVALID, "tmin must be below tmax");
    if (ao->flags & ~uint32_t(RT_AO_ROTATE)) return fail(RT_E_INVALID, "unknown rt_ao_flags bit");
    const uint32_t spp = std::max(1u, f->spp);
    if (!(is_pow2(spp) && spp <= 64)) return fail(RT_E_INVALID, "rt_render_ao_device needs spp to be a power of two <= 64");
    if (f->intersector != RT_ISECT_GRID || f->tri_test != RT_TRI_MOLLER_TRUMBORE)
        return fail(RT_E_INVALID, "rt_render_ao_device needs RT_ISECT_GRID and RT_TRI_MOLLER_TRUMBORE");
    const uint64_t n64 = uint64_t(f->width) * f->height * spp;
    if (n64 >= 0x80000000ull) return fail(RT_E_INVALID, "more than 2^31 - 1 samples");
    rtk::KAo G;
    std::memset(&G.a, 0, sizeof(G.a));
    G.a.num_dirs = ao->num_dirs;
    G.a.flags = ao->flags;
    G.a.tmin = ao->tmin;
    G.a.tmax = ao->tmax;
    G.a.counts = d_counts;
    if (ao->dirs)
    {
        for (uint32_t i = 0; i < 3u * ao->num_dirs; i++)
        {
            if (!std::isfinite(ao->dirs[i])) return fail(RT_E_INVALID, "dirs holds a non-finite entry");
            G.a.dirs[i] = ao->dirs[i];
        }
    }
    else if ((rc = rt_ao_table(ao->num_dirs, G.a.dirs)))
        return rc;
    if ((rc = rt_ao_rotations(G.a.rot))) return rc;
    std::lock_guard<std::mutex> lk(s->mtx);
    if ((rc = ensure_device(s))) return rc;
    if ((rc = prepare_samples(s, f, spp))) return rc;
    KParams& P = G.p;
    query_params(s, P, f);
    const uint32_t tiles = region_params(P, 0, 0, f->width, f->height, d_bgra, f->width, 0u);
    const uint32_t wgpt = (kTilePix * spp) / kWG;       // = spp: one wave per 64 sample slots of a tile
    const uint64_t blocks = uint64_t(tiles) * wgpt;
    if (blocks > 0x3FFFFFFFull) return fail(RT_E_INVALID, "frame too large for one launch");
    launch_shape(P, wgpt, uint32_t(blocks));            // (k_render_ao reads the tile half alone)
    const int var = kVarRays | kVarWaveGate | kVarDistSkip | scene_traversal_bits(s);
    const rtk::ao_fn fn = rtk::render_ao_kernel(var);
    if (!fn) return fail(RT_E_INVALID, "kernel variant not built: " + std::to_string(var));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if ((rc = begin_table_launch(s, st))) return rc;
    // the dispatch carries the scene's completion event, an event nothing still holds (launch_render's plain arm):
    // the predecessor's event, which order_all kept as ev_prev, stays what it was, so a capture of this call after
    // ONE warm-up queries no event recorded on the capturing stream
    hipEvent_t stop = nullptr;
    if ((rc = mark_free(s, nullptr, &stop))) return rc;
    hipExtLaunchKernelGGL(fn, dim3(uint32_t(blocks)), dim3(kWG), 0, st, nullptr, stop, 0u, G);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

} // extern "C"
