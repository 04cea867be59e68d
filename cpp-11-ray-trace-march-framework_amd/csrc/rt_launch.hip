// rt_launch.hip -- the launch side of librt_tracer.so's host code: the scene's events and the order of its
// launches across streams, the per-frame tables (prepare_samples) and parameters (frame_params), the per-origin
// records and miss masks, the render launches (launch_render: one frame or shard; launch_batch: n frames in one
// launch) and the entry points built on them -- frames, shards, batches, records, hit IDs, unshard, the timing
// getters and the three host copy-back paths.  What rt_queries.hip and rt_tracer.hip use of it is declared in
// rt_launch.h; DESIGN.md §4.34 says which helper a new entry point calls for what.

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rt_tracer.h"
#include "rt_device.h"
#include "rt_cam_bound.h"
#include "rt_launch.h"

namespace rtk {
namespace {
// RT_HOST_TRACE=1: the host time of a render call's phases, printed to stderr per call (a new frame
// shape's first call waits for the host; this names what it waits for)
struct HostTrace
{
    bool on = std::getenv("RT_HOST_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t0;
    char buf[512];
    int len = 0;
    void start() { if (on) { t0 = std::chrono::steady_clock::now(); len = 0; } }
    void mark(const char *what)
    {
        if (!on || len > 400) return;
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        len += std::snprintf(buf + len, sizeof(buf) - size_t(len), " %s %.1f", what, us);
    }
    void end() { if (on) std::fprintf(stderr, "rt_host_trace:%s\n", buf); }
};
HostTrace g_ht;

// A device buffer of >= n elements; growing frees the old one first (a free waits for the device)
template <class T> int grow(T *&p, size_t& cap, size_t n)
{
    if (n <= cap) return RT_OK;
    if (p) RT_HIP(hipFree(p));
    p = nullptr;
    cap = 0;
    RT_HIP(hipMalloc(&p, n * sizeof(T)));
    cap = n;
    return RT_OK;
}

// A stop event for the scene's next untimed launch: one of ev_done[] that no scene still holds as its
// ev_last / ev_prev (re-recording a held one would make that scene wait for this launch instead of
// its own), else a new one in a slot
int free_done_event(rt_scene *s, rtk::EvRef& out)
{
    for (rtk::EvRef& e : s->ev_done)
        if (e && e.use_count() == 1)
        {
            out = e;
            return RT_OK;
        }
    rtk::EvRef& slot = s->ev_done[0];
    if (int rc = new_event(slot, s->ev_time_flags)) return rc;
    out = slot;
    return RT_OK;
}

// AUTO's packed counts + empty-run loop: dims <= 512 and (box-run build) the box words exist
bool auto_runs(const rt_scene *s)
{
    return s->pack_ok && s->box_words;
}

// The same for one frame of a render launch: rt_frame.cam's 3x3 need not be orthonormal, and the direction is
// normalised BEFORE it (rtd::dir_from_xy), so the frame's directions are as long as the matrix makes them.
// kVarFastRcp's proof holds up to |d|_inf = kRcpMaxDir (rt_ray_common.h); a frame whose bound (rt_cam_bound.h,
// fp64, from the 3x3 alone) is above that or not finite takes the instantiation without the bit, the one a
// scene with rcp_safe = 0 takes.  The render kernels hold no per-wave vote for this: the choice is per frame.
int frame_traversal_bits(const rt_scene *s, const KParams& P)
{
    const int v = scene_traversal_bits(s);
    return cam_fast_rcp_ok(cam_dir_bound(P.m)) ? v : (v & ~kVarFastRcp);
}

// The record gate's per-record bound E is computed for |D_i| <= kGateDmax (rt_record_gate.h): a frame whose
// bound is above that or not finite runs without gate records, the loop of a scene created with RT_REC_GATE=0.
bool frame_gated(const rt_scene *s, const KParams& P)
{
    return s->rec_gate && cam_gate_ok(cam_dir_bound(P.m));
}

// Uploads the frame's sample table if it differs from the cached one.
// The scene's per-frame constants that live in device memory are rewritten only after its last
// launch has finished with them (launches are asynchronous; the copies are not stream-ordered).
int wait_scene_idle(rt_scene *s)
{
    if (s->ev_recorded) RT_HIP(hipEventSynchronize(s->ev_last->ev));
    if (s->ev_prev) RT_HIP(hipEventSynchronize(s->ev_prev->ev));
    s->ev_prev.reset();
    rtk::fref_ordered(s->fref);                 // nothing still reads a per-origin record buffer
    s->miss_busy = 0u;                          // ... or a miss mask
    return RT_OK;
}

// st waits for e -- unless e has already completed (a stream wait enqueues a packet that idles the
// chip for a few us even then)
hipError_t wait_unless_done(hipStream_t st, hipEvent_t e)
{
    return hipEventQuery(e) == hipSuccess ? hipSuccess : hipStreamWaitEvent(st, e, 0);
}

// Orders stream st after every launch of scene s that may still run: the last one (ev_last, implicit
// on its own stream) and, when that one overlapped its predecessor (RT_KERNEL_FLAG_OVERLAP), the
// predecessor (ev_prev).  The caller's next launch on st then follows them all.
// The last launch becomes the "launch two back" of the next one: an overlapped launch after this one
// on a third stream is ordered by nothing else.
// No earlier launch then still reads a per-origin record buffer when the caller's launch starts, so that
// launch may recompute either one (fref_ordered); a launch after it that asks to overlap it waits for
// this one's predecessors too (ev_prev above), whatever becomes of the caller's launch.
int order_all(rt_scene *s, hipStream_t st)
{
    rtk::fref_ordered(s->fref);
    s->miss_busy = 0u;                          // (the miss masks likewise)
    if (!s->ev_recorded) return RT_OK;
    if (st != s->last_stream) RT_HIP(wait_unless_done(st, s->ev_last->ev));
    if (s->ev_prev && s->prev_stream != st) RT_HIP(wait_unless_done(st, s->ev_prev->ev));
    s->ev_prev = s->ev_last;
    s->prev_stream = s->last_stream;
    return RT_OK;
}

// An overlapped launch on st (RT_KERNEL_FLAG_OVERLAP): it may run beside the scene's last launch, but
// after the one before that (at most two in flight)
int order_overlap(rt_scene *s, hipStream_t st)
{
    s->miss_busy = s->miss_last;                // the last launch's miss masks may still be read
    if (s->ev_prev && s->prev_stream != st) RT_HIP(wait_unless_done(st, s->ev_prev->ev));
    s->ev_prev = s->ev_last;
    s->prev_stream = s->last_stream;
    return RT_OK;
}

// camera.h:41-42 fov_xs = (float)tan(double(DegToRad(fov) / 2)) (H5), computed on the host
float fov_xs_of(const rt_frame *f)
{
    const float hfov = f->fov * float(0.0174532925);           // lin_alg.h:232 DegToRad
    return float(::tan(double(hfov / 2.0f)));
}

// Camera-space x per (column, sample) and y per (row, sample) of GenerateRay (camera.h:20-21,
// 40-42): the only parts of a ray's direction that depend on the pixel and the sample offsets
// alone, computed here with the kernels' own operations (rtd::cam_x / cam_y: IEEE float on the
// host too, no contraction) and uploaded when the frame shape changes.  tbl = the sample table.
std::vector<float> ndc_key(const rt_frame *f, uint32_t spp, const std::vector<float>& tbl)
{
    std::vector<float> key = { float(f->width), float(f->height), float(spp), fov_xs_of(f),
                               float(f->width) / float(f->height) };
    key.insert(key.end(), tbl.begin(), tbl.end());
    return key;
}

// the sample table of a frame (rt_frame.sample_offsets, or the Hammersley table)
std::vector<float> sample_table(const rt_frame *f, uint32_t spp)
{
    std::vector<float> tbl;
    if (f->sample_offsets)
        tbl.assign(f->sample_offsets, f->sample_offsets + 2 * size_t(spp));
    else
        hammersley(spp, tbl);
    return tbl;
}

// How a launch on st is ordered against the scene's earlier ones: after all of them (order_all), beside the last
// one (order_overlap), or by its caller (rt_render_frame_host_tiled's row bands).
enum class Order { all, overlap, callers };

// The head of every launch of the scene that reads its frame tables: ordered, the tables written, and from here
// on the scene's last launch.  The caller then says which per-origin record buffers it reads (fref_launched).
int begin_launch(rt_scene *s, hipStream_t st, Order o)
{
    if (o == Order::overlap)
    {
        if (int rc = order_overlap(s, st)) return rc;
    }
    else if (o == Order::all)
        if (int rc = order_all(s, st)) return rc;
    if (int rc = flush_tables(s, st)) return rc;
    s->last_stream = st;
    return RT_OK;
}

int prepare_ndc(rt_scene *s, const rt_frame *f, uint32_t spp, const std::vector<float>& tbl)
{
    const float fx = fov_xs_of(f), aspect = float(f->width) / float(f->height);
    std::vector<float> key = ndc_key(f, spp, tbl);
    if (key == s->ndc_key) return RT_OK;
    const size_t n = (size_t(f->width) + f->height) * spp;
    std::vector<float> h(n);
    for (uint32_t x = 0; x < f->width; x++)
        for (uint32_t k = 0; k < spp; k++) h[size_t(x) * spp + k] = rtd::cam_x(x, tbl[2 * k], f->width, fx);
    float *hy = h.data() + size_t(f->width) * spp;
    for (uint32_t y = 0; y < f->height; y++)
        for (uint32_t k = 0; k < spp; k++) hy[size_t(y) * spp + k] = rtd::cam_y(y, tbl[2 * k + 1], f->height, fx, aspect);
    if (int rc = wait_scene_idle(s)) return rc;
    s->tab_epoch++;
    if (int rc = grow(s->d_ndc, s->ndc_cap, n)) return rc;
    RT_HIP(hipMemcpy(s->d_ndc, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    s->ndc_key = key;
    s->ndc_w = f->width;
    s->ndc_spp = spp;
    return RT_OK;
}

int remember_tables(rt_scene *s, const rt_frame *f, uint32_t spp, const std::vector<float>& tbl)
{
    s->fp_w = f->width;
    s->fp_h = f->height;
    s->fp_spp = spp;
    std::memcpy(&s->fp_fov, &f->fov, 4);
    s->fp_custom = f->sample_offsets != nullptr;
    s->fp_tbl = tbl;
    s->fp_valid = true;
    return RT_OK;
}

// true when the scene's camera-space and sample tables are those of this frame (no host work)
bool tables_match(const rt_scene *s, const rt_frame *f, uint32_t spp)
{
    uint32_t fov;
    std::memcpy(&fov, &f->fov, 4);
    if (!s->fp_valid || s->fp_w != f->width || s->fp_h != f->height || s->fp_spp != spp || s->fp_fov != fov ||
        s->fp_custom != (f->sample_offsets != nullptr))
        return false;
    return !f->sample_offsets || std::memcmp(s->fp_tbl.data(), f->sample_offsets, sizeof(float) * 2 * spp) == 0;
}
} // namespace

int new_event(EvRef& r, unsigned flags)
{
    EvRef n = std::make_shared<EvHolder>();
    RT_HIP(hipEventCreateWithFlags(&n->ev, flags));
    r = std::move(n);
    return RT_OK;
}

// The traversal features that need a scene property, for the render launches (on top of kVarAutoCore)
// and for rt_trace_rays_device (on top of kVarRays): one table serves both paths.
int scene_traversal_bits(const rt_scene *s)
{
    return (s->rcp_safe ? kVarFastRcp : 0) | (auto_runs(s) ? kVarPackedRem | kVarSkipRun : 0);
}

int ensure_device(const rt_scene *s)
{
    int cur = -1;
    RT_HIP(hipGetDevice(&cur));
    if (cur != s->device) RT_HIP(hipSetDevice(s->device));
    return RT_OK;
}

// The frame tables of prepare_samples' device path, written on stream st after every launch that
// may still read the old ones (st's own, and the scene's last launch on another stream: ev1).
int flush_tables(rt_scene *s, hipStream_t st)
{
    if (!s->tab_dirty) return RT_OK;
    if (int rc = order_all(s, st)) return rc;
    const uint32_t n = (s->tab.W + s->tab.H) * s->tab.spp;
    hipLaunchKernelGGL(frame_tables_kernel(), dim3((n + kWG - 1) / kWG), dim3(kWG), 0, st, s->d_ndc, s->d_smp, s->tab);
    RT_HIP(hipGetLastError());
    s->tab_dirty = false;
    return RT_OK;
}

int begin_table_launch(rt_scene *s, hipStream_t st)
{
    if (int rc = begin_launch(s, st, Order::all)) return rc;
    fref_launched(s->fref, 0u);                 // (this launch reads no per-origin records)
    return RT_OK;
}

int mark_own(rt_scene *s, hipStream_t st)
{
    RT_HIP(hipEventRecord(s->ev_own->ev, st));
    s->ev_last = s->ev_own;
    s->ev_recorded = true;
    return RT_OK;
}

int mark_free(rt_scene *s, const EvRef *timed_stop, hipEvent_t *stop)
{
    if (timed_stop)
        s->ev_last = *timed_stop;
    else if (int rc = free_done_event(s, s->ev_last))
        return rc;
    s->ev_recorded = true;
    *stop = s->ev_last->ev;
    return RT_OK;
}

int prepare_samples(rt_scene *s, const rt_frame *f, uint32_t spp)
{
    if (tables_match(s, f, spp)) return RT_OK;
    s->fp_valid = false;
    const std::vector<float> tbl = sample_table(f, spp);
    const size_t n = (size_t(f->width) + f->height) * spp;
    if (spp <= kTabMaxSpp && n <= s->ndc_cap)
    {
        // the tables are written on the device, in stream order before the frame's launch
        // (flush_tables): a new frame shape costs no host wait and no synchronous copy
        std::vector<float> key = ndc_key(f, spp, tbl);
        if (key != s->ndc_key || tbl != s->smp_host)
        {
            s->tab.fx = fov_xs_of(f);
            s->tab.aspect = float(f->width) / float(f->height);
            s->tab.W = f->width;
            s->tab.H = f->height;
            s->tab.spp = spp;
            std::memcpy(s->tab.smp, tbl.data(), tbl.size() * sizeof(float));
            s->tab_dirty = true;
            s->tab_epoch++;
            s->ndc_key = key;
            s->ndc_w = f->width;
            s->ndc_spp = spp;
            s->smp_host = tbl;
        }
        return remember_tables(s, f, spp, tbl);
    }
    s->tab_dirty = false;           // a pending device write is superseded (its key differs: spp)
    if (int rc = prepare_ndc(s, f, spp, tbl)) return rc;
    if (tbl == s->smp_host) return remember_tables(s, f, spp, tbl);
    if (int rc = wait_scene_idle(s)) return rc;
    if (spp > s->smp_cap)
    {
        if (s->d_smp) RT_HIP(hipFree(s->d_smp));
        if (s->h_smp_pinned) RT_HIP(hipHostFree(s->h_smp_pinned));
        s->d_smp = nullptr;
        s->h_smp_pinned = nullptr;
        const uint32_t cap = std::max<uint32_t>(64, spp);
        RT_HIP(hipMalloc(&s->d_smp, sizeof(float2) * cap));
        RT_HIP(hipHostMalloc(&s->h_smp_pinned, sizeof(float2) * cap));
        s->smp_cap = cap;
    }
    std::memcpy(s->h_smp_pinned, tbl.data(), tbl.size() * sizeof(float));
    RT_HIP(hipMemcpy(s->d_smp, s->h_smp_pinned, tbl.size() * sizeof(float), hipMemcpyHostToDevice));
    s->smp_host = tbl;
    return remember_tables(s, f, spp, tbl);
}

int validate_frame(const rt_frame *f)
{
    constexpr uint32_t kKernelFlags = RT_KERNEL_FLAG_WIDE_HEAVY | RT_KERNEL_FLAG_EXHAUSTIVE |
                                      RT_KERNEL_FLAG_WAVE_CLOCK | RT_KERNEL_FLAG_OVERLAP | RT_KERNEL_BUDGET_MASK;
    if (!f) return fail(RT_E_INVALID, "frame is NULL");
    if (f->width == 0 || f->height == 0 || f->width > 65536 || f->height > 65536)
        return fail(RT_E_INVALID, "frame width/height must be in [1, 65536]");
    if (f->tri_test > RT_TRI_BARYCENTRIC) return fail(RT_E_INVALID, "unknown tri_test");
    if (f->intersector > RT_ISECT_RAY_MARCH) return fail(RT_E_INVALID, "unknown intersector");
    if (f->intersector == RT_ISECT_BRUTE_FORCE && f->tri_test != RT_TRI_MOLLER_TRUMBORE)
        return fail(RT_E_INVALID, "IntersectBruteForce uses IntersectRayTri only (renderer.cpp:176)");
    const uint32_t kind = f->kernel & RT_KERNEL_KIND_MASK;
    if (kind > RT_KERNEL_COMPACT || (f->kernel & ~(RT_KERNEL_KIND_MASK | kKernelFlags)))
        return fail(RT_E_INVALID, "unknown or removed kernel kind / flag");
    const uint32_t spp = std::max(1u, f->spp);
    if (spp > 4096) return fail(RT_E_INVALID, "spp must be <= 4096");
    if (kind == RT_KERNEL_COMPACT && ((f->kernel & RT_KERNEL_BUDGET_MASK) >> RT_KERNEL_BUDGET_SHIFT) > 64u)
        return fail(RT_E_INVALID, "compaction refill threshold must be <= 64 lanes");
    if ((kind == RT_KERNEL_LANES || kind == RT_KERNEL_COMPACT) && !(is_pow2(spp) && spp <= 64))
        return fail(RT_E_INVALID, "RT_KERNEL_LANES needs spp to be a power of two <= 64");
    return RT_OK;
}

// Fills the per-frame parameters (camera constants exactly as camera.h computes them).
void frame_params(const rt_scene *s, const rt_frame *f, KParams& P)
{
    std::memset(&P, 0, sizeof(P));
    const float (*c)[4] = reinterpret_cast<const float (*)[4]>(f->cam);
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) P.m[3 * r + k] = c[r][k];
    P.fov_xs = fov_xs_of(f);                                    // camera.h:42, double tan (H5)
    P.aspect = float(f->width) / float(f->height);
    P.ndcx = s->d_ndc;                                          // prepare_ndc (this frame's shape)
    P.ndcy = s->d_ndc + size_t(s->ndc_w) * s->ndc_spp;
    for (int k = 0; k < 3; k++)                                 // lin_alg.h:518-535
        P.org[k] = 0.0f * c[0][k] + 0.0f * c[1][k] + 0.0f * c[2][k] + c[3][k];
    P.W = f->width;
    P.H = f->height;
    P.spp = std::max(1u, f->spp);
    P.spp_shift = is_pow2(P.spp) ? log2u(P.spp) : 0;
    P.inv_spp = is_pow2(P.spp) ? 1.0f / float(P.spp) : 0.0f;
    P.smp = s->d_smp;
    scene_params(s, P);
    P.tri_test = f->tri_test;
    P.isect = f->intersector;
}

// The scene's own arrays and grid constants (frame_params' second half; rt_trace_rays_device fills
// nothing else)
void scene_params(const rt_scene *s, KParams& P)
{
    for (int a = 0; a < 3; a++)
    {
        P.bmin[a] = s->bmin[a];
        P.bmax[a] = s->bmax[a];
        P.dim[a] = int(s->dims[a]);
    }
    P.cw = s->cw;
    P.icw = s->icw;
    P.dxdz = int(s->dims[0] * s->dims[2]);
    P.max_steps = s->dims[0] + s->dims[1] + s->dims[2] + 3;
    P.off = s->d_off;
    P.cellw = s->d_cellw;
    P.cellwo = s->d_cellwo ? s->d_cellwo : s->d_cellw;
    P.oct_stride = s->d_cellwo ? s->oct_stride : 0u;
    P.cellwb = s->d_cellwb;
    P.box_stride = s->box_stride;
    P.refs = s->d_refs;
    P.frefs = s->d_frefs[0];                                    // ensure_origin_terms picks the buffer
    P.gates = s->rec_gate ? s->d_gates[0] : nullptr;            // (and its gate array)
    P.shade = s->d_shade;
    P.face_n = s->d_facen;
    P.tri_mt = s->d_trimt;
    P.tri_dist = s->d_tridist;
    P.dist_blk = s->d_distblk;
    P.ndist_blk = s->ndist_blk;
    P.scene_scale = s->scene_scale;
    for (int a = 0; a < 3; a++)
    {
        P.smin[a] = s->vmin[a];
        P.smax[a] = s->vmax[a];
    }
    P.ntris = s->ntris;
}

namespace {
bool use_lanes(const rt_frame *f, uint32_t spp)
{
    if ((f->kernel & RT_KERNEL_KIND_MASK) == RT_KERNEL_PIXEL_LOOP) return false;
    return is_pow2(spp) && spp <= 64;
}

// A frame of this origin may overlap the scene's last launch (RT_KERNEL_FLAG_OVERLAP) as far as the
// per-origin records go (rt_fref_slots.h).
bool fref_overlap_ok(const rt_scene *s, const float org[3])
{
    uint32_t ob[3];
    rtk::fref_bits(org, ob);
    return rtk::fref_overlap_ok(s->fref, ob);
}

// The per-reference origin terms for this frame's camera origin in a buffer of their own
// (rtk::fref_slot_for_launch), computed when neither buffer holds them (a moving camera pays one small
// launch per frame), ordered after every launch that may still read that buffer: the caller has ordered
// st after the launch before the last one and -- unless this launch overlaps it, when its buffers count as
// busy -- after the last one (order_all); busy: buffers that frames of this call read already.
// Sets P.frefs (and P.gates, the buffer's gate array -- null for a frame whose camera is outside the gate's
// proof, frame_gated) and marks the buffer in *used.
int ensure_origin_terms(rt_scene *s, KParams& P, hipStream_t st, uint32_t busy, uint32_t *used)
{
    bool compute = false;
    uint32_t ob[3];
    rtk::fref_bits(P.org, ob);
    const int b = rtk::fref_slot_for_launch(s->fref, ob, busy, &compute);
    if (b < 0) return fail(RT_E_INVALID, "internal: no free per-origin record buffer");
    if (compute)
    {
        if (s->nrefs)
            hipLaunchKernelGGL(origin_pre_kernel(), dim3((s->nrefs + kWG - 1) / kWG), dim3(kWG), 0, st, s->d_refs,
                               s->d_frefs[b], s->rec_gate ? s->d_gates[b] : nullptr, s->nrefs, P.org[0], P.org[1],
                               P.org[2]);
        RT_HIP(hipGetLastError());
        rtk::fref_computed(s->fref, b, ob);
    }
    P.frefs = s->d_frefs[b];
    P.gates = frame_gated(s, P) ? s->d_gates[b] : nullptr;
    *used |= 1u << b;
    return RT_OK;
}

// The miss mask of one frame of a lane-kernel launch (P complete: region, shard, ipt_shift, tiles_x_m),
// n_items work items, on stream st after the frame's tables (flush_tables) and before its render kernel.  The
// callers pass AUTO's lane kernels on the grid walk only -- no wave clocks, no hit IDs, no records, no stream
// capture (a captured k_miss_mask has not run when the next frame asks for its count).  Sets P.miss_mask /
// P.rowmiss, or leaves them null -- the kernel then traces every item, which is always exact --: the skip is
// off, the origin is inside the box, the frame's mask is known to flag nothing, or both buffers are read by
// launches this one is not ordered after.  *used: the scene's buffers the launch reads so far (this frame's
// is added; a buffer in it is not rewritten for a later frame of the same launch).
// A mask pays only where its key repeats, so a key gets one when it is asked for the SECOND time while still among
// the last kMissSeen unmasked keys: a camera that moves every frame never launches k_miss_mask.  And a buffer
// whose mask, of the current tables, was used within the last kMissKeep requests is not evicted: keys that rotate
// through the two buffers (three row bands per frame) settle on two masked keys and the others unmasked instead of
// recomputing one per request (more than 2 + kMissSeen rotating keys are never seen twice; fewer reuse a buffer
// within kMissKeep).
int ensure_miss_mask(rt_scene *s, KParams& P, uint32_t n_items, hipStream_t st, uint32_t *used)
{
    P.miss_mask = P.rowmiss = nullptr;
    s->miss_frame_slot = -1;
    if (!s->miss_skip || !s->h_miss_cnt || n_items == 0u) return RT_OK;
    bool inside = true;
    for (int a = 0; a < 3; a++) inside = inside && P.org[a] >= P.bmin[a] && P.org[a] <= P.bmax[a];
    if (inside) return RT_OK;                                   // rtd::point_in_aabb: nothing misses the box
    rtk::MissKey key;
    std::memset(&key, 0, sizeof(key));
    std::memcpy(key.m, P.m, sizeof(key.m));
    std::memcpy(key.org, P.org, sizeof(key.org));
    key.W = P.W; key.H = P.H; key.spp = P.spp;
    key.rx0 = P.rx0; key.ry0 = P.ry0; key.rw = P.rw; key.rh = P.rh;
    key.rank = P.rank; key.nranks = P.nranks; key.tiles_x = P.tiles_x; key.n_items = n_items;
    key.tab_epoch = s->tab_epoch;
    const uint64_t now = ++s->miss_clock;
    auto hand = [&](int b) {
        s->miss[b].stamp = now;
        P.rowmiss = s->miss[b].d + kMissHead;
        P.miss_mask = s->miss[b].d + miss_mask_offset(P.H);
        s->miss_frame_slot = b;
        *used |= 1u << b;
    };
    for (int b = 0; b < 2; b++)
        if (s->miss[b].valid && std::memcmp(&s->miss[b].key, &key, sizeof(key)) == 0)
        {
            // finished and nothing flagged: the frame stops paying for the mask (the word carries the tag of the
            // k_miss_mask that wrote it: an earlier mask of this buffer that finishes late is not mistaken for it)
            rtk::MissSlot& m = s->miss[b];
            if (*static_cast<volatile uint32_t *>(s->h_miss_cnt + b) == m.tag)
            {
                m.stamp = now;
                return RT_OK;
            }
            if (!m.wr_done && st != m.wr_stream)
            {
                if (hipEventQuery(m.wr_ev) == hipSuccess) m.wr_done = true;
                else RT_HIP(hipStreamWaitEvent(st, m.wr_ev, 0));
            }
            hand(b);
            return RT_OK;
        }
    int b = -1;
    for (int c = 0; c < 2; c++)
    {
        const rtk::MissSlot& m = s->miss[c];
        const bool writable = !((s->miss_busy >> c) & 1u) || (m.rd_any && !m.rd_multi && m.rd_stream == st);
        if (((*used >> c) & 1u) || !writable) continue;
        // in use: not evicted -- unless it is of an earlier version of the tables (a change of fov, shape or sample
        // table): tab_epoch only grows, so that key is never asked for again, and keeping its buffer would leave
        // the frames after the change without a mask for up to kMissKeep requests
        if (m.valid && m.key.tab_epoch == s->tab_epoch && now - m.stamp <= rtk::kMissKeep) continue;
        if (b < 0 || !m.valid || (s->miss[b].valid && m.stamp < s->miss[b].stamp)) b = c;
    }
    int seen = -1;
    for (uint32_t i = 0; i < s->miss_seen_n; i++)
        if (std::memcmp(&s->miss_seen[i], &key, sizeof(key)) == 0) seen = int(i);
    if (seen < 0)
    {
        // the key's first request: remembered, traced without a mask
        s->miss_seen[s->miss_seen_next] = key;
        s->miss_seen_next = (s->miss_seen_next + 1u) % rtk::kMissSeen;
        s->miss_seen_n = std::min(s->miss_seen_n + 1u, rtk::kMissSeen);
        return RT_OK;
    }
    if (b < 0) return RT_OK;
    s->miss_seen[seen].n_items = 0u;                            // (no frame has n_items == 0: the entry matches nothing now)
    rtk::MissSlot& m = s->miss[b];
    const size_t need = miss_buffer_words(P.H, n_items);
    if (need > m.cap)
    {
        // (every reader of the old buffer is ordered before st's next work, see above: st drained, it is free)
        m.valid = false;
        if (m.d)
        {
            RT_HIP(hipStreamSynchronize(st));
            RT_HIP(hipFree(m.d));
        }
        m.d = nullptr;
        m.cap = 0;
        RT_HIP(hipMalloc(&m.d, need * sizeof(uint32_t)));
        m.cap = need;
        RT_HIP(hipMemsetAsync(m.d, 0, kMissHead * sizeof(uint32_t), st));     // the kernel re-arms them itself
    }
    m.tag = 0x80000000u | ((((m.tag >> 24) + 1u) & 0x7Fu) << 24);      // 0x80 | generation, count 0
    *static_cast<volatile uint32_t *>(s->h_miss_cnt + b) = 0u;
    const uint32_t threads = std::max((n_items + 63u) & ~63u, P.H);
    // (the dispatch carries its completion event itself: no marker packet between it and the frame)
    if (!m.wr_ev) RT_HIP(hipEventCreateWithFlags(&m.wr_ev, s->ev_order_flags));
    hipExtLaunchKernelGGL(miss_mask_kernel(), dim3((threads + kWG - 1u) / kWG), dim3(kWG), 0, st, nullptr, m.wr_ev, 0u, P,
                          n_items, m.d, s->d_miss_cnt + b, m.tag);
    RT_HIP(hipGetLastError());
    m.wr_stream = st;
    m.wr_done = false;
    m.key = key;
    m.valid = true;
    m.rd_any = m.rd_multi = false;
    s->miss_computed++;
    hand(b);
    return RT_OK;
}

// The scene's launch on st reads the mask buffers `used` (0: none).  more: the launch runs beside the scene's
// last one without the two being ordered here (rt_render_frame_host_tiled's row bands), so it adds to that one's.
void miss_launched(rt_scene *s, uint32_t used, hipStream_t st, bool more)
{
    for (int b = 0; b < 2; b++)
        if ((used >> b) & 1u)
        {
            rtk::MissSlot& m = s->miss[b];
            m.rd_multi = m.rd_multi || (m.rd_any && m.rd_stream != st);
            m.rd_stream = st;
            m.rd_any = true;
        }
    s->miss_busy |= used;
    s->miss_last = more ? (s->miss_last | used) : used;
}

// AUTO's own choice of the wide section for a single-frame launch: a shard of >= 2 ranks of a scene
// with dense cells
bool auto_wide(const rt_scene *s, const KParams& P)
{
    return P.nranks >= 2u && s->max_cell_refs >= s->wh_auto_refs;
}

// The per-rank-count tunables' bit index (wh_lds, wg64_wide, wg64_o8: bit log2 N, 3 for N >= 8)
uint32_t lg_ranks(uint32_t nranks)
{
    return nranks >= 8u ? 3u : (nranks >= 4u ? 2u : (nranks >= 2u ? 1u : 0u));
}

// kernel-time events only outside stream capture (a captured record has no time to read)
// A timed event pair costs ~10 us of device time per launch (measured: bench step 0.755 ->
// 0.736 ms without), so only every time_every-th launch is timed (rt_scene_set_timing)
struct Timed { uint32_t kslot; hipEvent_t kt0; const EvRef *kt1; };     // kt0 / kt1 null: not timed

// Counts the launch and, for a timed one, readies its pair in the ring's next slot (end_timed advances the ring)
int begin_timed(rt_scene *s, hipStreamCaptureStatus cap, Timed& t)
{
    const bool timed = cap == hipStreamCaptureStatusNone && s->time_every && s->launches % s->time_every == 0u;
    s->launches++;
    t = Timed{ s->kt_next, nullptr, nullptr };
    if (!timed) return RT_OK;
    if (!s->kt0[t.kslot]) RT_HIP(hipEventCreateWithFlags(&s->kt0[t.kslot], s->ev_time_flags));
    // a ring slot's stop event still marking another scene's last launch is left to it
    if (!s->kt1[t.kslot] || s->kt1[t.kslot].use_count() > 1)
        if (int rc = new_event(s->kt1[t.kslot], s->ev_time_flags)) return rc;
    t.kt0 = s->kt0[t.kslot];
    t.kt1 = &s->kt1[t.kslot];
    return RT_OK;
}

// After the launch went out without an error
void end_timed(rt_scene *s, const Timed& t)
{
    if (!t.kt1) return;
    s->kt_last = t.kslot;
    s->kt_next = (t.kslot + 1u) % kTimeRing;
    s->kt_count = std::min(s->kt_count + 1u, kTimeRing);
}

// The scene's wave-clock buffer (RT_KERNEL_FLAG_WAVE_CLOCK) for a launch that writes `records` of them, four
// words each; clear: zeroed on st first (a batch's wide-section records are not all written)
int ensure_wave_clocks(rt_scene *s, size_t records, hipStream_t st, bool clear)
{
    const size_t need = records * 4u;
    if (int rc = grow(s->d_clk, s->clk_cap, need)) return rc;
    if (clear) RT_HIP(hipMemsetAsync(s->d_clk, 0, need * sizeof(uint64_t), st));
    s->clk_items = uint32_t(records);
    return RT_OK;
}

// Launches the render kernel over region/shard described by P (tiles_x, rank, ...): the variant, whether it may
// overlap the scene's last launch, its order, the per-origin state (records, miss mask), the launch, its end mark.
int launch_render(rt_scene *s, const rt_frame *f, KParams& P, uint32_t n_local_tiles, hipStream_t st,
                  bool order_streams = true)
{
    if (n_local_tiles == 0) return RT_OK;
    const bool lanes = use_lanes(f, P.spp);
    const uint32_t wgpt = lanes ? (kTilePix * P.spp) / kWG : 1u;       // (lanes: spp a power of two)
    const uint64_t blocks = uint64_t(n_local_tiles) * wgpt;
    if (blocks > 0x3FFFFFFFull) return fail(RT_E_INVALID, "frame too large for one launch");
    launch_shape(P, wgpt, uint32_t(blocks));
    if (!lanes) P.ipt_shift = 0u;                                      // (the pixel loop has no items per tile)
    const uint32_t kind = f->kernel & RT_KERNEL_KIND_MASK;
    const bool bary = P.tri_test == RT_TRI_BARYCENTRIC;
    const bool grid_mt = P.isect == RT_ISECT_GRID && !bary;
    // The per-camera records (frefs) are scene state: a launch on another stream than the last
    // one waits for it -- unless the caller allows overlap (RT_KERNEL_FLAG_OVERLAP) and nothing the
    // two launches share changes between them (as launch_batch): AUTO's lane kernel (not the wide
    // section's side-stream pair, not the wave clocks), the same tables and camera origin, and an
    // existing launch shape whose frame is not measured.
    // (order_streams false: the caller orders its streams itself, rt_render_frame_host_tiled)
    // No overlap inside a stream capture: plans there run on the launch stream (launch_plans).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    RT_HIP(hipStreamIsCapturing(st, &cap));
    bool overlap = false;
    if (order_streams && cap == hipStreamCaptureStatusNone && (f->kernel & RT_KERNEL_FLAG_OVERLAP) && s->ev_recorded &&
        st != s->last_stream &&
        kind == RT_KERNEL_AUTO && lanes && grid_mt && !(f->kernel & (RT_KERNEL_FLAG_WAVE_CLOCK | RT_KERNEL_FLAG_WIDE_HEAVY)) &&
        !auto_wide(s, P) && P.spp <= 64u && !s->tab_dirty)
    {
        overlap = fref_overlap_ok(s, P.org);
        const int v = kVarAutoCore | frame_traversal_bits(s, P);
        if (overlap && blocks >= s->hf_min_blocks)
        {
            const HfPeek pk = hf_peek(s, P, blocks, v, 0u, cam_signature(P));
            overlap = pk.found && (!pk.measure || pk.measure_ok);
        }
    }
    if (int rc = begin_launch(s, st, overlap ? Order::overlap : (order_streams ? Order::all : Order::callers))) return rc;
    g_ht.mark("tables");
    // AUTO (and the COMPACT arm built on its per-ray code): the feature set of kVarAuto that this
    // scene allows -- the Newton reciprocal needs rcp_safe, the packed counts and the empty-run
    // loop need pack_ok.  DESIGN.md §4.1 has the measured progression.
    const bool auto_path = lanes && grid_mt && (kind == RT_KERNEL_AUTO || kind == RT_KERNEL_COMPACT);
    int var = 0;
    if (auto_path)
    {
        var = kVarAutoCore | frame_traversal_bits(s, P) | ((f->kernel & RT_KERNEL_FLAG_WAVE_CLOCK) ? kVarWaveClock : 0);
        uint32_t used = 0;
        if (int rc = ensure_origin_terms(s, P, st, 0u, &used)) return rc;
        rtk::fref_launched(s->fref, used);
        g_ht.mark("origin");
    }
    else
    {
        rtk::fref_launched(s->fref, 0u);        // (this launch reads no per-origin records)
        if (P.isect == RT_ISECT_RAY_MARCH)     // (the lane kernels' and the pixel loop's)
            var = kVarMarch | ((f->kernel & RT_KERNEL_FLAG_EXHAUSTIVE) ? kVarExhaustive : 0);
        else if (P.isect == RT_ISECT_BRUTE_FORCE)
            var = kVarBrute;
    }
    // the miss skip: AUTO's lane kernels on the grid walk (RT_KERNEL_LANES stays the unskipped arm), frames
    // that ask for neither hit IDs nor records, outside a stream capture
    uint32_t mused = 0;
    s->miss_frame_slot = -1;
    if (auto_path && kind == RT_KERNEL_AUTO && !(var & kVarWaveClock) && !P.hits && !P.recs &&
        cap == hipStreamCaptureStatusNone)
        if (int rc = ensure_miss_mask(s, P, uint32_t(blocks) * kWavesPerWG, st, &mused)) return rc;
    miss_launched(s, mused, st, !order_streams);
    Timed t;
    if (int rc = begin_timed(s, cap, t)) return rc;
    const hipEvent_t kt0 = t.kt0, kt1 = t.kt1 ? (*t.kt1)->ev : nullptr;
    bool stop_done = false;             // the launch carried its own stop event (ev_last set)
    auto mark = [&](hipEvent_t e) { return e ? hipEventRecord(e, st) : hipSuccess; };
    if (var & kVarWaveClock)
    {
        if (int rc = ensure_wave_clocks(s, size_t(blocks) * kWavesPerWG, st, false)) return rc;
        P.wave_clk = s->d_clk;
    }
    const dim3 wg(kWG);
    const uint32_t budget = (f->kernel & RT_KERNEL_BUDGET_MASK) >> RT_KERNEL_BUDGET_SHIFT;
    // AUTO takes the wide section (kVarWideHeavy: AUTO's full record/count layout, spp <= 16) for
    // a shard of >= 2 ranks of a scene with dense cells: there a rank's launch is bound by its few
    // ~1000-test waves, which the section splits 16 ways (4 for spp 8-16) beside the lane kernel
    // (measured, tools/wh_probe.py, killeroo rank of 2 / 4 / 8: 0.36 / 0.33 / 0.25 ms with the
    // two-phase arm it replaced -> 0.35 / 0.20 / 0.15).  On a whole frame the
    // lanes are busy with other items anyway and the section's repeated walks cost more than they
    // save (+1-3 %).
    const bool wide_ok = auto_path && var == kVarAuto && P.spp <= 16u;
    const bool wide_heavy = wide_ok && kind == RT_KERNEL_AUTO &&
                            ((f->kernel & RT_KERNEL_FLAG_WIDE_HEAVY) || auto_wide(s, P));
    if (lanes && kind == RT_KERNEL_COMPACT && P.isect == RT_ISECT_GRID)
    {
        const uint32_t n_items = uint32_t(blocks * kWavesPerWG);
        const uint32_t refill = budget ? budget : kCompactRefill;
        const dim3 grid(std::max(1u, std::min(s->compact_wgs, (n_items + 3u) / 4u)));
        RT_HIP(mark(kt0));
        // bary: the plain distance-skip walk; AUTO's box-run walk where the scene allows it
        const kcfn_t cfn = bary ? compact_kernel(RT_TRI_BARYCENTRIC, kVarDistSkip)
                           : (auto_runs(s) && (var & kVarFastRcp))        // (rcp_safe, and this frame's camera)
                               ? compact_kernel(RT_TRI_MOLLER_TRUMBORE, kVarCompactBox)
                               : compact_kernel(RT_TRI_MOLLER_TRUMBORE, kVarWaveGate | kVarDistSkip | kVarOriginPre);
        hipLaunchKernelGGL(cfn, grid, wg, 0, st, P, n_items, refill);
        RT_HIP(mark(kt1));
    }
    else if (lanes)
    {
        // AUTO, LANES, and COMPACT where its layout does not apply
        const int kvar = ((kind == RT_KERNEL_AUTO || P.isect != RT_ISECT_GRID) ? var : 0) |
                         (wide_heavy ? kVarWideHeavy : 0);
        const kfn_t fn = lanes_kernel(bary ? RT_TRI_BARYCENTRIC : RT_TRI_MOLLER_TRUMBORE, kvar);
        if (!fn) return fail(RT_E_INVALID, "kernel variant not built: " + std::to_string(kvar));
        uint32_t grid = uint32_t(blocks);
        // heavy-first order: AUTO grid frames large enough that blocks start in several rounds
        // (and every wide-section launch of >= 64 blocks: its lane kernel's heaviest items)
        const bool front = kind == RT_KERNEL_AUTO && P.isect == RT_ISECT_GRID && !(kvar & kVarWaveClock) &&
                           (blocks >= s->hf_min_blocks || (wide_heavy && blocks >= 64u));
        // the wide section's LDS tier (kVarLdsSplit) per rank count (wh_lds, bit log2 N), without
        // RT_KERNEL_FLAG_OVERLAP (as launch_batch)
        const bool lds = wide_heavy && ((s->wh_lds >> lg_ranks(P.nranks)) & 1u) != 0u && !(f->kernel & RT_KERNEL_FLAG_OVERLAP);
        if (front || wide_heavy)
        {
            if (int rc = hf_prepare(s, P, blocks, kvar | (lds ? kVarLdsSplit : 0), front, st)) return rc;
            g_ht.mark("hf_prepare");
            grid += P.hf_front;
        }
        // one-wave workgroups (k_render_lanes_w64): the same blocks, each wave dispatched by itself
        kfn_t lfn = fn;
        uint32_t lgrid = grid, lwg = kWG;
        // (not for a scene with very dense cells: scene 5, a cell of 1,226 references, runs its whole
        // frame 3 % faster in 256-lane workgroups, while killeroo (426) and scene 4 (132) run 4-6 %
        // slower that way: profiles/r05av_wg64_dense.json -- unless the launch may overlap the one before
        // it, whose work fills the tail: config 5 as overlapped frames 2.575 vs 2.607 ms per step,
        // profiles/r06_pipelined_plan_ab.json)
        const bool pipelined = (f->kernel & RT_KERNEL_FLAG_OVERLAP) != 0u;
        if (s->wg64 && kvar == kVarAuto && grid >= s->wg64_min_blocks &&
            (s->max_cell_refs < s->wg64_max_refs || pipelined))
        {
            lfn = lanes_w64_kernel(kVarAuto);
            P.vblocks = grid;
            lgrid = kWavesPerWG * ((grid + kXcds - 1u) / kXcds * kXcds);
            lwg = 64u;
            s->w64_launches++;
        }
        s->lane_launches++;
        if (P.wh_wgs)
        {
            RT_HIP(mark(kt0));
            // the wide section runs on the side stream beside the lane kernel (fork / join by
            // events, so the pair also captures into a hipGraph); submitted first so its waves
            // -- the frame's longest -- start first
            if (!s->side)
            {
                RT_HIP(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
                RT_HIP(hipEventCreateWithFlags(&s->ev_fork, s->ev_order_flags));
                RT_HIP(hipEventCreateWithFlags(&s->ev_join, s->ev_order_flags));
            }
            RT_HIP(hipEventRecord(s->ev_fork, st));
            RT_HIP(hipStreamWaitEvent(s->side, s->ev_fork, 0));
            hipLaunchKernelGGL(wide_kernel(P.wh_g, lds), dim3(P.wh_wgs), wg, 0, s->side, P);
            hipLaunchKernelGGL(lfn, dim3(lgrid), dim3(lwg), 0, st, P);
            RT_HIP(hipEventRecord(s->ev_join, s->side));
            RT_HIP(hipStreamWaitEvent(st, s->ev_join, 0));
            RT_HIP(mark(kt1));
            if (int rc = mark_own(s, st)) return rc;        // (launch_plans forks after ev_last)
            stop_done = true;
        }
        else
        {
            // the dispatch carries its own events (no marker packets): the timed launch's pair, or
            // the scene's completion event alone
            hipEvent_t stop = nullptr;
            if (int rc = mark_free(s, t.kt1, &stop)) return rc;
            hipExtLaunchKernelGGL(lfn, dim3(lgrid), dim3(lwg), 0, st, kt0, stop, 0u, P);
            stop_done = true;
        }
        if ((P.hf_front || P.wh_on) && P.hf_measure)
            if (int rc = launch_plans(s, P, blocks, st, pipelined)) return rc;
    }
    else
    {
        RT_HIP(mark(kt0));
        hipLaunchKernelGGL(pixel_loop_kernel(bary ? RT_TRI_BARYCENTRIC : RT_TRI_MOLLER_TRUMBORE, var),
                           dim3(uint32_t(blocks)), wg, 0, st, P);
        RT_HIP(mark(kt1));
    }
    RT_HIP(hipGetLastError());
    g_ht.mark("launched");
    if (!stop_done)
        if (int rc = mark_own(s, st)) return rc;
    end_timed(s, t);
    return RT_OK;
}


// n frames (2 <= n <= kMaxBatch, scenes on one device, mutexes held by the caller) in ONE launch
// of k_render_batch.  P[i] holds frame i's parameters (frame_params + region + shard + outputs).
// Returns RT_E_INVALID with *batched == false, doing nothing, when the frames cannot share a
// launch (the caller then renders them one launch each).
int launch_batch(rt_scene *const *S, const rt_frame *F, uint32_t n, KParams *P, uint32_t n_local_tiles,
                 hipStream_t st, bool *batched)
{
    *batched = false;
    if (n < 2 || n > kMaxBatch || n_local_tiles == 0) return RT_E_INVALID;
    const uint32_t spp = P[0].spp;
    if (!use_lanes(&F[0], spp) || spp > 16u) return RT_E_INVALID;
    int var = -1;
    bool wide_heavy = false;
    for (uint32_t i = 0; i < n; i++)
    {
        const uint32_t kind = F[i].kernel & RT_KERNEL_KIND_MASK;
        if (kind != RT_KERNEL_AUTO ||
            (F[i].kernel & ~uint32_t(RT_KERNEL_FLAG_WIDE_HEAVY | RT_KERNEL_FLAG_WAVE_CLOCK | RT_KERNEL_FLAG_OVERLAP)) != 0u ||
            (F[i].kernel & RT_KERNEL_FLAG_WAVE_CLOCK) != (F[0].kernel & RT_KERNEL_FLAG_WAVE_CLOCK))
            return RT_E_INVALID;
        if (P[i].isect != RT_ISECT_GRID || P[i].tri_test != RT_TRI_MOLLER_TRUMBORE) return RT_E_INVALID;
        if (P[i].W != P[0].W || P[i].H != P[0].H || P[i].spp != spp || S[i]->device != S[0]->device)
            return RT_E_INVALID;
        // (the frame's camera counts: rt_cam_bound.h; a frame whose gate or reciprocal choice differs from
        // frame 0's cannot share the launch, and one without kVarFastRcp has no batch kernel)
        const int v = kVarAutoCore | frame_traversal_bits(S[i], P[i]);
        if (var >= 0 && v != var) return RT_E_INVALID;
        if (cam_gate_ok(cam_dir_bound(P[i].m)) != cam_gate_ok(cam_dir_bound(P[0].m))) return RT_E_INVALID;
        var = v;
        wide_heavy = wide_heavy || (F[i].kernel & RT_KERNEL_FLAG_WIDE_HEAVY) ||
                     (P[i].nranks >= 2u && S[i]->max_cell_refs >= S[0]->wh_auto_refs);
    }
    if (var != kVarAuto) return RT_E_INVALID;
    // the wide section always leads the batch kernel's own grid (measured against its own kernel on a
    // side stream, profiles/r03f_ab_wide_fused.json: 18 % faster at a rank of 8, 9 % at 4; a rank of
    // 2 0.321 ms fused vs 0.338, profiles/r03aa_wg64_wide_fused2_sweep.json; the side-stream arm was
    // removed in round 5)
    const bool fused = wide_heavy;
    const bool clk = (F[0].kernel & RT_KERNEL_FLAG_WAVE_CLOCK) != 0u;
    const uint32_t lgr = lg_ranks(P[0].nranks);
    // the section's LDS tier (kVarLdsSplit) per rank count (wh_lds, bit log2 N), for
    // launches that do not ask to overlap the previous one (RT_KERNEL_FLAG_OVERLAP): there the launch's
    // tail is exposed and the tier shortens it (a rank of 8's step 0.106 -> 0.096 ms), while an
    // overlapped launch's tail is filled by the next one and the tier's 256-lane grid costs more
    // (0.0875 -> 0.090 ms, profiles/r06_lds_tier_ab.json)
    const bool lds = fused && ((S[0]->wh_lds >> lgr) & 1u) != 0u && !(F[0].kernel & RT_KERNEL_FLAG_OVERLAP);
    const int kvar = var | (wide_heavy ? kVarWideHeavy : 0) | (fused ? kVarWideFused : 0) |
                     (fused && spp > 4u ? kVarWideG4 : 0) | (lds ? kVarLdsSplit : 0) |
                     (clk ? kVarWaveClock : 0);
    if (!batch_kernel(kvar, false)) return RT_E_INVALID;
    const uint32_t wgpt = (kTilePix * spp) / kWG;
    const uint64_t fblocks = uint64_t(n_local_tiles) * wgpt;
    const uint64_t blocks = fblocks * n;
    if (blocks > 0x3FFFFFFFull) return RT_E_INVALID;        // one launch per frame (each checks its own size)
    // A scene has two per-origin record buffers, all of them this launch's to read: frames of one scene at
    // more than two DISTINCT camera origins cannot share a launch.  norg[i]: the distinct origins of frame
    // i's scene among frames 0 .. i.
    uint32_t norg[kMaxBatch] = {};
    for (uint32_t i = 0; i < n; i++)
    {
        uint32_t seen[2][3], ob[3], nseen = 0;
        for (uint32_t j = 0; j <= i; j++)
        {
            if (S[j] != S[i]) continue;
            rtk::fref_bits(P[j].org, ob);
            bool fresh = true;
            for (uint32_t k = 0; k < nseen; k++) fresh = fresh && std::memcmp(ob, seen[k], sizeof(ob)) != 0;
            if (!fresh) continue;
            if (nseen == 2u) return RT_E_INVALID;           // a third origin: one launch per frame
            std::memcpy(seen[nseen++], ob, sizeof(ob));
        }
        norg[i] = nseen;
    }
    *batched = true;
    KBatch KB;
    std::memset(&KB, 0, sizeof(KB));
    KB.nframes = n;
    for (uint32_t i = 0; i <= n; i++) KB.base[i] = uint32_t(fblocks * i);
    for (uint32_t i = n + 1; i <= kMaxBatch; i++) KB.base[i] = uint32_t(blocks);
    // the batch's heavy-first / wide-section state lives in scene 0's table, keyed by the batch
    uint64_t ident = n;
    for (uint32_t i = 0; i < n; i++) ident = ident * 0x9E3779B97F4A7C15ull + uint64_t(uintptr_t(S[i]));
    rt_scene *s0 = S[0];
    const bool front = blocks >= s0->hf_min_blocks || (wide_heavy && blocks >= 64u);
    uint64_t cams = 0xcbf29ce484222325ull;
    for (uint32_t i = 0; i < n; i++) cams = cam_signature(P[i], cams);
    // (the batch kernel maps the launch's blocks -- every frame's -- by P[0]'s three band fields)
    for (uint32_t i = 0; i < n; i++) launch_shape(P[i], wgpt, uint32_t(blocks));
    // RT_KERNEL_FLAG_OVERLAP (every frame of the batch): this launch may run beside the scenes' last
    // launch on another stream -- its tail under this launch's start -- when no scene state changes
    // between them: the frame tables and the per-origin records stay, the batch's heavy-first
    // context exists and this frame is not measured (a measured frame clears and rewrites plan
    // buffers that an older version's frames read), no wave clocks or segmented-tier scratch
    // (per-scene buffers), no stream capture (its plans run on the launch stream).  At most two
    // launches of a scene are in flight: an overlapped launch waits for the one before the launch it
    // overlaps (ev_prev).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    RT_HIP(hipStreamIsCapturing(st, &cap));
    bool overlap = !clk && cap == hipStreamCaptureStatusNone;
    for (uint32_t i = 0; i < n; i++)
    {
        overlap = overlap && (F[i].kernel & RT_KERNEL_FLAG_OVERLAP) && !S[i]->tab_dirty && fref_overlap_ok(S[i], P[i].org);
        // a scene in the batch at two origins: both record buffers are this launch's, so it orders after
        // every launch of the scene
        if (norg[i] > 1u) overlap = false;
    }
    if (overlap && (front || wide_heavy))
    {
        const HfPeek pk = hf_peek(s0, P[0], blocks, kvar, ident | 1u, cams);
        overlap = pk.found && (!pk.measure || pk.measure_ok);
    }
    // per-origin records of every frame, and the cross-stream order of every scene's state
    uint32_t used[kMaxBatch] = {};             // per frame: its scene's record buffers this launch reads
    uint32_t mused[kMaxBatch] = {};            // ... and its scene's miss-mask buffers
    for (uint32_t i = 0; i < n; i++)
    {
        rt_scene *s = S[i];
        int first = -1;
        for (uint32_t j = 0; j < i && first < 0; j++)
            if (S[j] == s) first = int(j);
        if (first < 0)
        {
            const bool beside = overlap && s->ev_recorded && st != s->last_stream;
            if (int rc = begin_launch(s, st, beside ? Order::overlap : Order::all)) return rc;
            if (int rc = ensure_origin_terms(s, P[i], st, 0u, &used[i])) return rc;
        }
        else
        {
            uint32_t u = used[first];
            if (int rc = ensure_origin_terms(s, P[i], st, u, &u)) return rc;
            used[first] = u;
        }
        // the frame's miss mask (as launch_render; mused: per scene, at its first frame's index)
        if (!clk && cap == hipStreamCaptureStatusNone && !P[i].hits && !P[i].recs)
            if (int rc = ensure_miss_mask(s, P[i], uint32_t(fblocks) * kWavesPerWG, st, &mused[first < 0 ? i : uint32_t(first)]))
                return rc;
    }
    for (uint32_t i = 0; i < n; i++)
    {
        bool first = true;
        for (uint32_t j = 0; j < i; j++) first = first && S[j] != S[i];
        if (first) rtk::fref_launched(S[i]->fref, used[i]);
        if (first) miss_launched(S[i], mused[i], st, false);
    }
    if (front || wide_heavy)
        if (int rc = hf_prepare(s0, P[0], blocks, kvar, front, st, ident | 1u, cams)) return rc;
    // fused: the wide section's workgroups lead the grid, a multiple of the XCD count so the lane
    // blocks keep their block -> XCD assignment
    // (the rounding's extra workgroups join the LDS tier, or without one the G-lane tier)
    if (fused && P[0].wh_wgs)
    {
        P[0].wh_wgs = (P[0].wh_wgs + kXcds - 1u) & ~(kXcds - 1u);
        if (!P[0].wh_lds) P[0].wh_wgs_g = P[0].wh_wgs;
    }
    uint32_t grid = uint32_t(blocks) + P[0].hf_front + (fused ? P[0].wh_wgs : 0u);
    // one-wave workgroups (k_render_batch_w64, as k_render_lanes_w64): the same blocks and order.
    // Without a wide section (N = 1) the bench pair took 0.569 vs 0.598 ms with 256-lane
    // workgroups (profiles/r03y_wg64_batch_sweep.json).  Beside one, per rank count (wg64_wide, bit
    // log2 N, 3 for N >= 8): with the section fused from 2 ranks and one-wave workgroups on both
    // (profiles/r03aa_wg64_wide_*.json) a rank of 2 took 0.306 ms (0.321 with 256-lane ones, 0.338
    // unfused), of 8 0.117 (0.121); a rank of 4 0.206 vs 0.193, so 4 keeps 256-lane workgroups
    const bool w64 = s0->wg64 != 0u && !lds && (!wide_heavy || ((s0->wg64_wide >> lgr) & 1u) != 0u) &&
                     uint32_t(blocks) + P[0].hf_front >= s0->wg64_batch_min_blocks;
    uint32_t bwg = kWG;
    if (w64)
    {
        P[0].vblocks = uint32_t(blocks) + P[0].hf_front;
        grid = kWavesPerWG * ((fused ? P[0].wh_wgs : 0u) + (P[0].vblocks + kXcds - 1u) / kXcds * kXcds);
        bwg = 64u;
        s0->w64_launches++;
    }
    s0->lane_launches++;
    // the fused one-wave kernel held to 8 waves / SIMD (76 SGPRs; the plain build's 83 admit 7), per
    // rank count (wg64_o8, bit log2 N): a rank of 2 0.2925 vs 0.3025 ms, of 8 0.1171-0.1182 vs
    // 0.1139-0.1151 (profiles/r05f_ab_o8.json), so 2 only
    const bool o8 = ((s0->wg64_o8 >> lgr) & 1u) != 0u && (kvar & kVarWideFused) != 0;
    const kbfn_t fn = batch_kernel(kvar, w64, o8);
    if (clk)
    {
        // one record per lane item and per (listed item, wave) of the wide section
        if (int rc = ensure_wave_clocks(s0, size_t(blocks) * kWavesPerWG + size_t(kWhMax) * 17u, st, true)) return rc;
        P[0].wave_clk = s0->d_clk;
    }
    for (uint32_t i = 0; i < n; i++) KB.p[i] = P[i];
    // timing: scene 0's ring (one timed launch for the whole batch)
    Timed t;
    if (int rc = begin_timed(s0, cap, t)) return rc;
    // the dispatch's stop event marks every batched scene's last launch (no marker per scene: ten of
    // them cost config 5's step 50 us, profiles/r05u_marker_ab.json)
    hipEvent_t stop = nullptr;
    if (int rc = mark_free(s0, t.kt1, &stop)) return rc;
    // a timed launch carries its start / stop events in the dispatch itself: separate event records
    // around it cost a measured 3-4 % of that frame (profiles/r05j_frame_series_*.json, steps 8, 24, ...)
    hipExtLaunchKernelGGL(fn, dim3(grid), dim3(bwg), 0, st, t.kt0, stop, 0u, KB);
    for (uint32_t i = 1; i < n; i++)
    {
        S[i]->ev_last = s0->ev_last;
        S[i]->ev_recorded = true;
    }
    if ((P[0].hf_front || P[0].wh_on) && P[0].hf_measure)
        if (int rc = launch_plans(s0, KB.p[0], blocks, st, false)) return rc;
    RT_HIP(hipGetLastError());
    end_timed(s0, t);
    return RT_OK;
}

// Device staging frame (and, for rt_render_tiles, the scene's pinned host frame) of >= words.
int ensure_frame(rt_scene *s, size_t words, bool host)
{
    if (int rc = grow(s->d_frame, s->frame_cap, words)) return rc;
    if (host && words > s->hframe_cap)
    {
        if (s->h_frame) RT_HIP(hipHostFree(s->h_frame));
        s->h_frame = nullptr;
        RT_HIP(hipHostMalloc(&s->h_frame, words * 4));
        s->hframe_cap = words;
    }
    return RT_OK;
}

// Frame parameters of a device-resident render (see render_device); returns the local tile count.
uint32_t device_params(const rt_scene *s, const rt_frame *f, uint32_t rank, uint32_t nranks, bool shard,
                       uint32_t *d_out, uint32_t *d_hits, KParams& P)
{
    frame_params(s, f, P);
    const uint32_t ntiles = region_params(P, 0, 0, f->width, f->height, d_out, shard ? 0u : f->width, shard ? 1u : 0u);
    P.rank = rank; P.nranks = nranks;
    P.hits = d_hits;
    return ntiles > rank ? (ntiles - rank + nranks - 1) / nranks : 0;
}

// The device-resident render of a whole frame (shard false: d_out[y*W + x]) or of one rank's
// interleaved 16x16 tiles (shard true: d_out = the compact shard, also for nranks == 1),
// optionally with per-sample hit IDs.
int render_device(rt_scene *s, const rt_frame *f, uint32_t rank, uint32_t nranks, bool shard, uint32_t *d_out,
                  uint32_t *d_hits, void *hip_stream, const RecOut *recs = nullptr)
{
    if (!s || !d_out || nranks == 0 || rank >= nranks) return fail(RT_E_INVALID, "bad arguments");
    int rc = validate_frame(f);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(s->mtx);
    g_ht.start();
    if ((rc = ensure_device(s))) return rc;
    const uint32_t spp = std::max(1u, f->spp);
    if ((rc = prepare_samples(s, f, spp))) return rc;
    g_ht.mark("samples");
    KParams P;
    const uint32_t local = device_params(s, f, rank, nranks, shard, d_out, d_hits, P);
    if (recs) set_records(P, *recs);
    rc = launch_render(s, f, P, local, static_cast<hipStream_t>(hip_stream));
    g_ht.mark("done");
    g_ht.end();
    return rc;
}

// rt_render_batch_device's frames [0, n): one k_render_batch launch when they can share it.  The
// cheap checks (one device) come before anything touches a scene's device state; a scene listed
// twice with another frame shape or sample table than its last frame's would read the last one's
// tables, so such batches take one launch per frame (counted in rt_scene_info.batch_fallbacks).
int render_batch_chunk(rt_scene *const *S, const rt_frame *F, uint32_t n, uint32_t rank, uint32_t nranks,
                       uint32_t *const *outs, uint32_t *const *hits, const RecOut *recs, void *hip_stream)
{
    bool batched = false;
    bool one_device = true;
    for (uint32_t i = 1; i < n; i++) one_device = one_device && S[i]->device == S[0]->device;
    if (n >= 2 && one_device)
    {
        std::vector<rt_scene *> uniq(S, S + n);
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        std::vector<std::unique_lock<std::mutex>> locks;
        for (rt_scene *s : uniq) locks.emplace_back(s->mtx);
        int rc = ensure_device(S[0]);
        if (rc) return rc;
        KParams P[kMaxBatch];
        uint32_t local = 0;
        for (uint32_t i = 0; i < n; i++)
        {
            if ((rc = prepare_samples(S[i], &F[i], std::max(1u, F[i].spp)))) return rc;
            local = device_params(S[i], &F[i], rank, nranks, nranks > 1, outs[i], hits ? hits[i] : nullptr, P[i]);
            if (recs) set_records(P[i], recs[i]);
        }
        bool tables_ok = true;
        for (uint32_t i = 0; i < n; i++) tables_ok = tables_ok && tables_match(S[i], &F[i], std::max(1u, F[i].spp));
        if (tables_ok) rc = launch_batch(S, F, n, P, local, static_cast<hipStream_t>(hip_stream), &batched);
        if (batched)
        {
            if (rc == RT_OK) S[0]->batch_launches++;      // bench.py trusts this count (VALU roofline)
            return rc;
        }
    }
    if (n >= 2)
    {
        std::lock_guard<std::mutex> lk(S[0]->mtx);
        S[0]->batch_fallbacks++;
    }
    for (uint32_t i = 0; i < n; i++)
        if (int rc = render_device(S[i], &F[i], rank, nranks, nranks > 1, outs[i], hits ? hits[i] : nullptr, hip_stream,
                                   recs ? &recs[i] : nullptr))
            return rc;
    return RT_OK;
}
} // namespace
} // namespace rtk

using namespace rtk;

extern "C" {

int rt_render_frame_device(rt_scene *s, const rt_frame *f, uint32_t *d_bgra, void *hip_stream)
{
    return render_device(s, f, 0, 1, false, d_bgra, nullptr, hip_stream);
}

int rt_shard_elems(uint32_t width, uint32_t height, uint32_t nranks, uint64_t *elems)
{
    if (!elems || nranks == 0 || width == 0 || height == 0) return fail(RT_E_INVALID, "bad arguments");
    const uint64_t ntiles = uint64_t((width + kTile - 1) / kTile) * ((height + kTile - 1) / kTile);
    *elems = ((ntiles + nranks - 1) / nranks) * kTilePix;
    return RT_OK;
}

int rt_render_shard_device(rt_scene *s, const rt_frame *f, uint32_t rank, uint32_t nranks, uint32_t *d_shard,
                           void *hip_stream)
{
    return render_device(s, f, rank, nranks, true, d_shard, nullptr, hip_stream);
}

int rt_render_batch_device(rt_scene *const *scenes, const rt_frame *frames, uint32_t n, uint32_t rank,
                           uint32_t nranks, uint32_t *const *d_outs, uint32_t *const *d_hits, void *hip_stream)
{
    if (!scenes || !frames || !d_outs || nranks == 0 || rank >= nranks) return fail(RT_E_INVALID, "bad arguments");
    for (uint32_t i = 0; i < n; i++)
    {
        if (!scenes[i] || !d_outs[i]) return fail(RT_E_INVALID, "NULL scene or output");
        if (int rc = validate_frame(&frames[i])) return rc;
    }
    for (uint32_t i = 0; i < n;)
    {
        const uint32_t c = batch_chunk_len(n, i);
        if (int rc = render_batch_chunk(scenes + i, frames + i, c, rank, nranks, d_outs + i,
                                        d_hits ? d_hits + i : nullptr, nullptr, hip_stream))
            return rc;
        i += c;
    }
    return RT_OK;
}

int rt_render_records_device(rt_scene *const *scenes, const rt_frame *frames, uint32_t n, uint32_t rank,
                             uint32_t nranks, uint32_t *const *d_outs, const rt_tile *rects,
                             rt_sample_rec *const *d_recs, void *hip_stream)
{
    if (!scenes || !frames || !d_outs || !rects || !d_recs || n == 0 || nranks == 0 || rank >= nranks)
        return fail(RT_E_INVALID, "bad arguments");
    std::vector<RecOut> ro(n);
    // A records call never overlaps the scene's previous launch (RT_KERNEL_FLAG_OVERLAP is dropped): its
    // fixup below reads the scene's tables after the render and marks the call's end with its own event.
    std::vector<rt_frame> fr(frames, frames + n);
    for (rt_frame& f : fr) f.kernel &= ~uint32_t(RT_KERNEL_FLAG_OVERLAP);
    frames = fr.data();
    for (uint32_t i = 0; i < n; i++)
    {
        if (!scenes[i] || !d_outs[i] || !d_recs[i]) return fail(RT_E_INVALID, "NULL scene, output or record array");
        if (int rc = validate_frame(&frames[i])) return rc;
        if ((frames[i].kernel & RT_KERNEL_KIND_MASK) != RT_KERNEL_AUTO || frames[i].intersector != RT_ISECT_GRID ||
            frames[i].tri_test != RT_TRI_MOLLER_TRUMBORE)
            return fail(RT_E_INVALID, "records come from AUTO's grid / IntersectRayTri path only");
        const rt_tile& r = rects[i];
        if (r.x1 <= r.x0 || r.y1 <= r.y0 || r.x1 > frames[i].width || r.y1 > frames[i].height)
            return fail(RT_E_INVALID, "record rectangle outside the frame or empty");
        ro[i] = RecOut{ d_recs[i], r.x0, r.y0, r.x1 - r.x0, r.y1 - r.y0 };
    }
    if (n == 1)
    {
        if (int rc = render_device(scenes[0], &frames[0], rank, nranks, nranks > 1, d_outs[0], nullptr, hip_stream,
                                   &ro[0]))
            return rc;
    }
    else
        for (uint32_t i = 0; i < n;)
        {
            const uint32_t c = batch_chunk_len(n, i);
            if (int rc = render_batch_chunk(scenes + i, frames + i, c, rank, nranks, d_outs + i, nullptr,
                                            ro.data() + i, hip_stream))
                return rc;
            i += c;
        }
    // the raw records made final (k_record_fixup), per frame on the launch stream
    for (uint32_t i = 0; i < n; i++)
    {
        rt_scene *s = scenes[i];
        std::lock_guard<std::mutex> lk(s->mtx);
        if (int rc = ensure_device(s)) return rc;
        if (int rc = prepare_samples(s, &frames[i], std::max(1u, frames[i].spp))) return rc;
        KParams P;
        frame_params(s, &frames[i], P);
        set_records(P, ro[i]);
        const uint64_t nrec = uint64_t(ro[i].w) * ro[i].h * P.spp;
        if (nrec > 0xFFFFFFFFull) return fail(RT_E_INVALID, "record rectangle too large");
        hipLaunchKernelGGL(record_fixup_kernel(), dim3(uint32_t((nrec + kWG - 1) / kWG)), dim3(kWG), 0,
                           static_cast<hipStream_t>(hip_stream), P, uint32_t(nrec));
        RT_HIP(hipGetLastError());
        // the fixup reads the scene's tables (camera-space x / y, CSR offsets): a later call that
        // rewrites them (prepare_samples -> wait_scene_idle) must wait for it, as for a render launch.
        // Its own completion event (a free one: re-recording an event that the scene still holds as
        // ev_prev would move that mark past the launch it stands for)
        hipEvent_t done = nullptr;
        if (int rc = mark_free(s, nullptr, &done)) return rc;
        RT_HIP(hipEventRecord(done, static_cast<hipStream_t>(hip_stream)));
        s->last_stream = static_cast<hipStream_t>(hip_stream);
    }
    return RT_OK;
}

int rt_render_hits_device(rt_scene *s, const rt_frame *f, uint32_t rank, uint32_t nranks, uint32_t *d_out,
                          uint32_t *d_hits, void *hip_stream)
{
    if (!d_hits) return fail(RT_E_INVALID, "d_hits is NULL");
    return render_device(s, f, rank, nranks, nranks > 1, d_out, d_hits, hip_stream);
}

int rt_unshard_device(uint32_t width, uint32_t height, uint32_t nranks, const uint32_t *d_gathered,
                      uint32_t *d_bgra, void *hip_stream)
{
    if (!d_gathered || !d_bgra || nranks == 0) return fail(RT_E_INVALID, "bad arguments");
    uint64_t elems = 0;
    int rc = rt_shard_elems(width, height, nranks, &elems);
    if (rc) return rc;
    const uint32_t tiles_x = (width + kTile - 1) / kTile;
    hipLaunchKernelGGL(unshard_kernel(), dim3((width + 63) / 64, (height + 3) / 4), dim3(kWG), 0,
                       static_cast<hipStream_t>(hip_stream), d_gathered, d_bgra, width, height, tiles_x, nranks,
                       elems);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

int rt_last_kernel_ms(rt_scene *s, float *ms)
{
    if (!s || !ms) return fail(RT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (s->kt_last >= kTimeRing) return fail(RT_E_INVALID, "no timed kernel recorded yet");
    RT_HIP(hipEventSynchronize(s->kt1[s->kt_last]->ev));
    RT_HIP(hipEventElapsedTime(ms, s->kt0[s->kt_last], s->kt1[s->kt_last]->ev));
    return RT_OK;
}

int rt_scene_set_timing(rt_scene *s, uint32_t every)
{
    if (!s) return fail(RT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    s->time_every = every;
    s->launches = 0;
    return RT_OK;
}

int rt_kernel_times(rt_scene *s, float *ms, uint32_t max_n, uint32_t *n)
{
    if (!s || !n || (max_n && !ms)) return fail(RT_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    const uint32_t cnt = std::min(max_n, s->kt_count);
    const uint32_t next = s->kt_next;
    s->kt_count = 0;                      // consumed whatever happens below
    uint32_t got = 0;
    for (uint32_t i = 0; i < cnt; i++)
    {
        // a pair that cannot be read (a launch that failed between its two records) is skipped
        const uint32_t slot = (next + kTimeRing - cnt + i) % kTimeRing;
        float v = 0.0f;
        if (hipEventSynchronize(s->kt1[slot]->ev) == hipSuccess &&
            hipEventElapsedTime(&v, s->kt0[slot], s->kt1[slot]->ev) == hipSuccess && v >= 0.0f)
            ms[got++] = v;
        else
            (void)hipGetLastError();
    }
    *n = got;
    return RT_OK;
}

int rt_render_tiles(rt_scene *s, const rt_frame *f, const rt_tile *tiles, uint32_t n, uint32_t *const *bufs)
{
    if (!s || (n && (!tiles || !bufs))) return fail(RT_E_INVALID, "NULL argument");
    int rc = validate_frame(f);
    if (rc) return rc;
    if (n == 0) return RT_OK;
    uint32_t bx0 = 0xFFFFFFFFu, by0 = 0xFFFFFFFFu, bx1 = 0, by1 = 0;
    for (uint32_t i = 0; i < n; i++)
    {
        const rt_tile& t = tiles[i];
        if (!bufs[i] || t.x1 <= t.x0 || t.y1 <= t.y0 || t.x1 > f->width || t.y1 > f->height)
            return fail(RT_E_INVALID, "tile outside the frame or empty");
        bx0 = std::min(bx0, t.x0); by0 = std::min(by0, t.y0);
        bx1 = std::max(bx1, t.x1); by1 = std::max(by1, t.y1);
    }
    std::lock_guard<std::mutex> lk(s->mtx);
    if ((rc = ensure_device(s))) return rc;
    const uint32_t spp = std::max(1u, f->spp);
    if ((rc = prepare_samples(s, f, spp))) return rc;
    const uint32_t rw = bx1 - bx0, rh = by1 - by0;
    const size_t words = size_t(rw) * rh;
    if ((rc = ensure_frame(s, words, true))) return rc;
    KParams P;
    frame_params(s, f, P);
    const uint32_t ntiles = region_params(P, bx0, by0, rw, rh, s->d_frame, rw, 0u);
    if ((rc = launch_render(s, f, P, ntiles, s->stream))) return rc;
    // D2H in row bands; band k's rows are scattered into the tiles while band k+1 is in flight
    const uint32_t nb = std::min(kTileBands, rh), bh = (rh + nb - 1) / nb;
    for (uint32_t b = 0; b < nb; b++)
    {
        const uint32_t ya = b * bh, yb = std::min(rh, ya + bh);
        if (ya >= yb) break;
        if (!s->tile_ev[b]) RT_HIP(hipEventCreateWithFlags(&s->tile_ev[b], hipEventDisableTiming));
        RT_HIP(hipMemcpyAsync(s->h_frame + size_t(ya) * rw, s->d_frame + size_t(ya) * rw,
                              size_t(yb - ya) * rw * 4, hipMemcpyDeviceToHost, s->stream));
        RT_HIP(hipEventRecord(s->tile_ev[b], s->stream));
    }
    for (uint32_t b = 0; b < nb; b++)
    {
        const uint32_t ya = by0 + b * bh, yb = std::min(by1, ya + bh);
        if (ya >= yb) break;
        RT_HIP(hipEventSynchronize(s->tile_ev[b]));
        for (uint32_t i = 0; i < n; i++)                         // framebuffer.h:41-45 layout
        {
            const rt_tile& t = tiles[i];
            const uint32_t tw = t.x1 - t.x0;
            for (uint32_t y = std::max(t.y0, ya); y < std::min(t.y1, yb); y++)
                std::memcpy(bufs[i] + size_t(y - t.y0) * tw, s->h_frame + size_t(y - by0) * rw + (t.x0 - bx0),
                            size_t(tw) * 4);
        }
    }
    return RT_OK;
}

int rt_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0) return fail(RT_E_INVALID, "bad arguments");
    *out = nullptr;
    RT_HIP(hipHostMalloc(out, bytes));
    return RT_OK;
}

int rt_host_free(void *p)
{
    if (p) RT_HIP(hipHostFree(p));
    return RT_OK;
}

int rt_render_frame_host(rt_scene *s, const rt_frame *f, uint32_t *h_bgra, const uint32_t *band_y1,
                         uint32_t nbands)
{
    if (!s || !h_bgra || (nbands && !band_y1)) return fail(RT_E_INVALID, "NULL argument");
    int rc = validate_frame(f);
    if (rc) return rc;
    if (nbands > kMaxBands) return fail(RT_E_INVALID, "more than 64 row bands");
    for (uint32_t b = 0; b < nbands; b++)
        if (band_y1[b] == 0 || band_y1[b] > f->height || (b && band_y1[b] <= band_y1[b - 1]) ||
            (b + 1 == nbands && band_y1[b] != f->height))
            return fail(RT_E_INVALID, "band ends must increase strictly and end at the frame height");
    std::lock_guard<std::mutex> lk(s->mtx);
    if ((rc = ensure_device(s))) return rc;
    const uint32_t spp = std::max(1u, f->spp);
    if ((rc = prepare_samples(s, f, spp))) return rc;
    const uint32_t W = f->width, H = f->height;
    if ((rc = ensure_frame(s, size_t(W) * H, false))) return rc;
    KParams P;
    frame_params(s, f, P);
    const uint32_t ntiles = region_params(P, 0, 0, W, H, s->d_frame, W, 0u);
    s->nbands = 0;
    if ((rc = launch_render(s, f, P, ntiles, s->stream))) return rc;
    const uint32_t nb = nbands ? nbands : 1;
    for (uint32_t b = 0, ya = 0; b < nb; b++)
    {
        const uint32_t yb = nbands ? band_y1[b] : H;
        if (!s->band_ev[b]) RT_HIP(hipEventCreateWithFlags(&s->band_ev[b], hipEventDisableTiming));
        RT_HIP(hipMemcpyAsync(h_bgra + size_t(ya) * W, s->d_frame + size_t(ya) * W, size_t(yb - ya) * W * 4,
                              hipMemcpyDeviceToHost, s->stream));
        RT_HIP(hipEventRecord(s->band_ev[b], s->stream));
        s->band_y1[b] = yb;
        ya = yb;
    }
    s->nbands = nb;
    return RT_OK;
}

int rt_render_frame_host_tiled(rt_scene *s, const rt_frame *f, uint32_t *h_tiles, uint32_t tiles_x, uint32_t tiles_y,
                               uint32_t nlaunch)
{
    if (!s || !h_tiles || tiles_x == 0 || tiles_y == 0 || nlaunch == 0) return fail(RT_E_INVALID, "bad arguments");
    int rc = validate_frame(f);
    if (rc) return rc;
    const uint32_t W = f->width, H = f->height;
    if (tiles_y > kMaxBands) return fail(RT_E_INVALID, "more than 64 tile rows");
    // row-band launches of one scene overlap on two streams and share its scene-wide debug and
    // wide-section buffers (wave clocks from index 0, the side stream's fork / join): one launch only
    if (nlaunch > 1u && (f->kernel & (RT_KERNEL_FLAG_WAVE_CLOCK | RT_KERNEL_FLAG_WIDE_HEAVY)))
        return fail(RT_E_INVALID, "row-band launches (nlaunch > 1) take neither WAVE_CLOCK nor WIDE_HEAVY");
    std::lock_guard<std::mutex> lk(s->mtx);
    if ((rc = ensure_device(s))) return rc;
    const uint32_t spp = std::max(1u, f->spp);
    if ((rc = prepare_samples(s, f, spp))) return rc;
    if ((rc = ensure_frame(s, size_t(W) * H, false))) return rc;
    if (!s->stream2)
    {
        RT_HIP(hipStreamCreateWithFlags(&s->stream2, hipStreamNonBlocking));
        RT_HIP(hipEventCreateWithFlags(&s->ev_t_fork, hipEventDisableTiming));
        RT_HIP(hipEventCreateWithFlags(&s->ev_t_join, hipEventDisableTiming));
    }
    // Framebuffer::Resize's tile rows (framebuffer.cpp:106-117): row r spans [r * th, (r + 1) * th),
    // the last one to H; launch j renders tile rows [j * R / n, (j + 1) * R / n)
    const uint32_t tw = W / tiles_x, th = H / tiles_y;
    const uint32_t nl = std::min(nlaunch, tiles_y);
    auto row_y = [&](uint32_t r) { return r >= tiles_y ? H : r * th; };
    hipStream_t st[2] = { s->stream, s->stream2 };
    // both streams after everything earlier on this scene (the scene's tables and records are shared)
    if (s->ev_recorded)
    {
        RT_HIP(hipStreamWaitEvent(st[0], s->ev_last->ev, 0));
        if (s->ev_prev) RT_HIP(hipStreamWaitEvent(st[0], s->ev_prev->ev, 0));
        s->ev_prev.reset();
    }
    rtk::fref_ordered(s->fref);                 // (so either per-origin record buffer may be recomputed)
    s->miss_busy = s->miss_last = 0u;           // (and either miss mask; the row-band launches below add theirs)
    KParams P0;
    frame_params(s, f, P0);
    if (use_lanes(f, spp) && P0.isect == RT_ISECT_GRID && P0.tri_test == RT_TRI_MOLLER_TRUMBORE &&
        ((f->kernel & RT_KERNEL_KIND_MASK) == RT_KERNEL_AUTO || (f->kernel & RT_KERNEL_KIND_MASK) == RT_KERNEL_COMPACT))
    {
        uint32_t used = 0;                      // (every launch before this one is waited for above)
        if ((rc = ensure_origin_terms(s, P0, st[0], 0u, &used))) return rc;
        rtk::fref_launched(s->fref, used);
    }
    if ((rc = flush_tables(s, st[0]))) return rc;      // before the fork: both streams read them
    RT_HIP(hipEventRecord(s->ev_t_fork, st[0]));
    RT_HIP(hipStreamWaitEvent(st[1], s->ev_t_fork, 0));
    s->nbands = 0;
    for (uint32_t j = 0; j < nl; j++)
    {
        const uint32_t r0 = j * tiles_y / nl, r1 = (j + 1) * tiles_y / nl;
        const uint32_t ya = row_y(r0), yb = row_y(r1);
        if (ya >= yb) continue;
        KParams P = P0;
        const uint32_t ntiles = region_params(P, 0, ya, W, yb - ya, s->d_frame, W, 2u);
        P.fb_tw = tw; P.fb_th = th; P.fb_tx = tiles_x; P.fb_ty = tiles_y;
        P.fb_mtw = tw ? uint32_t(((1ull << 32) + tw - 1) / tw) : 0u;
        P.fb_mth = th ? uint32_t(((1ull << 32) + th - 1) / th) : 0u;
        // launches alternate between the two streams, so one launch's tail overlaps the next one's
        // start and its tile rows' copy-back overlaps the next launch's render
        hipStream_t sj = st[j & 1u];
        if ((rc = launch_render(s, f, P, ntiles, sj, false))) return rc;
        // the launch's tile rows are words [ya * W, yb * W) of the tile layout: ONE contiguous copy
        // (a copy per tile row cost ~14 us of launch overhead each, measured: 9 copies of a whole
        // frame 0.50 ms vs one 0.37, profiles/r04l_e2e_breakdown.json)
        const uint32_t b = s->nbands;
        if (!s->band_ev[b]) RT_HIP(hipEventCreateWithFlags(&s->band_ev[b], hipEventDisableTiming));
        RT_HIP(hipMemcpyAsync(h_tiles + size_t(ya) * W, s->d_frame + size_t(ya) * W, size_t(yb - ya) * W * 4,
                              hipMemcpyDeviceToHost, sj));
        RT_HIP(hipEventRecord(s->band_ev[b], sj));
        s->band_y1[b] = yb;
        s->nbands = b + 1;
    }
    // the frame is done when both streams are: join on the first one, whose event ev1 marks it
    RT_HIP(hipEventRecord(s->ev_t_join, st[1]));
    RT_HIP(hipStreamWaitEvent(st[0], s->ev_t_join, 0));
    if ((rc = mark_own(s, st[0]))) return rc;
    s->last_stream = st[0];
    // bands land per tile row but not in row order across the two streams: rt_frame_host_wait(y1)
    // needs every row below y1, so a band's wait covers the bands before it (events in row order)
    return RT_OK;
}

int rt_frame_host_wait(rt_scene *s, uint32_t y1)
{
    if (!s) return fail(RT_E_INVALID, "NULL argument");
    hipEvent_t ev[kMaxBands];
    uint32_t n = 0;
    {
        std::lock_guard<std::mutex> lk(s->mtx);
        if (s->nbands == 0) return fail(RT_E_INVALID, "no rt_render_frame_host in flight");
        // every band below y1 (rt_render_frame_host_tiled's bands land from two streams, so a later
        // band may be done before an earlier one); a finished event costs nothing to wait on
        while (n < s->nbands && (n == 0 || s->band_y1[n - 1] < y1)) { ev[n] = s->band_ev[n]; n++; }
    }
    for (uint32_t b = 0; b < n; b++)
        RT_HIP(hipEventSynchronize(ev[b]));     // events are only re-recorded by a later frame
    return RT_OK;
}

} // extern "C"
