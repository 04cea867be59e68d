// rt_launch.h -- what the library's three host files share (not part of the ABI): rt_tracer.hip (ABI basics,
// rt_scene_create / destroy, rt_debug_*), rt_launch.hip (events and ordering, frame tables, the render launches
// and the copy-back paths) and rt_queries.hip (samples, rays, occlusion, distance, marches, primary rays, AO).  DESIGN.md
// §4.34 says which of these a new entry point must call.
#pragma once
#include <string>
#include <vector>

#include "rt_scene.h"

namespace rtk {

// rt_internal_fail (rt_tracer.hip: sets the thread-local message rt_last_error returns; returns `code`) by the name
// the host files call it
inline int fail(int code, const std::string& msg) { return rt_internal_fail(code, msg); }

inline bool is_pow2(uint32_t x) { return x && !(x & (x - 1)); }

inline uint32_t log2u(uint32_t x)
{
    uint32_t r = 0;
    while ((1u << r) < x) r++;
    return r;
}

// ---- rt_tracer.hip
// sampling.h:113-120, sampling.cpp:194-210 (base 2), renderer.cpp:52-55
void hammersley(uint32_t spp, std::vector<float>& xy);

// ---- rt_launch.hip: a call's first steps, in this order, under the scene's mutex
int validate_frame(const rt_frame *f);
int ensure_device(const rt_scene *s);
// The frame's camera-space and sample tables (no host work when they are the scene's current ones)
int prepare_samples(rt_scene *s, const rt_frame *f, uint32_t spp);
// The per-frame parameters (camera constants exactly as camera.h computes them; P is zeroed first) ...
void frame_params(const rt_scene *s, const rt_frame *f, KParams& P);
// ... and the scene's own arrays and grid constants, frame_params' second half
void scene_params(const rt_scene *s, KParams& P);
// The traversal features that need a scene property (on top of kVarAutoCore, or of kVarRays)
int scene_traversal_bits(const rt_scene *s);

// The region of the frame a launch renders, as whole-frame tiles dealt to one rank (a shard's caller sets P.rank /
// P.nranks after it); returns the region's tile count
inline uint32_t region_params(KParams& P, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t *out, uint32_t pitch,
                              uint32_t shard_mode)
{
    P.rx0 = x0; P.ry0 = y0; P.rw = w; P.rh = h;
    P.tiles_x = (w + kTile - 1) / kTile;
    P.rank = 0; P.nranks = 1;
    P.out = out; P.pitch = pitch; P.shard_mode = shard_mode;
    return P.tiles_x * ((h + kTile - 1) / kTile);
}

// Per-sample records requested from the product kernels (rt_render_records_device, rt_trace_samples): the
// rectangle's samples land in d[((y - y0) * w + (x - x0)) * spp + s].
struct RecOut { rt_sample_rec *d; uint32_t x0, y0, w, h; };

inline void set_records(KParams& P, const RecOut& r)
{
    P.recs = r.d;
    P.rec_x0 = r.x0;
    P.rec_y0 = r.y0;
    P.rec_w = r.w;
    P.rec_h = r.h;
}

// The launch shape of a lane kernel over P's region and shard (set before it): wg_per_tile workgroups a tile, and
// the band map of a launch of total_blocks lane blocks (a batch: every frame's).
// kVarXcdBands turn size: one row of this launch's tiles (ceil(tiles_x / nranks) local tiles
// span a full frame row in shard mode).  Measured best of 1/4 .. 4 rows and 1..16 tiles:
// whole rows interleave over the XCDs, so each L2 sees compact rows AND the frame's cost
// spreads evenly (half rows put every left half on the even XCDs).
inline void launch_shape(KParams& P, uint32_t wg_per_tile, uint32_t total_blocks)
{
    P.wg_per_tile = wg_per_tile;
    P.ipt_shift = log2u(wg_per_tile * kWavesPerWG);
    P.tiles_x_m = udiv_magic(P.tiles_x);
    P.xcd_chunk = ((P.tiles_x + P.nranks - 1u) / P.nranks) * wg_per_tile;
    // ... and the band map's two quotients, once per launch (xcd_band_block): the launch's lane blocks are
    // total_blocks with a front (the grid's hf_front blocks more lead it) and without one
    P.xcd_chunk_m = udiv_magic(P.xcd_chunk);
    P.xcd_full = xcd_band_full(total_blocks, P.xcd_chunk);
}

// Writes the frame tables of prepare_samples' device path on st, if any are pending
int flush_tables(rt_scene *s, hipStream_t st);
// A launch of the scene on st that reads its frame tables and no per-origin records: ordered after every launch
// that may still read the old tables (order_all), the tables written (flush_tables), and itself the scene's last
// launch.  The caller launches its kernel and marks its end with one of the two below.
int begin_table_launch(rt_scene *s, hipStream_t st);
// A launch's end, recorded on st after it in the scene's own event
int mark_own(rt_scene *s, hipStream_t st);
// A launch's end in an event that nothing still holds -- the timed launch's stop event (timed_stop, begin_timed),
// else a free one of ev_done[] --: *stop is for the dispatch to carry (hipExtLaunchKernelGGL: no marker packet), or
// for the caller to record after its kernel
int mark_free(rt_scene *s, const EvRef *timed_stop, hipEvent_t *stop);
// a new shared event (rt_scene::ev_last and its sources)
int new_event(EvRef& r, unsigned flags);

} // namespace rtk
