// rt_lane_run.h -- the per-lane run of grid_intersect's box walk: from the three
// lower bounds of a box's exit crossings (box_exit_bound, rt_walk.h) the run's limit tl, then per axis the
// add chain x, fl(x + dt), ... while x < tl, and the chains' step counts packed as c0 | c1 << 11 | c2 << 22
// (the box counts' layout).
//
// Plain float / int, no HIP types: librt_tracer.so runs these functions (grid_intersect, wide_trace) and
// tests/lane_chain_check.cpp compiles the same ones with g++ over 64-lane value types.  What differs between
// the two -- the wave vote and the lane mask -- comes in through the two hooks of a wave type W:
//   W::any(p)         wave-uniform: does p hold in some active lane (W::count(p): in how many)
//   W::pick(p, a, b)  per lane: a where p holds, else b
// (box_exit_bound itself stays in rt_walk.h: tests/test_build_guard.py pins its two fused operations there;
// this header has none.)
//
// ---- what a run computes ----------------------------------------------------------------------------
// The reference form is three guarded loops per lane,
//     while (x_a < tl && c_a < f_a) { x_a += dt_a; c_a++; }                        (lane_chain_guarded)
// with f_a the box's count along axis a.  The lean form (lane_chain_lean) runs the wave through
// wave-uniform trips: every trip adds in the lanes whose x_a < tl still holds and keeps x_a, c_a in the
// others (a select of the old value, not an add of 0: exact whatever x_a holds), and the trip loop ends
// when the compare is false in every active lane.  A lane's compare only ever goes from true to false --
// once false, x_a no longer changes -- so per lane these are the guarded loop's adds, in the same order,
// c_a single IEEE additions, as long as the guard c_a < f_a never ends the guarded loop first.
//
// ---- when the guard is implied: the vote ------------------------------------------------------------
// The guard ends a guarded loop first iff x_a(k) < tl for every k = 0 .. f_a, in particular
// x_a(f_a) < tl.  box_exit_bound's derivation (rt_walk.h, grid_intersect) gives b_a <= x_a(f_a)
// whenever its own arithmetic stayed finite.  A b_a that is a number (not a NaN) is either -inf or finite.
// b_a = -inf (x_a = -inf, or dt_a = -inf with f_a > 0: e_a = -inf, and -inf less a margin of +inf stays -inf)
// makes tl = -inf: no x < tl, no step on any axis in either form.  A finite b_a needs x_a finite and
// fl(f_a dt_a + x_a) finite -- so dt_a is finite too: the fused 0 * inf + x and f * NaN + x are NaN, and a +inf
// e_a less its +inf margin is NaN -- and a finite margin; then every rounding the derivation counts is a rounding
// to nearest of a finite sum and the bound holds.  (x_a(f_a) itself may have rounded up to +inf next to FLT_MAX;
// +inf >= tl all the same.  dt_a < 0 does not occur in a walk; it gives b_a <= e_a <= x_a and no step in either
// form.)
// tl = fminf(fminf(b_0, b_1), b_2) skips NaN operands, so tl <= b_a for every b_a that is a number.  Hence
//     (V)  no b_a of the lane is a NaN   ==>   x_a(f_a) >= b_a >= tl for a = 0, 1, 2
// and under (V) the first k with !(x_a(k) < tl) is <= f_a: the guard is never what ends the loop.  That
// holds for a stuck chain too (fl(x + dt) == x): its x_a(f_a) is x_a, and (V) says x_a >= tl, no step.
// A NaN b_a arises from a NaN or infinite crossing or step, or from f_a dt_a + x_a beyond FLT_MAX (a
// direction component below ~1e-35 of the others: dt_a = cw / d_a); then tl may lie above x_a(f_a) and the
// guard counts.  The vote is wave-uniform and taken once per run: when (V) fails in any active lane the
// whole wave takes the guarded loops.  Every frame of an orthonormal camera passes (V) in every run.
//
// ---- bounds whatever the data -----------------------------------------------------------------------
// A field holds at most 1,023, so under (V) a chain takes at most 1,023 trips; the trip loop counts blocks
// down from kLaneChainBlocks (wave-uniform) and cannot run longer whatever x, dt and tl hold.  After the
// lean chains c_a is clamped to f_a (a no-op under (V)): a run never moves further than the box's own
// counts, which is what keeps grid_intersect's `cell` inside the ray's copy of the grid.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RT_LRUN_FN __device__ __forceinline__
#else
#define RT_LRUN_FN inline
#endif

// trips per block of the lean loop: one vote and one exit branch per block
#ifndef RT_LANE_CHAIN_UNROLL    // (tools/build_variant.sh -DRT_LANE_CHAIN_UNROLL=n: the A/B arms; 0: the guarded loops)
#define RT_LANE_CHAIN_UNROLL 4
#endif

namespace rtk {

constexpr int kLaneChainUnroll = RT_LANE_CHAIN_UNROLL;
constexpr int kLaneFieldMax = 1023;         // the largest count a box field holds
// blocks that cover kLaneFieldMax + 1 trips: the lean loop's hard bound
constexpr int kLaneChainBlocks = kLaneChainUnroll > 0 ? (kLaneFieldMax + kLaneChainUnroll) / kLaneChainUnroll : 0;

// The reference form of one axis, per lane (also what a wave that fails the vote runs).
RT_LRUN_FN void lane_chain_guarded(float& x, float dt, float tl, int f, int& c)
{
    while (x < tl && c < f) { x += dt; c++; }
}

// The lean form of one axis for the whole wave; F, I: a lane's float and int (the checker's: 64 of them).
template <class W, class F, class I>
RT_LRUN_FN void lane_chain_lean(F& x, const F& dt, const F& tl, I& c)
{
    auto a = x < tl;
    if (!W::any(a)) return;
    int blocks = kLaneChainBlocks;
#if defined(__clang__)
#pragma unroll 1    // (the block IS the unrolling: left alone the compiler unrolls the block loop four times more)
#endif
    do
    {
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < kLaneChainUnroll; j++)
        {
            x = W::pick(a, x + dt, x);
            c = W::pick(a, c + 1, c);
            a = x < tl;
        }
        // One exit on one scalar word: min(blocks - 1, lanes still adding << 10) is blocks - 1 while a lane adds
        // (1 << 10 exceeds every budget) and 0 when none does.  Written as `any(a) && --blocks != 0` the compiler
        // builds both conditions as lane masks: two s_cselect_b64, an s_or_b64 and an s_andn2_b64 per block.
        const uint32_t live = W::count(a) << 10;
        blocks = uint32_t(blocks - 1) < live ? blocks - 1 : int(live);
    } while (blocks != 0);
}

// The run's limit: the least of the three bounds (fminf skips a NaN).
RT_LRUN_FN float lane_run_limit(float b0, float b1, float b2)
{
    return __builtin_fminf(__builtin_fminf(b0, b1), b2);
}

// (V) for the wave, as two votes on single compares (a compare's lane mask is its ballot; a predicate
// combined per lane would be materialised in a VGPR and compared back, rt_wave.h wave_all): no active
// lane holds a NaN bound.
RT_LRUN_FN bool lane_unordered(float a, float b) { return __builtin_isunordered(a, b); }
template <class W, class F>
RT_LRUN_FN bool lane_run_proven(const F& b0, const F& b1, const F& b2)
{
    return !(W::any(lane_unordered(b0, b1)) | W::any(lane_unordered(b2, b2)));
}

RT_LRUN_FN int lane_run_pack(int c0, int c1, int c2) { return c0 + (c1 << 11) + (c2 << 22); }

// The three chains of a run.  `proven`: lane_run_proven of the wave -- the lean chains, else the guarded loops.
template <class W, class F, class I>
RT_LRUN_FN void lane_run_chains(bool proven, F& x0, F& x1, F& x2, const F& dt0, const F& dt1, const F& dt2,
                                const F& tl, const I& f0, const I& f1, const I& f2, I& c0, I& c1, I& c2)
{
    if (kLaneChainUnroll > 0 && proven)
    {
        lane_chain_lean<W>(x0, dt0, tl, c0);
        lane_chain_lean<W>(x1, dt1, tl, c1);
        lane_chain_lean<W>(x2, dt2, tl, c2);
        c0 = W::pick(f0 < c0, f0, c0);
        c1 = W::pick(f1 < c1, f1, c1);
        c2 = W::pick(f2 < c2, f2, c2);
    }
    else
    {
        lane_chain_guarded(x0, dt0, tl, f0, c0);
        lane_chain_guarded(x1, dt1, tl, f1, c1);
        lane_chain_guarded(x2, dt2, tl, f2, c2);
    }
}

#if defined(__HIPCC__)
// The device's wave: the vote is a ballot of exec's lanes, the mask a select.
struct LaneWave
{
    static __device__ __forceinline__ bool any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
    static __device__ __forceinline__ uint32_t count(bool p) { return uint32_t(__builtin_popcountll(__builtin_amdgcn_ballot_w64(p))); }
    template <class T>
    static __device__ __forceinline__ T pick(bool p, T a, T b) { return p ? a : b; }
};

// One lane's run inside a box (boxw: its counts, no guard set; b0..b2: box_exit_bound of the three axes):
// moves the crossing times along their chains and returns the steps taken in the box counts' layout.
// LEAN false: the guarded loops alone, no vote (the wide section, rt_kernels.hip wide_trace: with both forms
// in them its kernels stand at 66 VGPRs for 64, a wave per SIMD).
template <bool LEAN = true>
__device__ __forceinline__ int lane_run(float& nct0, float& nct1, float& nct2, float dt0, float dt1, float dt2,
                                        float b0, float b1, float b2, int f0, int f1, int f2)
{
    const float tl = lane_run_limit(b0, b1, b2);
    int c0 = 0, c1 = 0, c2 = 0;
    lane_run_chains<LaneWave>(LEAN && lane_run_proven<LaneWave>(b0, b1, b2), nct0, nct1, nct2, dt0, dt1, dt2, tl, f0,
                              f1, f2, c0, c1, c2);
    return lane_run_pack(c0, c1, c2);
}
#endif

}  // namespace rtk
