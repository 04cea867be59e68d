// rt_walk.h -- the grid walk, for every kernel that traces a ray: the reference's Grid::Intersect
// (3D-DDA over the packed cell words, box runs, the per-camera-record ray/triangle tests) as
// grid_intersect over dda_setup, test_cell and the DDA step macros.  See DESIGN.md §4.1-4.13; the
// layers above it are rt_frame_isect.h, rt_item_coord.h and rt_item.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "rt_device.h"
#include "rt_kparams.h"
#include "rt_lane_run.h"
#include "rt_record_gate.h"
#include "rt_setup_div.h"
#include "rt_wave.h"

// grid_intersect's per-lane runs take rt_lane_run.h's lean add chains; a unit that defines this false before
// including the walk keeps the guarded loops alone (rt_ao.hip says why it does)
#ifndef RT_WALK_LEAN_CHAINS
#define RT_WALK_LEAN_CHAINS true
#endif

namespace rtk {
namespace {

// kVarLdsSplit: cell lists shorter than this (in every lane) are tested whole by every wave, with no
// reduction; longer ones are split between the workgroup's waves
#ifndef RT_LDS_SPLIT_MIN       // (tools/build_variant.sh -DRT_LDS_SPLIT_MIN=n: the A/B arms)
#define RT_LDS_SPLIT_MIN 8
#endif
constexpr uint32_t kLdsSplitMin = RT_LDS_SPLIT_MIN;

// CSR range of a cell: one u32 load of the packed (start << 11 | count) word when the scene
// fits the packing (every scene of the reference does), else the two CSR offsets (a cell of
// >= 2,048 references or >= 2^21 in all: tests/test_gpu_variants.py B1 walks that side).
__device__ __forceinline__ void cell_range(const KParams& P, uint32_t cell, uint32_t& kb, uint32_t& ke)
{
    if (P.cellw)
    {
        const uint32_t w = P.cellw[cell];
        const uint32_t cnt = w & 2047u;
        kb = cnt ? (w >> 11) : 0u;
        ke = kb + cnt;
    }
    else
    {
        kb = P.off[cell];
        ke = P.off[cell + 1];
    }
}

typedef float vf4 __attribute__((ext_vector_type(4)));
// constant address space: uniform loads of memory no store of the render kernels touches (frefs
// are written by k_origin_pre, an earlier launch) select s_load through the scalar cache
typedef const __attribute__((address_space(4))) vf4 cvf4;
typedef float vf16 __attribute__((ext_vector_type(16)));    // one 64-byte record in 16 SGPRs

// The per-lane list loop of the per-camera-record test: this lane's list [kb, ke) in order
// (grid.cpp:243-267), lowering tb on every accepted hit.  The first-half terms (r0..r2) per
// iteration, the second-half terms (r3) only when the gate passes.  Measured against a one-ahead
// prefetch in VGPRs (+12, 6 waves/SIMD) and by LDS-DMA into a per-wave slot
// (global_load_lds_dwordx4; no VGPRs, but four DMA issues per record): both slower on the frame
// and no shorter on the lone heavy waves (profiles/r02e_ab_lane_prefetch.json).
// (kVarLdsSplit: this wave's share kb + first, kb + first + step, ... of the list)
template <bool STATS, int VAR>
__device__ __forceinline__ void lane_list(const KParams& P, rtd::f2v ra, rtd::f2v rc, uint32_t kb, uint32_t ke,
                                          float& tb, float& u, float& v, uint32_t& tri, uint32_t& tests,
                                          uint32_t first = 0u, uint32_t step = 1u)
{
    constexpr bool F = (VAR & kVarFastRcp) != 0;
    constexpr bool SPLIT = (VAR & kVarLdsSplit) != 0;
    for (uint32_t k = kb + (SPLIT ? first : 0u); k < ke; k += (SPLIT ? step : 1u))
    {
        if constexpr ((VAR & kVarWaveClock) != 0)
            if (first_active_lane()) wave_counters()[1] += 1u;
        if (STATS) tests++;
        const float4 *rp = P.frefs + size_t(k) * 4u;     // one address, immediate offsets
        const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
        float inv, pu;
        const bool ok1 = rtd::mt_rec_first<F>(ra, rc, rtd::f2v{r0.x, r0.y}, rtd::f2v{r0.z, r0.w},
                                              rtd::f2v{r1.x, r1.y}, rtd::f2v{r1.z, r1.w},
                                              rtd::f2v{r2.x, r2.y}, inv, pu);
        if (__any(ok1))
        {
            const float2 r3 = *reinterpret_cast<const float2 *>(rp + 3);
            float pv, pt;
            const bool h = ok1 & rtd::mt_rec_second(ra, rc, rtd::f2v{r2.z, r2.w}, r3.x, r3.y, inv, pu, pv, pt);
            const bool take = h & (pt < tb);
            tb = take ? pt : tb;
            u = take ? pu : u;
            v = take ? pv : v;
            tri = take ? k : tri;
        }
    }
}

// Tests a cell's list [kb, ke) in order (grid.cpp:243-267); true when it produced a hit.
// grid.cpp:258-260 accepts cur_t when cur_t < t && cur_t < next_crossing_t[step_axis].  t is
// FLT_MAX on entry (a hit ends the walk, grid.cpp:270-271) and neither bound is ever NaN, so the
// two compares are one against tb = min(t, nct_ax), which every accepted hit lowers to its t:
// the same hits are taken in the same order (strict '<' keeps the first of equal t, H8).
//
// kVarLdsSplit (the wide section's LDS tier, wide_item_lds): the workgroup's waves hold the same rays in
// the same walk state, so they reach every call with the same lanes and lists.  When some lane's list
// has kLdsSplitMin references or more (a vote, so alike in every wave), wave w tests only positions
// kb + w, kb + w + 4, ...; each lane's local first minimum (t, position) is written to LDS, and after a
// workgroup barrier every wave takes the lexicographic minimum over the four (smaller t, then the lower
// list position: the reference's first minimum, H8) with its u, v.  The buffers alternate by parity
// (lpar), so one barrier per reduction suffices: a wave can only overwrite a buffer after every wave
// has passed the next barrier, i.e. finished reading it.
template <bool STATS, int TRI, int VAR>
__device__ __forceinline__ bool test_cell(const KParams& P, float ox, float oy, float oz, float dx, float dy,
                                          float dz, uint32_t kb, uint32_t ke, float nct_ax, float& t,
                                          float& u, float& v, uint32_t& tri, uint32_t& tests, uint32_t& lpar,
                                          float tmin = 0.0f, float t_in = 0.0f)
{
    constexpr bool PRE = (VAR & kVarOriginPre) != 0 && TRI == RT_TRI_MOLLER_TRUMBORE;
    constexpr bool F = (VAR & kVarFastRcp) != 0;
    constexpr bool SPLIT = (VAR & kVarLdsSplit) != 0;
    // kVarAnyHit (rt_occluded_rays_device): t holds the ray's tmax and is never lowered, so tb below is
    // min(tmax, nct_ax); a test counts when it also lies above tmin, and the first one that counts ends the
    // lane's list (true).  u, v, tri are not written.
    constexpr bool ANY = (VAR & kVarAnyHit) != 0;
    static_assert(!SPLIT || (PRE && !STATS), "the LDS tier runs AUTO's record test");
    static_assert(!ANY || ((VAR & kVarRays) != 0 && (VAR & kVarWaveGate) != 0 && !PRE && !STATS &&
                           TRI == RT_TRI_MOLLER_TRUMBORE), "the any-hit walk is the ray queries' fast arm");
    // kVarCross (rt_crossing_rays_device): t holds tmax as above; a test counts when it lies in (tmin, tmax) AND in
    // the cell's own interval [t_in, nct_ax), t_in the crossing the walk took into this cell.  Every counted test
    // adds one to tri (the ray's count) and, where det > 0, one to tests (its front count); nothing ends the list.
    constexpr bool CROSS = (VAR & kVarCross) != 0;
    static_assert(!CROSS || (!ANY && (VAR & kVarRays) != 0 && (VAR & kVarWaveGate) != 0 && !PRE && !STATS &&
                             TRI == RT_TRI_MOLLER_TRUMBORE), "the counting walk is the ray queries' fast arm");
    (void)lpar;
    (void)t_in;
    // wave-uniform, and the same in every wave of the workgroup (their lanes and lists are the same)
    bool split = false;
    if constexpr (SPLIT) split = __any(ke - kb >= kLdsSplitMin);
    const uint32_t first = split ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0u, step = split ? kWavesPerWG : 1u;
    rtd::f2v ra = {dx, dy}, rc = {dy, dz};         // the ray as the record test's register pairs
    // min(t, nct_ax) as a compare and select: neither is ever NaN (and -0 / +0 compare equal in
    // every later '<'), and fminf would canonicalise both operands first (2 more VALU per cell)
    const float tb0 = t < nct_ax ? t : nct_ax;
    // every accepted hit lowers tb strictly, so "some hit was taken" is tb < tb0; u, v and tri
    // are updated in place (the caller's values stand when nothing is taken)
    float tb = tb0;
    bool uniform_done = false;                // wave-uniform
    if constexpr ((VAR & kVarUniform) != 0 && PRE)
    {
        // Wave-uniform list: every lane testing this step sits in the same cell (the common case
        // in dense geometry: a wave is a 4x4-pixel x 4-sample block).  The loop runs on scalar
        // registers and the records arrive through the scalar cache (s_load), off the
        // vector-memory path; results are the same ray/record pairs in the same order.
        const uint32_t kb0 = __builtin_amdgcn_readfirstlane(kb), ke0 = __builtin_amdgcn_readfirstlane(ke);
        // one integer compare for the vote (the empty asm keeps the compiler from splitting it
        // back into two equalities, which materialises the combined predicate in a VGPR)
        uint32_t diff = (kb ^ kb0) | (ke ^ ke0);
        asm volatile("" : "+v"(diff));
        if (wave_all(diff == 0u))
        {
            if constexpr ((VAR & kVarWaveClock) != 0)
                if (first_active_lane()) wave_counters()[0] += ke0 - kb0;
            cvf4 *crefs = (cvf4 *)P.frefs;
            const uint32_t kfirst = kb0 + (SPLIT ? first : 0u), kstep = SPLIT ? step : 1u;
            if (!SPLIT || kfirst < ke0)
            {
                // software pipeline over two register sets in turn: record k + 1 is in flight
                // while record k is tested, with no per-record register copies (scalar loads may
                // return out of order, so each set is waited for where it is first read)
                //
                // rec_k: list position of the record `ahead` records past p (formed where a hit is
                // taken: the empty asm keeps it from becoming a second loop counter)
                auto rec_k = [&](cvf4 *p, uint32_t ahead) {
                    uint64_t d = uint64_t(p) - uint64_t(crefs);
                    asm("" : "+s"(d));
                    return uint32_t(d >> 6) + ahead;
                };
                auto test_rec = [&](const vf4 r0, const vf4 r1, const vf4 r2, const vf4 r3, auto pos) {
                    if (STATS) tests++;
                    // the gate skips the record's second half AND the acceptance for the whole
                    // wave when no lane passes det and u (the common case in a dense cell)
                    float inv, cu;
                    const bool ok1 = rtd::mt_rec_first<F>(ra, rc, rtd::f2v{r0.x, r0.y}, rtd::f2v{r0.z, r0.w},
                                                          rtd::f2v{r1.x, r1.y}, rtd::f2v{r1.z, r1.w},
                                                          rtd::f2v{r2.x, r2.y}, inv, cu);
                    if (__any(ok1))
                    {
                        float cv, ct;
                        const bool hit = ok1 & rtd::mt_rec_second(ra, rc, rtd::f2v{r2.z, r2.w}, r3.x, r3.y, inv, cu,
                                                                  cv, ct);
                        const bool take = hit & (ct < tb);
                        tb = take ? ct : tb;
                        u = take ? cu : u;
                        v = take ? cv : v;
                        const uint32_t k = pos();          // wave-uniform, outside the select
                        tri = take ? k : tri;
                    }
                };
                cvf4 *np = crefs + size_t(kfirst) * 4u;
                if constexpr (!SPLIT)
                {
                    // A running record pointer over PAIRS of records, then the odd one: the loop has
                    // one exit, so its test is one scalar compare and branch per two records (a
                    // second exit in the middle makes the compiler carry the exit condition as a
                    // lane mask).  The next record is ALWAYS loaded: the buffers end in kFrefPad
                    // zero records (rt_kparams.h), so the load one record past the list's end is in
                    // bounds, and what it returns is never tested.  The list position is formed
                    // only where a hit is taken (rec_k).  The loads and their waits are asm
                    // statements, which keep their order: written as plain loads, the compiler
                    // sinks each load to its first use and the pipeline is gone.  Each wait names
                    // the set it is for, so that set is read after it and stays allocated until its
                    // load has returned (the last load's data is dropped).
                    const uint32_t n = ke0 - kb0;
                    vf16 a, b;
                    cvf4 *const cgates = (cvf4 *)P.gates;
                    bool gated = false;             // wave-uniform
                    if constexpr (!STATS) gated = n >= kGateMinList && cgates != nullptr;
                    if (gated)
                    {
                        // The gated loop (rt_record_gate.h), for long lists (few of
                        // whose records any lane's first half passes): the same pipeline over the
                        // records' 32-byte gate records, a PAIR of them per 16-register set and one
                        // vote per pair.  A lane the gate rejects fails the record's det / u test, so a
                        // record every active lane rejects would leave every lane as it is: it is
                        // skipped unloaded.  Any other record is loaded into the set its gate pair
                        // came in -- the pair's compares have issued, the set is free until the next
                        // gate load into it -- and takes test_rec unchanged, record a before record b:
                        // the same hits in the same order.  The gate loads run up to three records past
                        // the list's end, inside the gate array's zero pad (gate_buffer_bytes); a
                        // record past the end is never tested (`two`).
                        // The loop counts the list position k (of the set's first record) beside the
                        // gate pointer, so a record's address is one shift away: crefs + (k << 6) as base
                        // and 32-bit offset (the host passes a gate pointer only while the record buffer is
                        // below 4 GiB).
                        cvf4 *gp = cgates + size_t(kb0) * 2u;
                        uint32_t k = kb0;
                        const uint32_t kend = kb0 + (n & ~3u);
                        auto gate_pair = [&](vf16& s, uint32_t ahead, bool two) {
                            using rtd::f2v;
                            // the direction from the ray's pairs, opaque here: the products then select
                            // an element of the pair (op_sel), where loop-invariant (d, d) pairs would be
                            // hoisted into six more VGPRs
                            asm("" : "+v"(ra), "+v"(rc));
                            const bool ja = gate_rejects(ra.x, ra.y, rc.y, f2v{s[0], s[1]}, f2v{s[2], s[3]},
                                                         f2v{s[4], s[5]}, s[6]);
                            const bool jb = gate_rejects(ra.x, ra.y, rc.y, f2v{s[8], s[9]}, f2v{s[10], s[11]},
                                                         f2v{s[12], s[13]}, s[14]);
                            const uint64_t ma = __builtin_amdgcn_ballot_w64(!ja);
                            const uint64_t mb = two ? __builtin_amdgcn_ballot_w64(!jb) : 0ull;
                            if ((ma | mb) != 0ull)
                            {
                                if (ma != 0ull)
                                {
                                    const uint32_t ro = (k + ahead) << 6;
                                    asm volatile("s_load_dwordx16 %0, %1, %2" : "=&s"(s) : "s"(crefs), "s"(ro));
                                    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(s));
                                    test_rec(vf4{s[0], s[1], s[2], s[3]}, vf4{s[4], s[5], s[6], s[7]},
                                             vf4{s[8], s[9], s[10], s[11]}, vf4{s[12], s[13], s[14], s[15]},
                                             [&] { return k + ahead; });
                                }
                                if (mb != 0ull)
                                {
                                    const uint32_t ro = (k + ahead + 1u) << 6;
                                    asm volatile("s_load_dwordx16 %0, %1, %2" : "=&s"(s) : "s"(crefs), "s"(ro));
                                    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(s));
                                    test_rec(vf4{s[0], s[1], s[2], s[3]}, vf4{s[4], s[5], s[6], s[7]},
                                             vf4{s[8], s[9], s[10], s[11]}, vf4{s[12], s[13], s[14], s[15]},
                                             [&] { return k + ahead + 1u; });
                                }
                            }
                        };
                        asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=&s"(a) : "s"(gp));
                        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a));
                        if (k != kend)
                            do
                            {
                                asm volatile("s_load_dwordx16 %0, %1, 0x40" : "=&s"(b) : "s"(gp));
                                gate_pair(a, 0u, true);
                                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b));
                                asm volatile("s_load_dwordx16 %0, %1, 0x80" : "=&s"(a) : "s"(gp));
                                gate_pair(b, 2u, true);
                                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a));
                                gp += 8;
                                k += 4u;
                                asm volatile("" : "+s"(gp), "+s"(k));   // two counters: neither derived from the other
                            } while (k != kend);
                        const uint32_t rem = n & 3u;
                        if (rem != 0u)
                        {
                            asm volatile("s_load_dwordx16 %0, %1, 0x40" : "=&s"(b) : "s"(gp));
                            gate_pair(a, 0u, rem >= 2u);
                            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b));
                            if (rem == 3u) gate_pair(b, 2u, false);
                        }
                    }
                    else
                    {
                    cvf4 *const endp = np + size_t(n >> 1) * 8u;
                    asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=&s"(a) : "s"(np));
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a));
                    if (np != endp)
                        do
                        {
                            asm volatile("s_load_dwordx16 %0, %1, 0x40" : "=&s"(b) : "s"(np));
                            test_rec(vf4{a[0], a[1], a[2], a[3]}, vf4{a[4], a[5], a[6], a[7]},
                                     vf4{a[8], a[9], a[10], a[11]}, vf4{a[12], a[13], a[14], a[15]},
                                     [&] { return rec_k(np, 0u); });
                            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b));
                            asm volatile("s_load_dwordx16 %0, %1, 0x80" : "=&s"(a) : "s"(np));
                            test_rec(vf4{b[0], b[1], b[2], b[3]}, vf4{b[4], b[5], b[6], b[7]},
                                     vf4{b[8], b[9], b[10], b[11]}, vf4{b[12], b[13], b[14], b[15]},
                                     [&] { return rec_k(np, 1u); });
                            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a));
                            np += 8;
                            asm volatile("" : "+s"(np));    // the pointer itself is the loop counter
                        } while (np != endp);
                    if (n & 1u)
                        test_rec(vf4{a[0], a[1], a[2], a[3]}, vf4{a[4], a[5], a[6], a[7]},
                                 vf4{a[8], a[9], a[10], a[11]}, vf4{a[12], a[13], a[14], a[15]},
                                 [&] { return rec_k(np, 0u); });
                    }
                }
                else
                {
                vf4 a0 = np[0], a1 = np[1], a2 = np[2], a3 = np[3];
                for (uint32_t k = kfirst;; k += 2u * kstep)
                {
                    vf4 b0, b1, b2, b3;
                    const bool more1 = k + kstep < ke0;
                    if (more1)
                    {
                        np = crefs + size_t(k + kstep) * 4u;
                        b0 = np[0];
                        b1 = np[1];
                        b2 = np[2];
                        b3 = np[3];
                    }
                    test_rec(a0, a1, a2, a3, [&] { return k; });
                    if (!more1) break;
                    const bool more2 = k + 2u * kstep < ke0;
                    if (more2)
                    {
                        np = crefs + size_t(k + 2u * kstep) * 4u;
                        a0 = np[0];
                        a1 = np[1];
                        a2 = np[2];
                        a3 = np[3];
                    }
                    test_rec(b0, b1, b2, b3, [&] { return k + kstep; });
                    if (!more2) break;
                }
                }
            }
            uniform_done = true;
        }
    }
    if constexpr (PRE)
    {
        if (!uniform_done) lane_list<STATS, VAR>(P, ra, rc, kb, ke, tb, u, v, tri, tests, first, step);
    }
    else if constexpr (ANY)
    {
        // The list in order, as below, until this lane's first test that counts: hit, cur_t < nct_ax,
        // tmin < cur_t and cur_t < tmax, all strict (tb = min(tmax, nct_ax): neither is NaN here -- the kernel
        // walks no ray whose bounds are -- and a NaN nct_ax makes tb NaN, which counts nothing, as the
        // reference's own compare against it).  A lane that found one leaves the loop; the others go on, and
        // the det / u vote inside the test is exact for whichever lanes still take part.
        // (the lane leaves through the loop's own bound, so the loop keeps its single exit: a second one in the
        // middle is carried as a lane mask)
        bool counted = false;
        for (uint32_t k = kb; k < ke; k++)
        {
            const float4 *rp = P.refs + size_t(k) * 3;
            const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
            float ct = 0.0f, cu, cv;
            const bool hit = rtd::ray_tri_mt_gated<F>(ox, oy, oz, dx, dy, dz, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z,
                                                      r1.w, r2.x, ct, cu, cv);
            counted = hit & (ct < tb) & (tmin < ct);
            ke = counted ? 0u : ke;
        }
        return counted;
    }
    else if constexpr (CROSS)
    {
        // The whole list in order: hit, t_in <= cur_t (the one inclusive bound), cur_t < nct_ax, tmin < cur_t and
        // cur_t < tmax (tb as above; a NaN t_in or nct_ax counts nothing, as the compare itself).  det is the
        // test's own (triangle.h:48), read only where the test counted.
        for (uint32_t k = kb; k < ke; k++)
        {
            const float4 *rp = P.refs + size_t(k) * 3;
            const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
            float ct = 0.0f, cu, cv, det;
            const bool hit = rtd::ray_tri_mt_gated_det<F>(ox, oy, oz, dx, dy, dz, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y,
                                                          r1.z, r1.w, r2.x, ct, cu, cv, det);
            const bool counted = hit & (t_in <= ct) & (ct < tb) & (tmin < ct);
            tri += counted ? 1u : 0u;
            tests += (counted & (det > 0.0f)) ? 1u : 0u;
        }
        return false;
    }
    else
    for (uint32_t k = kb; k < ke; k++)
    {
        if (STATS) tests++;
        const float4 *rp = P.refs + size_t(k) * 3;          // one address, immediate offsets
        const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
        float ct, cu, cv;
        bool hit;
        const uint32_t id = __float_as_uint(r2.y);
        if (TRI == RT_TRI_BARYCENTRIC)
        {
            const float4 fn = P.face_n[id];
            hit = rtd::ray_tri_bary_pred(ox, oy, oz, dx, dy, dz, r0.x, r0.y, r0.z, r0.w, r1.x,
                                         r1.y, r1.z, r1.w, r2.x, fn.x, fn.y, fn.z, ct, cu, cv);
        }
        else if (VAR & kVarWaveGate)
            // (kVarRays: per-lane origins, so the 48-byte records and the whole test per ray; the vote
            // is exact for any set of lanes)
            hit = rtd::ray_tri_mt_gated<F && (VAR & kVarRays) != 0>(ox, oy, oz, dx, dy, dz, r0.x, r0.y, r0.z, r0.w, r1.x,
                                                                    r1.y, r1.z, r1.w, r2.x, ct, cu, cv);
        else
            hit = rtd::ray_tri_mt_pred(ox, oy, oz, dx, dy, dz, r0.x, r0.y, r0.z, r0.w, r1.x,
                                       r1.y, r1.z, r1.w, r2.x, ct, cu, cv);
        const bool take = hit & (ct < tb);                     // grid.cpp:258-260
        tb = take ? ct : tb;
        u = take ? cu : u;
        v = take ? cv : v;
        tri = take ? id : tri;
    }
    if constexpr (SPLIT)
    {
        if (split)
        {
            // the four waves' first minima of this cell -> the list's (kLdsSplit: see above)
            const uint32_t base = lpar * (kWavesPerWG * 64u), lane = threadIdx.x & 63u;
            float2 *tk = lds_red_tk() + base, *uv = lds_red_uv() + base;
            tk[threadIdx.x] = make_float2(tb, __uint_as_float(tb < tb0 ? tri : 0xFFFFFFFFu));
            uv[threadIdx.x] = make_float2(u, v);
            lds_barrier();
            float bt = tb0;
            uint32_t bk = 0xFFFFFFFFu, bj = 0u;
#pragma unroll
            for (uint32_t j = 0; j < kWavesPerWG; j++)
            {
                const float2 o = tk[j * 64u + lane];
                const uint32_t ok = __float_as_uint(o.y);
                const bool better = (o.x < bt) | ((o.x == bt) & (ok < bk));
                bt = better ? o.x : bt;
                bk = better ? ok : bk;
                bj = better ? j : bj;
            }
            lpar ^= 1u;
            if (bk != 0xFFFFFFFFu)
            {
                const float2 w = uv[bj * 64u + lane];
                tb = bt;
                u = w.x;
                v = w.y;
                tri = bk;
            }
        }
    }
    t = tb < tb0 ? tb : t;
    return t != rtd::kFltMax;                                  // grid.cpp:270-271
}

// One DDA advance over plain local variables (grid.cpp:236-239 + 274-277), exact because
// untouched axes keep their values.  A macro, not a member function or a capturing lambda:
// selecting between struct fields through `this`/references becomes a pointer select, which
// defeats SROA and put the walk state in LDS/scratch (measured).
// Step axis of grid.cpp:236-239 restated: with m = min(nct), the nested strict '<' chain picks
// the HIGHEST axis index among those equal to m (all 7 tie patterns checked), so
// a2 = nct2 == m, a1 = !a2 && nct1 == m, else a0.  nct is never NaN (finite setup, FLT_MAX for
// zero components).  Each crossing time advances as nct_a + (a ? dt_a : 0.0f): the step axis
// gets the reference's single IEEE add (grid.cpp:277), and x + 0.0f == x for every value nct
// takes (finite or +inf, never -0 or NaN: every setup term is >= 0, see dda_setup).  The state
// updates run unconditionally -- when MORE is false the caller breaks and the state is dead --
// so the step has no divergent branch.  Sets NCT_AX to the step axis' crossing t and MORE to
// false when the ray leaves the grid (grid.cpp:275-276).
// (RT_DDA_AXIS_: the step axis, written once for the four steps below; each expands it in place, so the tokens
// the compiler sees are those of the written-out form)
#define RT_DDA_AXIS_                                                                           \
        const float m_ = __builtin_fminf(__builtin_fminf(nct0, nct1), nct2);                   \
        const bool a2_ = nct2 == m_;                                                           \
        const bool a1_ = !a2_ && nct1 == m_;                                                   \
        const bool a0_ = !a2_ && !a1_
#define RT_DDA_ADVANCE_ADD(NCT_AX, MORE)                                                       \
    do {                                                                                       \
        RT_DDA_AXIS_;                                                                          \
        NCT_AX = m_;                                                                           \
        MORE = (a2_ ? rem2 : (a1_ ? rem1 : rem0)) != 0;                                        \
        nct0 += a0_ ? dt0 : 0.0f;                                                              \
        nct1 += a1_ ? dt1 : 0.0f;                                                              \
        nct2 += a2_ ? dt2 : 0.0f;                                                              \
        rem0 -= int(a0_); rem1 -= int(a1_); rem2 -= int(a2_);                                  \
        cell += a2_ ? cs2 : (a1_ ? cs1 : cs0);                                                 \
    } while (0)

// RT_DDA_ADVANCE_ADD with the three remaining-cell counts packed into one word: rem0 in bits
// 0-9, rem1 in 11-20, rem2 in 22-30, guard bits 10, 21, 31 (needs dims <= 512; rt_scene::
// pack_ok).  The step subtracts the axis unit unconditionally; a count that was 0 borrows into
// its guard bit, so MORE = no guard bit set == (rem of the step axis != 0) -- the walk exits
// exactly where RT_DDA_ADVANCE_ADD's does (the borrowed state is dead after the exit).
constexpr int kRemGuards = int((1u << 10) | (1u << 21) | (1u << 31));
#define RT_DDA_ADVANCE_PACKED(NCT_AX, MORE)                                                    \
    do {                                                                                       \
        RT_DDA_AXIS_;                                                                          \
        NCT_AX = m_;                                                                           \
        remp -= a2_ ? (1 << 22) : (a1_ ? (1 << 11) : 1);                                       \
        MORE = (remp & kRemGuards) == 0;                                                       \
        nct0 += a0_ ? dt0 : 0.0f;                                                              \
        nct1 += a1_ ? dt1 : 0.0f;                                                              \
        nct2 += a2_ ? dt2 : 0.0f;                                                              \
        cell += a2_ ? cs2 : (a1_ ? cs1 : cs0);                                                 \
    } while (0)

// RT_DDA_ADVANCE_PACKED without the exit test: a step inside a proven-empty run (the
// empty-run blocks of grid_intersect read MORE from the packed word after the block).
#define RT_DDA_BARE_STEP()                                                                     \
    do {                                                                                       \
        RT_DDA_AXIS_;                                                                          \
        remp -= a2_ ? (1 << 22) : (a1_ ? (1 << 11) : 1);                                       \
        nct0 += a0_ ? dt0 : 0.0f;                                                              \
        nct1 += a1_ ? dt1 : 0.0f;                                                              \
        nct2 += a2_ ? dt2 : 0.0f;                                                              \
        cell += a2_ ? cs2 : (a1_ ? cs1 : cs0);                                                 \
    } while (0)


// The box-run walk's step: RT_DDA_ADVANCE_PACKED, with the step axis' unit also taken from the
// box counts (boxw, build_box_words' empty-cell layout = the packed counts' layout): a count
// that was 0 borrows into its guard bit when the step leaves the box.
#define RT_DDA_ADVANCE_BOX(NCT_AX, MORE)                                                       \
    do {                                                                                       \
        RT_DDA_AXIS_;                                                                          \
        NCT_AX = m_;                                                                           \
        const int u_ = a2_ ? (1 << 22) : (a1_ ? (1 << 11) : 1);                                \
        remp -= u_;                                                                            \
        boxw -= u_;                                                                            \
        MORE = (remp & kRemGuards) == 0;                                                       \
        nct0 += a0_ ? dt0 : 0.0f;                                                              \
        nct1 += a1_ ? dt1 : 0.0f;                                                              \
        nct2 += a2_ ? dt2 : 0.0f;                                                              \
        cell += a2_ ? cs2 : (a1_ ? cs1 : cs0);                                                 \
    } while (0)
// A step inside a box run: only the crossing times and the box counts move; the run's end
// rebuilds the cell index and the remaining-cell counts from the box counts' difference.
// (RT_DDA_BOX_AXIS_, RT_DDA_BOX_MOVE_: its axis choice and its move, written once for the two forms)
#define RT_DDA_BOX_AXIS_                                                                       \
        const float m_ = __builtin_fminf(__builtin_fminf(nct0, nct1), nct2);                   \
        const bool a2_ = nct2 == m_;                                                           \
        const bool e1_ = nct1 == m_
#define RT_DDA_BOX_MOVE_                                                                       \
        boxw -= a2_ ? (1 << 22) : (e1_ ? (1 << 11) : 1);                                       \
        nct0 += (a2_ | e1_) ? 0.0f : dt0;                                                      \
        nct1 += (e1_ & !a2_) ? dt1 : 0.0f;                                                     \
        nct2 += a2_ ? dt2 : 0.0f
#define RT_DDA_BOX_BARE_STEP()                                                                 \
    do {                                                                                       \
        RT_DDA_BOX_AXIS_;                                                                      \
        RT_DDA_BOX_MOVE_;                                                                      \
    } while (0)
// RT_DDA_BOX_BARE_STEP that also hands out the crossing it takes (kVarAnyHit: the last one of a run is the
// run's largest, which decides whether the walk has passed tmax).
#define RT_DDA_BOX_BARE_STEP_T(NCT_AX)                                                         \
    do {                                                                                       \
        RT_DDA_BOX_AXIS_;                                                                      \
        NCT_AX = m_;                                                                           \
        RT_DDA_BOX_MOVE_;                                                                      \
    } while (0)
constexpr int kBoxUnits3 = 3 | (3 << 11) | (3 << 22);   // 3 in every box-count field

// A lower bound of x(f) = the add chain x, fl(x + dt), ... after f steps (a box run's exit crossing
// along one axis; grid_intersect's per-lane runs).  Only compared against crossing times, never part
// of a pixel's arithmetic: its two explicit FMAs (the fused f dt + x, and the margin) are the
// only ones outside rtd::rcp_nr (tests/test_build_guard.py).  A still axis (x = FLT_MAX, dt = 0)
// gives ~FLT_MAX.
__device__ __forceinline__ float box_exit_bound(float x, float dtv, int f)
{
    const float e = __builtin_fmaf(float(f), dtv, x), k = float(f + 2) * 0x1p-23f;
    return e - __builtin_fmaf(__builtin_fabsf(x), k, __builtin_fabsf(e) * k);
}

// Grid entry + per-axis DDA setup of Grid::Intersect (aabb.h:9-83, grid.h:44-51,
// grid.cpp:174-216), axis arrays unrolled into scalars.  Instead of pos/step/out per axis the
// walk keeps the cells left before 'pos == out' (rem) and the signed GridIdx stride of a step
// (cs): grid.cpp:274-277 exits after the same steps.  False when the ray misses the grid.
// RCP_SETUP false: the division form -- ray_aabb's own reciprocals and six divisions -- for the one walk whose
// kernel the reciprocal form costs a wave per SIMD (grid_intersect says which).
#ifndef RT_SETUP_RCP            // (tools/build_variant.sh -DRT_SETUP_RCP=0: the A/B arm with the six divisions)
#define RT_SETUP_RCP 1
#endif
template <bool RCP_SETUP = (RT_SETUP_RCP != 0)>
__device__ __forceinline__ bool dda_setup(const KParams& P, float ox, float oy, float oz, float dx, float dy, float dz,
                                          float& nct0, float& nct1, float& nct2, float& dt0, float& dt1, float& dt2,
                                          int& rem0, int& rem1, int& rem2, int& cs0, int& cs1, int& cs2, int& cell,
                                          float *enter_out = nullptr)
{
    // One reciprocal per axis serves ray_aabb's slabs AND the six quotients below (rt_setup_div.h).
    // ix = 1.0f / dx in every lane: rtd::rcp_nr where the whole wave's d lie in the quotients' window
    // (inside rcp_nr's proven range), else -- a zero, tiny, huge or NaN component in some lane; rare --
    // the wave divides, as rtd::rcp_exact does.  `bad`: lanes that fail the window so far (wave-uniform).
    float ix = 0.0f, iy = 0.0f, iz = 0.0f;
    unsigned long long bad = ~0ull;
    if constexpr (RCP_SETUP)
    {
        ix = rtd::rcp_nr(dx);
        iy = rtd::rcp_nr(dy);
        iz = rtd::rcp_nr(dz);
        bad = setup_div_bad_lanes(dx) | setup_div_bad_lanes(dy) | setup_div_bad_lanes(dz);
        if (bad != 0ull)
        {
            ix = 1.0f / dx;
            iy = 1.0f / dy;
            iz = 1.0f / dz;
        }
    }
    float enter_t, leave_t, gx, gy, gz;
    if (rtd::point_in_aabb(ox, oy, oz, P.bmin, P.bmax))
    {
        enter_t = 0.0f;
        gx = ox; gy = oy; gz = oz;
    }
    else if (RCP_SETUP ? rtd::ray_aabb_rcp(ox, oy, oz, ix, iy, iz, P.bmin, P.bmax, enter_t, leave_t)
                       : rtd::ray_aabb(ox, oy, oz, dx, dy, dz, P.bmin, P.bmax, enter_t, leave_t))
    {
        gx = ox + dx * enter_t;
        gy = oy + dy * enter_t;
        gz = oz + dz * enter_t;
    }
    else
        return false;

    // grid.h:44-48 ToVoxel, grid.h:50-51 ToPos, grid.cpp:190-216 per-axis setup
    auto to_voxel = [&](float g, int a) {
        const int vx = rtd::cvt_i32_x86((g - P.bmin[a]) * P.icw);
        const int hi = P.dim[a] - 1;
        return vx < 0 ? 0 : (vx > hi ? hi : vx);
    };
    const int pos0 = to_voxel(gx, 0), pos1 = to_voxel(gy, 1), pos2 = to_voxel(gz, 2);
    dt0 = dt1 = dt2 = 0.0f;
    rem0 = rem1 = rem2 = cs0 = cs1 = cs2 = 0;
    // The two numerators of an axis: the distance to the first cell face along d ((bmin + float(pos + 1) cw)
    // - g for d > 0, (bmin + float(pos) cw) - g otherwise) and +-cw; both are divided by d.
    auto face = [&](float d, float g, int pos, int a) { return (P.bmin[a] + float(d > 0.0f ? pos + 1 : pos) * P.cw) - g; };
    const float n0 = face(dx, gx, pos0, 0), n1 = face(dy, gy, pos1, 1), n2 = face(dz, gz, pos2, 2);
    const float c0 = dx > 0.0f ? P.cw : -P.cw, c1 = dy > 0.0f ? P.cw : -P.cw, c2 = dz > 0.0f ? P.cw : -P.cw;
    // The six quotients: n / d's bits from the axis' reciprocal (setup_div, 5 instructions against the
    // division's 11) when every lane's n and d and the cell width lie in its window, else by division.
    const uint32_t cwb = __float_as_uint(P.cw) & 0x7FFFFFFFu;   // (positive floats order as their bits)
    if constexpr (RCP_SETUP) bad |= setup_div_bad_lanes(n0) | setup_div_bad_lanes(n1) | setup_div_bad_lanes(n2);
    float q0, q1, q2, w0, w1, w2;
    if (RCP_SETUP && bad == 0ull && cwb >= __float_as_uint(kSetupDivLo) && cwb <= __float_as_uint(kSetupDivHi))
    {
        q0 = setup_div(n0, dx, ix); w0 = setup_div(c0, dx, ix);
        q1 = setup_div(n1, dy, iy); w1 = setup_div(c1, dy, iy);
        q2 = setup_div(n2, dz, iz); w2 = setup_div(c2, dz, iz);
    }
    else
    {
        q0 = n0 / dx; w0 = c0 / dx;
        q1 = n1 / dy; w1 = c1 / dy;
        q2 = n2 / dz; w2 = c2 / dz;
    }
    auto setup = [&](float d, float q, float w, int pos, int a, int stride, float& nct, float& dtv, int& rem, int& cs) {
        if (d == 0.0f)
            nct = rtd::kFltMax;
        else if (d > 0.0f)
        {
            nct = enter_t + q;
            dtv = w;
            rem = P.dim[a] - 1 - pos;           // steps until pos + 1 == dim
            cs = stride;
        }
        else
        {
            nct = enter_t + q;
            dtv = w;
            rem = pos;                          // steps until pos - 1 == -1
            cs = -stride;
        }
    };
    setup(dx, q0, w0, pos0, 0, 1, nct0, dt0, rem0, cs0);
    setup(dy, q1, w1, pos1, 1, P.dxdz, nct1, dt1, rem1, cs1);
    setup(dz, q2, w2, pos2, 2, P.dim[0], nct2, dt2, rem2, cs2);
    cell = pos0 + pos2 * P.dim[0] + pos1 * P.dxdz;
    if (enter_out) *enter_out = enter_t;
    return true;
}

// Offset of the ray's octant copy in P.cellwo (0 when there is one copy).  An axis with d == 0
// never steps, so either sign is right for it (-0.0 counts as +).
__device__ __forceinline__ int oct_offset(const KParams& P, float dx, float dy, float dz)
{
    const uint32_t o = uint32_t(dx < 0.0f) | (uint32_t(dy < 0.0f) << 1) | (uint32_t(dz < 0.0f) << 2);
    return int(o * P.oct_stride);
}

// Offset of the ray's box-run copy in P.cellwb: octant (as oct_offset) x 3 + major axis (the
// largest |d| component; any choice is exact, the copy only shapes the boxes for speed).
__device__ __forceinline__ int box_offset(const KParams& P, float dx, float dy, float dz)
{
    const uint32_t o = uint32_t(dx < 0.0f) | (uint32_t(dy < 0.0f) << 1) | (uint32_t(dz < 0.0f) << 2);
    const float ax = __builtin_fabsf(dx), ay = __builtin_fabsf(dy), az = __builtin_fabsf(dz);
    const uint32_t m = (ax >= ay && ax >= az) ? 0u : (ay >= az ? 1u : 2u);
    return int((o * 3u + m) * P.box_stride);
}

// Records of the product walks (rt_render_records_device): the GridIdx of the last cell walked on a
// miss, from the state the walk ends in.  The exit step along axis a borrowed into the guard bit of
// a's packed remaining-cell count -- the LOWEST set guard, since a borrow only carries upward -- and
// `cell` already includes that step.  The walk itself is unchanged: this runs after it, and only a
// record store reads the result.
constexpr uint32_t kVoxelUnknown = 0xFFFFFFFEu;     // not recoverable from this walk's end state
__device__ __forceinline__ uint32_t exit_voxel(int remp, int cell, int cs0, int cs1, int cs2)
{
    const uint32_t g = uint32_t(remp) & uint32_t(kRemGuards);
    return uint32_t(cell - ((g & (1u << 10)) ? cs0 : ((g & (1u << 21)) ? cs1 : cs2)));
}

// grid.cpp:159-281 Grid::Intersect (NEW_GRID_TRAVERSAL), axis arrays unrolled into scalars
// so nothing is runtime-indexed (no scratch).  Counters are compiled in only for records.
template <bool STATS, int TRI, int VAR>
__device__ __forceinline__ bool grid_intersect(const KParams& P, float ox, float oy, float oz,
                                               float dx, float dy, float dz,
                                               float& t, float& u, float& v, uint32_t& tri,
                                               uint32_t& voxel, uint32_t& steps, uint32_t& tests, float tmin = 0.0f)
{
    // kVarAnyHit (rt_occluded_rays_device, include/rt_tracer.h): the same walk over (tmin, tmax), tmax passed
    // in t.  It returns true at the first test that counts (test_cell) and false at the first step whose
    // crossing time is >= tmax (`stop` below: one compare per step on the crossing the advance hands out; a NaN
    // crossing stops nothing).  Both exits only end the walk sooner, and nothing is indexed by tmin or tmax:
    // the arguments on termination and on `cell` below hold unchanged.  t, u, v, tri, voxel are not written.
    constexpr bool ANY = (VAR & kVarAnyHit) != 0;
    // kVarCross (rt_crossing_rays_device): the any-hit walk's interval and step rule, but a counted test ends
    // nothing, and each looked-up cell is tested against its own interval [t_in, exit crossing): t_in is the
    // crossing of the last step taken before the cell (-inf before the first), which every arm below hands on --
    // the plain arms from the advance of the iteration before, the box runs from the run's last bare step.  The
    // crossings a walk takes never decrease, so the intervals are disjoint and a (ray, triangle) pair listed in
    // several cells counts in at most one.  The counts leave in tri (count) and tests (front), which enter as 0;
    // the return value is false and t, u, v are not written.
    constexpr bool CROSS = (VAR & kVarCross) != 0;
    constexpr bool IVAL = ANY || CROSS;                 // the walks over (tmin, tmax)
    float tmax = 0.0f;
    if constexpr (IVAL) tmax = t;
    bool found = false;                 // kVarAnyHit: the walk's result
    float t_in = -__builtin_inff();     // kVarCross: the crossing into the cell about to be tested
    (void)tmax;
    (void)found;
    (void)t_in;
    float nct0, nct1, nct2, dt0, dt1, dt2;
    int rem0, rem1, rem2, cs0, cs1, cs2, cell;
    // (the ray-query walk with the Newton 1/det but without packed counts: its kernel stands at 63 VGPRs and
    // went to 72 -- a wave per SIMD -- with the reciprocal form of the setup's quotients in this walk, its
    // common one, so this instantiation keeps the divisions.  The same kernel's rare branch for long
    // directions, rt_rays.hip's walk without kVarFastRcp, is another instantiation and takes the reciprocal
    // form; both forms give n / d's bits)
    constexpr bool RCP_SETUP = RT_SETUP_RCP != 0 &&
                               ((VAR & kVarRays) == 0 || (VAR & kVarPackedRem) != 0 || (VAR & kVarFastRcp) == 0);
    if (!dda_setup<RCP_SETUP>(P, ox, oy, oz, dx, dy, dz, nct0, nct1, nct2, dt0, dt1, dt2, rem0, rem1, rem2, cs0, cs1,
                              cs2, cell))
        return false;
    if constexpr (!IVAL) t = rtd::kFltMax;
    uint32_t lpar = 0u;                 // kVarLdsSplit: the reduction buffers' parity (test_cell)

    if constexpr ((VAR & kVarSkipRun) != 0 && (VAR & kVarPackedRem) != 0)
    {
        // Box runs (AUTO; build_box_words): a looked-up empty cell hands the lane an empty box
        // (its corner at the cell, extending along the ray's octant) as per-axis step counts in
        // the packed counts' layout.  Every step takes its axis unit from both words; while no
        // box count has borrowed, the lane is inside the box and its cell is empty: no lookup,
        // no test.  A non-empty cell's word leaves boxw = 0, so the next step borrows and looks
        // the next cell up.  Same cells in the same order, same tests: only lookups of
        // proven-empty cells are skipped.  Termination as below: every iteration that does not
        // exit decrements a positive remaining-cell count.
        // Two phases (profiles/r04g_ab_box_run_modes.json): the APPROACH, through
        // the empty space before the wave's first contact, runs per lane (each lane jumps to just
        // before its own box exit by per-axis add chains, then waits at its first non-empty cell);
        // from the moment every active lane is at its own non-empty cell the wave walks in
        // LOCK-STEP, with wave-uniform bare steps while every lane is inside its box, so rays of a
        // wave that cross the same cells test them together (wave-uniform lists).
        static_assert(!STATS, "the records kernel walks the distance words, not the box runs");
        int remp = rem0 | (rem1 << 11) | (rem2 << 22);
        int boxw = kRemGuards;                              // no box yet: look the first cell up
        const int coff = box_offset(P, dx, dy, dz);
        cell += coff;
        bool sync = false;                                  // wave-uniform: the lock-step phase
        for (;;)
        {
            uint32_t kb = 0, ke = 0;
            float nct_ax;
            bool more;
            if ((boxw & kRemGuards) != 0)
            {
                const uint32_t w = P.cellwb[uint32_t(cell)];
                const uint32_t ne = uint32_t(int(w) >> 31);           // all ones: a non-empty cell
                kb = (w >> 11) & 0xFFFFFu;
                ke = kb + (w & ne & 2047u);
                boxw = int(w & ~ne);
            }
            // kVarRays (rt_rays.hip: a caller's rays, which need not share cells): the lane stays in the
            // per-lane phase for the whole walk -- it never waits at its first non-empty cell (a parked lane
            // would idle behind 63 unrelated walks) and never enters lock-step; `sync` stays false.
            // No input can hang or misdirect this loop: `cell` is dda_setup's clamped start cell plus the
            // ray's copy offset (box_offset: octant < 8, major axis < 3) plus steps, and every step along
            // axis a takes a unit from that axis' remaining-cell count in remp, which started at the cells
            // left to the grid's face and ends the walk when it borrows -- so `cell` never leaves the ray's
            // copy of the grid, whatever the crossing times hold (NaN and inf included: they only choose
            // WHICH axis steps).  A per-lane run moves at most the box's own counts (each add chain is
            // bounded by its field, the bare steps by the borrow), and a box is clipped to the grid.  Every
            // record index [kb, ke) comes from a cell word.  Nothing is indexed by a value of the ray.
            if constexpr ((VAR & kVarRays) == 0)
            if (!sync)
            {
                // Approach: a lane at its first non-empty cell waits there (no step, no test; the
                // cell is looked up again) until every active lane of the wave is at its own.
                // Waiting changes no lane's walk, only when it is taken.
                if (wave_all(kb < ke))
                    sync = true;
                else if (kb < ke)
                {
                    boxw = kRemGuards;
                    continue;
                }
            }
            RT_DDA_ADVANCE_BOX(nct_ax, more);
            bool hit = false;
            if (kb < ke) hit = test_cell<STATS, TRI, VAR>(P, ox, oy, oz, dx, dy, dz, kb, ke, nct_ax, t, u, v, tri, tests, lpar, tmin, t_in);
            // kVarAnyHit: the step just taken -- out of a looked-up cell -- crossed at nct_ax; a lane that stops
            // here takes no run (its box counts are dead: a set guard keeps it out)
            [[maybe_unused]] bool stop = false;
            if constexpr (IVAL)
            {
                found = hit;
                stop = nct_ax >= tmax;
                boxw = stop ? kRemGuards : boxw;
                t_in = nct_ax;          // kVarCross: the next looked-up cell's entry, unless a run steps on
            }
            const bool inside = (uint32_t(boxw) & uint32_t(kRemGuards)) == 0u;
            if (!sync && inside)
            {
                // Per-lane box run.  Inside a box the three crossing-time sequences are independent
                // add chains x_a(k+1) = fl(x_a(k) + dt_a), and the box is left at the first of the
                // (f_a + 1)-th crossings E_a = x_a(f_a) (f_a = the box field).  tl is a lower bound
                // of every E_a: f dt + x fused (one rounding) is within 2^-24 |.| of it, the chain
                // within f 2^-24 max|x_k| <= f 2^-24 (|x| + |E|) of it, so
                // E_a >= e_a - (f_a + 2) 2^-23 (|e_a| + |x_a|) with room for the bound's own
                // roundings.  Each axis then takes its crossings below tl (at most f_a of them):
                // every taken crossing is < tl <= every untaken one, so these are exactly the
                // walk's next sum c_a steps, in some order, all inside the box (empty cells, no
                // test, no exit).  Bare steps then run to the box's exit (normally one) -- the
                // same cells, crossing times and exits as one step per cell.
                const uint32_t b0 = uint32_t(boxw);
                const int f0 = boxw & 1023, f1 = (boxw >> 11) & 1023, f2 = int(uint32_t(boxw) >> 22);
                // (rt_lane_run.h: tl, the three chains -- wave-uniform trips where the bounds prove the
                // count guard redundant, else the guarded loops -- and the packed step counts)
                boxw -= lane_run<RT_WALK_LEAN_CHAINS>(nct0, nct1, nct2, dt0, dt1, dt2, box_exit_bound(nct0, dt0, f0),
                                                      box_exit_bound(nct1, dt1, f1), box_exit_bound(nct2, dt2, f2), f0,
                                                      f1, f2);
                if constexpr (IVAL)
                {
                    // Rule 3 of the any-hit walk asks after EVERY step whether its crossing was >= tmax; inside
                    // an empty box nothing is tested, so only the cell the run arrives at needs the answer: was
                    // any crossing of the run >= tmax.  The crossings a walk takes never decrease (each is the
                    // minimum of three add chains with dt >= 0), the add chains above take only crossings below
                    // tl, and every bare step's crossing is an untaken one, >= tl: the LAST bare step's
                    // crossing is the run's largest, and it alone is compared.
                    // kVarCross: the same value is the crossing into the cell the run arrives at -- the last
                    // step taken before it -- and so that cell's t_in.  (It is a term of an add chain, not
                    // recoverable from the state after the step as nct - dt.)
                    float last;
                    do
                        RT_DDA_BOX_BARE_STEP_T(last);
                    while ((uint32_t(boxw) & uint32_t(kRemGuards)) == 0u);
                    stop = last >= tmax;
                    t_in = last;
                }
                else
                do
                    RT_DDA_BOX_BARE_STEP();
                while ((uint32_t(boxw) & uint32_t(kRemGuards)) == 0u);
                const uint32_t d = b0 - uint32_t(boxw);
                remp = int(uint32_t(remp) - d);           // wrapping (d may reach 2^31)
                cell += int(d & 2047u) * cs0 + int((d >> 11) & 2047u) * cs1 + int(d >> 22) * cs2;
                more = (remp & kRemGuards) == 0;
            }
            else if (sync && wave_all(inside))
            {
                // Wave-uniform runs while every active lane is inside its box (the boxes are
                // clipped to the grid, so inside the box is inside the grid): blocks of 4 bare
                // steps while every box count of every lane is >= 3 (the first three steps of a
                // block stay inside; the fourth may leave, which the next vote sees), then
                // single steps.  A bare step moves only the crossing times and boxw; the run's
                // end rebuilds the cell index and the remaining-cell counts from the box
                // counts' difference, which is sum n_a * unit_a over the run's n_a steps along
                // axis a (n_a <= 1024, 1024, 512: no field of the difference carries).  A lane
                // that hit holds boxw < 0 (guard set), so runs only start when no lane hit.
                // (if + do-while: a while loop's exit edge made the compiler copy the whole
                // walk state every iteration.)
                const uint32_t b0 = uint32_t(boxw);
                if (wave_all((uint32_t(boxw - kBoxUnits3) & uint32_t(kRemGuards)) == 0u))
                    do
                    {
                        RT_DDA_BOX_BARE_STEP();
                        RT_DDA_BOX_BARE_STEP();
                        RT_DDA_BOX_BARE_STEP();
                        RT_DDA_BOX_BARE_STEP();
                    } while (wave_all((uint32_t(boxw - kBoxUnits3) & uint32_t(kRemGuards)) == 0u));
                if (wave_all((uint32_t(boxw) & uint32_t(kRemGuards)) == 0u))
                    do
                        RT_DDA_BOX_BARE_STEP();
                    while (wave_all((uint32_t(boxw) & uint32_t(kRemGuards)) == 0u));
                const uint32_t d = b0 - uint32_t(boxw);
                remp = int(uint32_t(remp) - d);           // wrapping (d may reach 2^31)
                cell += int(d & 2047u) * cs0 + int((d >> 11) & 2047u) * cs1 + int(d >> 22) * cs2;
                more = (remp & kRemGuards) == 0;
            }
            if constexpr (IVAL) more &= !stop;
            if (hit | !more) break;
        }
        if constexpr (IVAL) return found;
        // records only: the exit cell in the ray's box-word copy (trace_sample removes the copy's
        // offset, so nothing extra is live across the walk)
        voxel = exit_voxel(remp, cell, cs0, cs1, cs2);
        return t != rtd::kFltMax;                            // t is only set by a hit
    }

    if (P.cellw && (VAR & kVarDistSkip))
    {
        // Distance skipping: after an empty cell at L-inf distance d from geometry the next
        // d-1 cells of the walk are provably empty, so they take the DDA step only.
        // Termination: every iteration that does not exit decrements a positive rem (the step
        // axis' count; MORE is false when it is 0), so a walk ends within rem0+rem1+rem2+1
        // iterations whatever nct holds.
        int skip = 0;
        int remp = rem0 | (rem1 << 11) | (rem2 << 22);      // kVarPackedRem only
        const int coff = oct_offset(P, dx, dy, dz);
        cell += coff;
        for (;;)
        {
            if (STATS) { voxel = uint32_t(cell - coff); steps++; }
            uint32_t kb = 0, ke = 0;
            float nct_ax;
            bool more;
            if (skip == 0)
            {
                const uint32_t w = P.cellwo[uint32_t(cell)];
                const uint32_t cnt = w & 2047u;
                kb = w >> 11;
                ke = kb + cnt;
                skip = cnt ? 0 : int(kb) - 1;
            }
            else
                skip--;
            if (VAR & kVarPackedRem)
                RT_DDA_ADVANCE_PACKED(nct_ax, more);
            else
                RT_DDA_ADVANCE_ADD(nct_ax, more);
            // one exit test per iteration (a hit, or the grid's end here or in the empty run
            // below), and the result read from t after the loop: the walk's loop-carried state
            // stays in VGPRs instead of per-exit lane masks (SALU per wave, PMC-measured)
            bool hit = false;
            if (kb < ke) hit = test_cell<STATS, TRI, VAR>(P, ox, oy, oz, dx, dy, dz, kb, ke, nct_ax, t, u, v, tri, tests, lpar, tmin, t_in);
            bool done = hit | !more;
            if constexpr (IVAL)
            {
                // (one cell per iteration here: every step's crossing is seen, and is the next cell's t_in.  The
                // wave-uniform empty run below belongs to the bits that took the box-run arm above: no interval
                // walk reaches it)
                found = hit;
                done |= nct_ax >= tmax;
                t_in = nct_ax;
            }
            if constexpr ((VAR & kVarSkipRun) != 0 && (VAR & kVarPackedRem) != 0 && !STATS)
            {
                // Wave-uniform empty run: while every active lane is inside a run of cells the
                // distance field proves empty, the wave takes bare DDA steps -- the same advances
                // and the same exits as one iteration per cell, with no cell word or test work.
                // Uniform, so no lane waits on another's run; the run ends when the first lane's
                // does.  (A lane inside a run has no hit and more == true, so done is false.)
                if (wave_all(skip > 0))
                {
                    // Blocks of 4, then 2, then 1 bare steps: one vote per block instead of one per
                    // step, and no exit test inside a block.  A lane that leaves the grid inside a
                    // block keeps stepping to the block's end, harmlessly: its state is dead (the
                    // walk ends with no further lookup), and the borrow into a guard bit is sticky
                    // for far more steps than a block holds (a field must count down 2^10 / 2^9
                    // more times to clear it), so MORE read after the block is the exit test.  The
                    // vote also requires every lane inside the grid: a lane with MORE false at the
                    // entry (it left the grid on an empty cell's step) takes no block.
                    auto run_ok = [&](int n) {    // (skip >= n) & more, as ONE integer compare
                        return wave_all(((uint32_t(remp) & uint32_t(kRemGuards)) | (uint32_t(skip - n) & 0x80000000u)) ==
                                        0u);
                    };
                    while (run_ok(4))
                    {
                        RT_DDA_BARE_STEP();
                        RT_DDA_BARE_STEP();
                        RT_DDA_BARE_STEP();
                        RT_DDA_BARE_STEP();
                        skip -= 4;
                    }
                    if (run_ok(2))
                    {
                        RT_DDA_BARE_STEP();
                        RT_DDA_BARE_STEP();
                        skip -= 2;
                    }
                    if (run_ok(1))
                    {
                        RT_DDA_BARE_STEP();
                        skip -= 1;
                    }
                    more = (remp & kRemGuards) == 0;
                    done = !more;
                }
            }
            if (done) break;
        }
        if constexpr (IVAL) return found;
        // a lane leaving the grid inside a block of bare steps stepped on: its last cell is lost
        if constexpr (!STATS)
        {
            if constexpr ((VAR & kVarSkipRun) != 0) voxel = kVoxelUnknown;
            else if constexpr ((VAR & kVarPackedRem) != 0) voxel = exit_voxel(remp, cell - coff, cs0, cs1, cs2);
            else voxel = uint32_t(cell - coff - (rem0 < 0 ? cs0 : (rem1 < 0 ? cs1 : cs2)));   // rem_a went to -1
        }
        return t != rtd::kFltMax;                            // t is only set by a hit
    }

    // One cell per iteration with its CSR range (the plain LANES arm, and scenes whose cell
    // lists do not fit the packed word).  max_steps = dims sum + 3 bounds it redundantly.
    for (uint32_t iter = 0; iter < P.max_steps; iter++)
    {
        if (STATS) { voxel = uint32_t(cell); steps++; }
        // Issue the CSR range loads first; the step's ALU work below overlaps their latency.
        uint32_t kb = 0, ke = 0;
        cell_range(P, uint32_t(cell), kb, ke);
        float nct_ax;
        bool more;
        RT_DDA_ADVANCE_ADD(nct_ax, more);
        if (kb < ke && test_cell<STATS, TRI, VAR>(P, ox, oy, oz, dx, dy, dz, kb, ke, nct_ax, t, u, v, tri, tests, lpar, tmin, t_in))
            return true;
        if (!more) break;
        if constexpr (IVAL)
        {
            if (nct_ax >= tmax) break;
            t_in = nct_ax;
        }
    }
    if constexpr (!STATS) voxel = uint32_t(cell - (rem0 < 0 ? cs0 : (rem1 < 0 ? cs1 : cs2)));   // records only
    return false;
}

} // namespace
} // namespace rtk
