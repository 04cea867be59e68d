// rt_wave.h -- wave, LDS and kernarg helpers under every device layer: votes, quad
// broadcasts, the LDS tier's buffers and barriers, wave-uniform loads, the kernel's own arguments re-read.
// Nothing here knows of the grid, a ray or a tile.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_kparams.h"

namespace rtk {
namespace {

// Morton decode of an 8-bit index inside a 16x16 tile: x = even bits, y = odd bits.
__device__ __forceinline__ uint32_t compact_bits(uint32_t v)
{
    v &= 0x55u;
    v = (v | (v >> 1)) & 0x33u;
    v = (v | (v >> 2)) & 0x0Fu;
    return v;
}

// Orders this wave's LDS writes before its later LDS reads of other lanes' data (a wave
// executes its LDS operations in order; this keeps the compiler from reordering them).
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Workgroup barrier for the LDS tier's reductions (kVarLdsSplit): this wave's LDS (and scalar)
// operations complete, then s_barrier.  The memory clobber keeps the compiler from moving LDS accesses
// across it (the s_barrier builtin alone is not a memory operation).
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// kVarLdsSplit: the per-lane (t, list position) and (u, v) of every wave of the workgroup,
// double-buffered by reduction parity: [parity][wave][lane] each
__device__ __forceinline__ float2 *lds_red_tk()
{
    __shared__ float2 r[2 * kWavesPerWG * 64];
    return r;
}
__device__ __forceinline__ float2 *lds_red_uv()
{
    __shared__ float2 r[2 * kWavesPerWG * 64];
    return r;
}

// kVarWaveClock debug counters of this wave: [0] records tested in wave-uniform loops,
// [1] iterations of the per-lane list loop
__device__ __forceinline__ uint32_t *wave_counters()
{
    __shared__ uint32_t c[kWavesPerWG * 2u];
    return c + (threadIdx.x >> 6) * 2u;
}

// Wave-uniform "every active lane": the predicate's lane mask against exec.  Pass a single
// compare: a predicate combined from several is materialised in a VGPR and compared back
// (2 VALU per vote, seen in the empty-run loop's ISA), where a compare's mask is the ballot.
__device__ __forceinline__ bool wave_all(bool p)
{
    return __builtin_amdgcn_ballot_w64(p) == __builtin_amdgcn_ballot_w64(true);
}

// v of lane (lane & ~3) + J: a DPP quad_perm broadcast within each quad of lanes (every lane of
// the quad must be active, as in process_item's resolve, where the whole wave is)
template <int J>
__device__ __forceinline__ float quad_bcast(float v)
{
    constexpr int ctrl = J | (J << 2) | (J << 4) | (J << 6);
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, false));
}
template <int J>
__device__ __forceinline__ uint32_t quad_bcast_u(uint32_t v)
{
    constexpr int ctrl = J | (J << 2) | (J << 4) | (J << 6);
    return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), ctrl, 0xF, 0xF, false));
}

__device__ __forceinline__ bool first_active_lane()
{
    return (threadIdx.x & 63u) == uint32_t(__ffsll((long long)__ballot(1)) - 1);
}

// The kernel's KParams re-read from the kernarg segment.  Parameters used only after the
// walk (output, shading, tile bookkeeping) are taken from here, so the compiler reloads them
// with s_load after the walk instead of holding ~30 SGPRs of them live across it (the render
// kernels' SGPR budget decides 8 vs 7 waves per SIMD).  The empty asm hides the pointer's
// origin (a register round trip), so these loads cannot be merged with the kernel entry's.
// off: byte offset of the frame's KParams in the kernarg segment (0 for the single-frame
// kernels, whose first argument is the KParams; a frame of KBatch in the batch kernel).
__device__ __forceinline__ const KParams& late_params(const KParams& P, uint32_t off = 0u)
{
    (void)P;
    const uint64_t a = uint64_t(__builtin_amdgcn_kernarg_segment_ptr()) + off;
    uint32_t lo = uint32_t(a), hi = uint32_t(a >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    return *(const KParams *)(const __attribute__((address_space(4))) KParams *)((uint64_t(hi) << 32) | lo);
}

// The batch kernels' KBatch, re-read from the kernarg segment (as late_params).
__device__ __forceinline__ const KBatch& late_batch()
{
    const uint64_t a = uint64_t(__builtin_amdgcn_kernarg_segment_ptr());
    uint32_t lo = uint32_t(a), hi = uint32_t(a >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    return *(const KBatch *)(const __attribute__((address_space(4))) KBatch *)((uint64_t(hi) << 32) | lo);
}

// Frame of launch block b (wave-uniform).
__device__ __forceinline__ uint32_t batch_frame(const KBatch& B, uint32_t b)
{
    uint32_t f = 0;
    for (uint32_t j = 1; j < kMaxBatch; j++) f += (j < B.nframes && b >= B.base[j]) ? 1u : 0u;
    return f;
}

// A wave-uniform word read through the scalar cache (words a kernel wrote and finished before this
// one was dispatched -- the plan's marks, the miss mask -- as the per-origin records of test_cell are read).
__device__ __forceinline__ uint32_t uniform_word(const uint32_t *p)
{
    return *(const __attribute__((address_space(4))) uint32_t *)(uint64_t(p));
}
// ... and a word that can always be read, for the loads of a group that have nothing to fetch: the kernel's arguments
__device__ __forceinline__ const uint32_t *spare_word()
{
    return (const uint32_t *)uint64_t(__builtin_amdgcn_kernarg_segment_ptr());
}

} // namespace
} // namespace rtk
