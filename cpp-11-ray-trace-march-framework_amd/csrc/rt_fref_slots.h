// rt_fref_slots.h -- which of a scene's two per-camera-origin record buffers (rt_scene::d_frefs) a frame
// reads, and when a buffer may be recomputed.  Host only, no HIP, C++11: rt_launch.hip
// runs these functions and tests/fref_slot_check.cpp checks the same ones exhaustively on the CPU.
#pragma once
#include <cstdint>
#include <cstring>

namespace rtk {

// ok: buffer b holds computed records; org: of which origin (bit patterns); last: bit b = the scene's
// last launch reads buffer b AND may still run beside the next one.  Only a launch that overlaps the
// last one (RT_KERNEL_FLAG_OVERLAP, order_overlap) finds bits set: a launch ordered after every earlier
// launch drops them first (fref_ordered).
struct FrefSlots
{
    bool ok[2] = { false, false };
    uint32_t org[2][3] = { { 0, 0, 0 }, { 0, 0, 0 } };
    uint32_t last = 0;
};

inline void fref_bits(const float org[3], uint32_t ob[3])
{
    std::memcpy(ob, org, 3 * sizeof(uint32_t));
}

// The buffer a frame of origin `ob` reads: the one holding that origin, else the one to compute it into
// -- never one of mask `busy` (bit b: buffer b), preferring an empty one.  -1: both are busy.
inline int fref_slot(const FrefSlots& f, const uint32_t ob[3], uint32_t busy, bool *compute)
{
    for (int b = 0; b < 2; b++)
        if (f.ok[b] && std::memcmp(ob, f.org[b], 3 * sizeof(uint32_t)) == 0)
        {
            *compute = false;
            return b;
        }
    *compute = true;
    for (int b = 0; b < 2; b++)
        if (!(busy & (1u << b)) && !f.ok[b]) return b;
    for (int b = 0; b < 2; b++)
        if (!(busy & (1u << b))) return b;
    return -1;
}

// A frame of this origin may overlap the scene's last launch as far as the records go: its origin is
// computed, or the buffer it would be computed into is one the last launch does not read.
inline bool fref_overlap_ok(const FrefSlots& f, const uint32_t ob[3])
{
    bool compute;
    return fref_slot(f, ob, f.last, &compute) >= 0;
}

// The buffer of a frame of this launch: fref_slot past the last launch's buffers (none for an ordered
// launch) and those that earlier frames of this launch read (`busy`).
inline int fref_slot_for_launch(const FrefSlots& f, const uint32_t ob[3], uint32_t busy, bool *compute)
{
    return fref_slot(f, ob, f.last | busy, compute);
}

// buffer b now holds origin ob (its k_origin_pre is in the stream)
inline void fref_computed(FrefSlots& f, int b, const uint32_t ob[3])
{
    std::memcpy(f.org[b], ob, 3 * sizeof(uint32_t));
    f.ok[b] = true;
}

// The next launch is ordered after every earlier launch of the scene (order_all, a host wait): none of
// them still reads a buffer, so none is busy.
inline void fref_ordered(FrefSlots& f)
{
    f.last = 0u;
}

// the launch just issued reads the buffers of mask `used` (0: no per-origin records at all)
inline void fref_launched(FrefSlots& f, uint32_t used)
{
    f.last = used;
}

} // namespace rtk
