// rt_cam_bound.h -- how long a camera ray's direction components can be, from the frame's 3x3 alone.
//
// Host only, plain float / double: librt_tracer.so calls it once per frame where it picks the frame's
// traversal features (rt_launch.hip: frame_gated, frame_traversal_bits), and tests/record_gate_check.cpp compiles the same
// function, so the library and the checker cannot disagree about which cameras keep the record gate.
//
// rt_frame.cam is the caller's matrix and need not be orthonormal.  rtd::dir_from_xy (camera.h:39-46)
// normalises the camera-space direction p first and multiplies by the 3x3 afterwards,
//     D_i = fl(fl(fl(px m[i]) + fl(py m[3 + i])) + fl(pz m[6 + i])),      | |p| - 1 | <= 4u, u = 2^-24,
// so by Cauchy-Schwarz |D_i| <= |p| |column i| (1 + 3u) before underflow: the column norm times
// (1 + 2^-20) covers the roundings of p, of the three products and two sums, and of this function's own
// fp64 arithmetic (squares of f32 are exact in fp64; two sums and a square root).
//
// Two proofs lean on the bound:
//   * the record gate (rt_record_gate.h): its per-record E holds for |D_i| <= kGateDmax = 1.0001.  A frame
//     above that -- or with a non-finite entry -- runs without gate records (KParams::gates = nullptr), the
//     loop a scene created with RT_REC_GATE=0 always takes;
//   * kVarFastRcp (rt_ray_common.h): rcp_nr is exact for |det| < 2^126, which rcp_safe guarantees for
//     |D|_inf <= kRcpMaxDir = 8.  A frame above that takes the instantiations without kVarFastRcp, the ones
//     a scene with rcp_safe = 0 always takes.
#pragma once
#include <cmath>

#include "rt_record_gate.h"     // kGateDmax

namespace rtk {

// rt_ray_common.h's kRcpMaxDir (asserted equal there): the |d|_inf up to which rcp_safe covers kVarFastRcp
constexpr double kCamRcpMaxDir = 8.0;

// The bound of |D_i| over every camera ray of a frame whose 3x3 is m (row-vector convention, m[3 r + c], as
// KParams::m): max over the three columns; +inf or NaN when an entry is not finite.
inline double cam_dir_bound(const float m[9])
{
    double b = 0.0;
    for (int i = 0; i < 3; i++)
    {
        const double a = m[i], c = m[3 + i], e = m[6 + i];
        const double n = std::sqrt(a * a + c * c + e * e) * (1.0 + 1.0 / 1048576.0);
        if (n != n) return n;                       // a NaN entry: the bound is NaN
        if (n > b) b = n;
    }
    return b;
}

// What a frame of that bound may use; a NaN bound fails both.
inline bool cam_gate_ok(double bound) { return bound <= kGateDmax; }
inline bool cam_fast_rcp_ok(double bound) { return bound <= kCamRcpMaxDir; }

// the same from a 4x4 view matrix as rt_frame.cam holds it (rows: right, up, back, eye)
inline double cam_dir_bound44(const float cam[16])
{
    const float m[9] = { cam[0], cam[1], cam[2], cam[4], cam[5], cam[6], cam[8], cam[9], cam[10] };
    return cam_dir_bound(m);
}

} // namespace rtk
