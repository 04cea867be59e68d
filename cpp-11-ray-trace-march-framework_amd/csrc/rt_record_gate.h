// rt_record_gate.h -- the u-slab gate of the per-camera-record test: a 7-instruction
// sufficient test for "the record's first half (rtd::mt_rec_first: det and u, triangle.h:77-87) rejects
// this ray", from operands precomputed per camera origin and a per-record error bound.  Never a
// geometric cull: a ray the gate does not reject takes the unchanged record test.
//
// Plain float / double, no HIP types: librt_tracer.so runs these functions (k_origin_pre: make_gate; the
// wave-uniform record loop of rt_walk.h: gate_rejects) and tests/record_gate_check.cpp compiles the same
// ones with g++ against the reference's first half.
//
// ---- derivation ------------------------------------------------------------------------------------
// One CSR reference with f32 e1, e2, T = o - v0 (as rtd::make_frec forms them) and an f32 ray direction
// D with |D_i| <= Dmax = 1.0001.  GenerateRay normalises the camera-space direction and multiplies by the
// camera's 3x3 AFTERWARDS, so this holds for an orthonormal camera and not for any rt_frame.cam: the host
// bounds |D_i| per frame from the matrix (rt_cam_bound.h) and passes the gate records only to frames inside
// Dmax (rt_launch.hip, frame_gated); the others take the ungated loop.  u = 2^-24, fl() = one f32 rounding,
// g_k = k u / (1 - k u).  The reference computes (rtd::mt_rec_first, the order of triangle.h:45-87)
//     p     = fl(D x e2)                          each component fl(fl(a b) - fl(c d))
//     det_r = fl(fl(fl(e1x px) + fl(e1y py)) + fl(e1z pz)),   y_r likewise with T for e1
//     u_r   = fl(y_r fl(1 / det_r))
//     ok1   = !(|det_r| < 1e-8) && !(u_r < 0 || u_r > 1)
// Exact values: Det = e1 . (D x e2) = D . (e2 x e1),  Y = T . (D x e2) = D . (e2 x T).
//
// (1) Rounding of det_r and y_r.  With s = (|e2y|+|e2z|, |e2x|+|e2z|, |e2x|+|e2y|): |p_i - (D x e2)_i|
//     <= g_2 Dmax s_i and |p_i| <= (1 + g_2) Dmax s_i.  In the dot each term passes at most three
//     roundings (its product, two sums), so |det_r - sum e1_i p_i| <= g_3 sum |e1_i| |p_i|.  Together
//         |det_r - Det| <= (g_2 + g_3 (1 + g_2)) Dmax sum |e1_i| s_i  <  6u Dmax sum |e1_i| s_i =: ed
//     (5u + O(u^2) < 6u), and |y_r - Y| <= 6u Dmax sum |T_i| s_i =: ey the same way.
//     Gradual underflow: a product that lands in the subnormals is off by <= 2^-150 absolute (sums of
//     subnormals are exact).  Nine products per dot, the six of p scaled by |e1_i| or |T_i| <= 2^40
//     (make_gate gives up above that): < 2^-106 in all, far inside the 2^-100 of E.  Inputs <= 2^40 also
//     keep every intermediate below 2^84: no overflow, so det_r, y_r and -- when |det_r| >= 1e-8 -- u_r
//     are finite and ok1 holds no NaN case for a finite-E record.
// (2) What ok1 implies.  u_r = q (1 + d1)(1 + d2) + eta with q = y_r / det_r, |d| <= u (the correctly
//     rounded reciprocal -- rcp_nr is exact wherever ok1 reads it -- and the product), |eta| <= 2^-150
//     (the product may underflow; the reciprocal of |det_r| < 2^84 is normal).  0 <= u_r <= 1 gives
//     -2^-149 <= q <= (1 - u)^-2 <= 1 + 3u, so |q - 1/2| <= 1/2 + 3u and
//         |y_r - det_r / 2| <= (1/2 + 3u) |det_r|.
//     With (1):  |Y - Det/2| <= |y_r - det_r/2| + ey + ed/2 <= (1/2 + 3u)(|Det| + ed) + ey + ed/2
//                             <= |Det|/2 + 3u |Det| + ey + 1.01 ed.
// (3) The two dots.  Y - Det/2 = D . NZ and Det/2 = D . NH with NZ = e2 x T - (e2 x e1)/2,
//     NH = (e2 x e1)/2.  So ok1 implies
//         |D . NZ| <= |D . NH| + 6u Dmax |NH|_1 + ey + 1.01 ed                    (3u |Det| = 6u |D . NH|).
// (4) The kernel's f32 evaluation.  nz = fl(NZ), nh = fl(NH) (u |N_i| each, or 2^-150 in the subnormals),
//     g = fl(fl(fl(dx n_x) + fl(dy n_y)) + fl(dz n_z)) (g_3 sum |D_i n_i|, three products that may
//     underflow): |g_z - D . NZ| <= (4u + O(u^2)) Dmax |nz|_1 + 2^-147, and the same for g_h.  Hence ok1
//     implies |g_z| <= |g_h| + B,
//         B = ey + 1.01 ed + 4u Dmax |nz|_1 + 4u Dmax |nh|_1 + 6u Dmax |nh|_1     (+ O(u^2) B + 2^-105).
// (5) The compare.  The record is rejected iff |g_z| > fl(|g_h| + E).  fl(x) >= x (1 - u), so no ok1 ray
//     is rejected when E (1 - u) >= B + u |g_h|; |g_h| <= (1 + 4u) Dmax |nh|_1 and B holds 10u Dmax
//     |nh|_1, so E = 2 B is (more than) enough: the factor 2 is the final add's rounding.
// (6) make_gate's own arithmetic is fp64: products of two f32 are exact, each of the few sums is off by
//     2^-53 of the magnitudes it adds -- together < 2^-51 Dmax (sum |T_i| s_i + sum |e1_i| s_i) in
//     D . N, against the 6u of ey + ed -- and B is a sum of positive terms (a dozen roundings of 2^-53).
//     These, and every O(u^2) above, are covered by the factor (1 + 2^-20); the underflow terms by 2^-100:
//         E = roundup_f32( 2 B (1 + 2^-20) + 2^-100 ).
// E = +inf (never rejected, n = 0) when a component of e1, e2 or T exceeds 2^40 in magnitude or is not
// finite, or B is not finite.  A NaN on either side of the compare (a NaN direction) does not reject:
// '>' is false.  The zero record of a buffer's pad rejects nothing (0 > 0 is false).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RT_GATE_HD __host__ __device__ __forceinline__
#else
#define RT_GATE_HD inline
#endif

namespace rtk {

// One gate record: 8 floats (32 B) per CSR reference, as (nz_i, nh_i) pairs for packed f32 math:
//   { nz.x, nh.x, nz.y, nh.y, nz.z, nh.z, E, 0 }
constexpr uint32_t kGateFloats = 8;
constexpr double kGateDmax = 1.0001;            // bound of a ray direction's components (rt_cam_bound.h checks it)
constexpr double kGateU = 1.0 / 16777216.0;     // 2^-24
constexpr double kGateMaxIn = 1099511627776.0;  // 2^40

RT_GATE_HD double gate_abs(double x) { return x < 0.0 ? -x : x; }

// x rounded to f32, upward (x > 0 and below FLT_MAX, or +inf / NaN -> +inf)
RT_GATE_HD float gate_round_up(double x)
{
    if (!(x < 3.0e38)) return __builtin_inff();
    float e = float(x);
    if (double(e) < x)
    {
        uint32_t b;
        __builtin_memcpy(&b, &e, 4);
        b += 1u;                                // the next float up (e > 0, finite)
        __builtin_memcpy(&e, &b, 4);
    }
    return e;
}

// The gate record of one reference for one camera origin (T = o - v0 as make_frec rounds it).
RT_GATE_HD void make_gate(float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float tx, float ty,
                          float tz, float g[kGateFloats])
{
    const double a1[3] = { e1x, e1y, e1z }, a2[3] = { e2x, e2y, e2z }, at[3] = { tx, ty, tz };
    bool big = false;
    for (int i = 0; i < 3; i++)
        big = big || !(gate_abs(a1[i]) <= kGateMaxIn) || !(gate_abs(a2[i]) <= kGateMaxIn) ||
              !(gate_abs(at[i]) <= kGateMaxIn);                       // (a NaN fails '<=')
    // NH = (e2 x e1) / 2, NZ = e2 x T - NH
    const double nh[3] = { 0.5 * (a2[1] * a1[2] - a2[2] * a1[1]), 0.5 * (a2[2] * a1[0] - a2[0] * a1[2]),
                           0.5 * (a2[0] * a1[1] - a2[1] * a1[0]) };
    const double nz[3] = { (a2[1] * at[2] - a2[2] * at[1]) - nh[0], (a2[2] * at[0] - a2[0] * at[2]) - nh[1],
                           (a2[0] * at[1] - a2[1] * at[0]) - nh[2] };
    const float fz[3] = { float(nz[0]), float(nz[1]), float(nz[2]) }, fh[3] = { float(nh[0]), float(nh[1]), float(nh[2]) };
    const double s[3] = { gate_abs(a2[1]) + gate_abs(a2[2]), gate_abs(a2[0]) + gate_abs(a2[2]),
                          gate_abs(a2[0]) + gate_abs(a2[1]) };
    const double sum_e1 = gate_abs(a1[0]) * s[0] + gate_abs(a1[1]) * s[1] + gate_abs(a1[2]) * s[2];
    const double sum_t = gate_abs(at[0]) * s[0] + gate_abs(at[1]) * s[1] + gate_abs(at[2]) * s[2];
    const double n1z = gate_abs(double(fz[0])) + gate_abs(double(fz[1])) + gate_abs(double(fz[2]));
    const double n1h = gate_abs(double(fh[0])) + gate_abs(double(fh[1])) + gate_abs(double(fh[2]));
    const double ud = kGateU * kGateDmax;
    const double B = 6.0 * ud * sum_t + 1.01 * (6.0 * ud * sum_e1) + 4.0 * ud * n1z + 4.0 * ud * n1h + 6.0 * ud * n1h;
    const double E = 2.0 * B * (1.0 + 1.0 / 1048576.0) + 0x1p-100;
    const float Ef = big ? __builtin_inff() : gate_round_up(E);
    const bool off = !(Ef < __builtin_inff());
    g[0] = off ? 0.0f : fz[0];
    g[1] = off ? 0.0f : fh[0];
    g[2] = off ? 0.0f : fz[1];
    g[3] = off ? 0.0f : fh[1];
    g[4] = off ? 0.0f : fz[2];
    g[5] = off ? 0.0f : fh[2];
    g[6] = off ? __builtin_inff() : Ef;
    g[7] = 0.0f;
}

// The gate predicate on pairs: V2 holds two floats x, y, with V2 * float (both elements times the
// scalar) and V2 + V2 as separately rounded f32 operations, no contraction: the device's v_pk_mul_f32 /
// v_pk_add_f32, or two plain operations each.
//   n0 = (nz.x, nh.x), n1 = (nz.y, nh.y), n2 = (nz.z, nh.z) of the gate record, E its bound
// True: the reference's first half rejects this ray (ok1 is false), proven; false: not known.
template <class V2>
RT_GATE_HD bool gate_rejects(float dx, float dy, float dz, V2 n0, V2 n1, V2 n2, float E)
{
    const V2 m = (n0 * dx + n1 * dy) + n2 * dz;                       // (g_z, g_h)
    return __builtin_fabsf(m.x) > __builtin_fabsf(m.y) + E;           // a NaN on either side: false
}

} // namespace rtk
