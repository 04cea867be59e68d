// rt_miss_mask.h -- the proof behind the lane kernels' miss skip: provably_misses()
// answers true only if EVERY camera-space (x, y) of a rectangle gives a ray that rtd::ray_aabb_rcp
// rejects, that is a ray for which Grid::Intersect returns at its first test (aabb.h:34-83).  A work
// item whose 64 samples all lie in such a rectangle stores its row's miss colour without generating a ray.
//
// Plain double, no HIP types, no FMA (the library is built with -ffp-contract=off, the checker too):
// k_miss_mask (rt_plan.hip) runs these functions on the device, tests/miss_mask_check.cpp compiles the
// same ones with g++ against the oracle's GenRay / RayAABB.
//
// ---- what is enclosed ---------------------------------------------------------------------------
// rtd::dir_from_xy followed by rtd::ray_aabb_rcp, f32 operation by f32 operation, in their order:
//   d = 0 + x x + y y + z z (z = -1), s = sqrt(d), l = 1 / s, x' = x l, y' = y l, z' = z l,
//   D_c = (x' m[c] + y' m[3 + c]) + z' m[6 + c]            nine products, six sums
//   i_c = 1 / D_c, the slab order by its sign, t = (b - o) i     one difference, one product per bound
//   the two early returns, with the tmin / tmax selections between them (selections do not round)
// One enclosure serves every kernel variant: rcp_exact, rcp_nr and the IEEE division all return the
// correctly rounded 1 / d wherever the kernels use them (rt_debug_rcp_check, rt_setup_div.h).
//
// ---- why the widening is enough -----------------------------------------------------------------
// Every f32 operation above is op = +, -, *, /, sqrt, correctly rounded to nearest even: fl(v) with
// |fl(v) - v| <= 2^-24 |v| when fl(v) is normal and <= 2^-150 when it is subnormal (gradual underflow;
// overflow is excluded below).  Rounding is monotone, so with the operands anywhere in their intervals
// fl(v) lies in [fl(v_lo), fl(v_hi)], v_lo / v_hi the real minimum / maximum of op over the operand
// box (attained at the endpoints: sums, the four corner products, monotone 1 / x and sqrt on one sign).
// The header evaluates v_lo and v_hi in fp64 -- one fp64 operation on fp64 endpoints, so within 2^-53
// relative of the real value (a device sqrt or division that is a few fp64 ulp off is covered as well,
// see below), or within 2^-1074 absolute where the fp64 result itself underflows -- and then widens:
//   lo' = lo - (|lo| 2^-23 + 2^-140),   hi' = hi + (|hi| 2^-23 + 2^-140)                  (mm_round)
// 2^-23 |lo| >= (2^-24 + 2^-25) |v_lo| covers the f32 half ulp and leaves 2^-25 relative -- 2^28 fp64
// ulp -- for the fp64 evaluation, the widening's own two roundings included; 2^-140 covers the 2^-150
// of a subnormal f32 result and any fp64 underflow.  By induction over the operations every f32 value
// the kernel can form lies inside its interval.
//
// ---- when the answer is false without a proof ---------------------------------------------------
//   * the origin satisfies point_in_aabb (Grid::Intersect starts inside; nothing to skip);
//   * any bound is not finite or above 2^100 in magnitude (tested after every operation, so f32
//     overflow, inf - inf and 0 x inf never enter an enclosure; NaN fails the comparison);
//   * a direction component's interval touches zero or reaches below 2^-100 in magnitude (the slab
//     order then depends on the sample, and 1 / D_c could overflow).
// No property of the 3x3 is used: scaled, sheared and rank-deficient cameras take the same path and
// simply fail one of the tests above more often.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RT_MM_FN __host__ __device__ inline
#else
#define RT_MM_FN inline
#endif

namespace rtk {

constexpr double kMmRel = 0x1p-23;      // relative widening per f32 operation
constexpr double kMmAbs = 0x1p-140;     // absolute widening per f32 operation
constexpr double kMmBig = 0x1p100;      // no bound above this ...
constexpr double kMmTiny = 0x1p-100;    // ... and no direction component below this

struct MmIv { double lo, hi; };         // a closed interval, lo <= hi

RT_MM_FN double mm_abs(double v) { return v < 0.0 ? -v : v; }
RT_MM_FN double mm_min(double a, double b) { return a < b ? a : b; }
RT_MM_FN double mm_max(double a, double b) { return a > b ? a : b; }

// the enclosure of one f32 operation's result from the fp64 bounds of its real result; ok is cleared
// when a bound is not finite or above kMmBig
RT_MM_FN MmIv mm_round(double lo, double hi, bool& ok)
{
    MmIv r;
    r.lo = lo - (mm_abs(lo) * kMmRel + kMmAbs);
    r.hi = hi + (mm_abs(hi) * kMmRel + kMmAbs);
    if (!(r.lo >= -kMmBig && r.hi <= kMmBig)) ok = false;
    return r;
}

RT_MM_FN MmIv mm_pt(float v) { return MmIv{ double(v), double(v) }; }
RT_MM_FN MmIv mm_add(const MmIv& a, const MmIv& b, bool& ok) { return mm_round(a.lo + b.lo, a.hi + b.hi, ok); }
RT_MM_FN MmIv mm_mul(const MmIv& a, const MmIv& b, bool& ok)
{
    const double p0 = a.lo * b.lo, p1 = a.lo * b.hi, p2 = a.hi * b.lo, p3 = a.hi * b.hi;
    return mm_round(mm_min(mm_min(p0, p1), mm_min(p2, p3)), mm_max(mm_max(p0, p1), mm_max(p2, p3)), ok);
}
// 1 / a for an interval of one sign that excludes zero (the callers test it)
RT_MM_FN MmIv mm_rcp(const MmIv& a, bool& ok) { return mm_round(1.0 / a.hi, 1.0 / a.lo, ok); }
// f32 (b - o) * i with b and o exact f32 values
RT_MM_FN MmIv mm_slab(float b, float o, const MmIv& i, bool& ok)
{
    return mm_mul(mm_round(double(b) - double(o), double(b) - double(o), ok), i, ok);
}

// True only if every (x, y) in [xlo, xhi] x [ylo, yhi] gives rtd::dir_from_xy(m, x, y) a direction that
// rtd::ray_aabb_rcp(org, 1 / dir, bmin, bmax) rejects in f32.  m: the camera's 3x3 (KParams::m), org:
// its origin; all four arrays are exact f32 values.
RT_MM_FN bool provably_misses(const float *m, const float *org, const float *bmin, const float *bmax, double xlo,
                              double xhi, double ylo, double yhi)
{
    if (org[0] >= bmin[0] && org[1] >= bmin[1] && org[2] >= bmin[2] && org[0] <= bmax[0] && org[1] <= bmax[1] &&
        org[2] <= bmax[2])
        return false;                                               // rtd::point_in_aabb
    bool ok = true;
    if (!(xlo <= xhi && ylo <= yhi && xlo >= -kMmBig && xhi <= kMmBig && ylo >= -kMmBig && yhi <= kMmBig)) return false;
    const MmIv x{ xlo, xhi }, y{ ylo, yhi }, z = mm_pt(-1.0f);
    // d = 0; d += x * x; d += y * y; d += z * z  (the squares as products: an interval across zero
    // then reaches below zero, which is wider than needed and still an enclosure)
    MmIv d = mm_add(mm_pt(0.0f), mm_mul(x, x, ok), ok);
    d = mm_add(d, mm_mul(y, y, ok), ok);
    d = mm_add(d, mm_mul(z, z, ok), ok);
    if (!ok || !(d.lo > 0.0)) return false;
    const MmIv s = mm_round(__builtin_sqrt(d.lo), __builtin_sqrt(d.hi), ok);
    if (!ok || !(s.lo > 0.0)) return false;
    const MmIv len = mm_rcp(s, ok);
    const MmIv xn = mm_mul(x, len, ok), yn = mm_mul(y, len, ok), zn = mm_mul(z, len, ok);
    MmIv tn[3], tf[3];
    for (int c = 0; c < 3; c++)
    {
        // x * m[c] + y * m[3 + c] + z * m[6 + c], left to right
        MmIv D = mm_add(mm_mul(xn, mm_pt(m[c]), ok), mm_mul(yn, mm_pt(m[3 + c]), ok), ok);
        D = mm_add(D, mm_mul(zn, mm_pt(m[6 + c]), ok), ok);
        if (!ok) return false;
        const bool neg = D.hi < 0.0;
        if (!(neg ? D.hi <= -kMmTiny : D.lo >= kMmTiny)) return false;      // touches zero, or tiny
        const MmIv i = mm_rcp(D, ok);
        tn[c] = mm_slab(neg ? bmax[c] : bmin[c], org[c], i, ok);
        tf[c] = mm_slab(neg ? bmin[c] : bmax[c], org[c], i, ok);
        if (!ok) return false;
    }
    // if ((tmin > tymax) || (tymin > tmax)) return false;  -- certain for the whole rectangle
    if (tn[0].lo > tf[1].hi || tn[1].lo > tf[0].hi) return true;
    // if (tymin > tmin) tmin = tymin; if (tymax < tmax) tmax = tymax;  (for the rays that got here)
    const MmIv tmin{ mm_max(tn[0].lo, tn[1].lo), mm_max(tn[0].hi, tn[1].hi) };
    const MmIv tmax{ mm_min(tf[0].lo, tf[1].lo), mm_min(tf[0].hi, tf[1].hi) };
    // if ((tmin > tzmax) || (tzmin > tmax)) return false;
    return tmin.lo > tf[2].hi || tn[2].lo > tmax.hi;
}

} // namespace rtk
