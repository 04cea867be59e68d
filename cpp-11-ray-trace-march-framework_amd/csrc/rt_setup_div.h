// rt_setup_div.h -- the quotients of the per-axis DDA setup (grid.cpp:190-216: (edge - g) / d and
// cw / d per axis, rt_walk.h dda_setup) over ONE reciprocal per axis: 5 instructions per quotient
// instead of the 11 of the correctly rounded f32 division, same bits as n / d.
//
// Plain float, no HIP types: librt_tracer.so runs these functions (dda_setup) and
// tests/setup_div_check.cpp compiles the same ones with g++ against the IEEE n / d.
//
// ---- why setup_div(n, d, r) == n / d ------------------------------------------------------------
// f32, round to nearest even, u = 2^-24, fl() = one rounding.  Inside the window below, with
// r = fl(1 / d) the correctly rounded reciprocal (rtd::rcp_nr, proven equal to 1.0f / d over every
// float of 2^-126 <= |d| < 2^126 by rt_debug_rcp_check; the checker uses 1.0f / d):
//   q0 = fl(n r)               = (n / d)(1 + a)(1 + b), |a|, |b| <= u: within 2u + u^2 of n / d,
//                              under 2 ulp(q0)
//   e0 = fl(n - d q0)          one rounding of the exact remainder (an integer k 2^(ed + eq - 46),
//                              |k| < 2^25: exact unless k needs its 25th bit): (n - d q0)(1 + c), |c| <= u
//   q1 = fl(q0 + e0 r)         q0 + e0 r = n / d + (n / d - q0)(a' + c'), |a'|, |c'| <~ u, is within
//                              (2u + u^2) 2.01u < 2^-45 (relative) of n / d.  Rounding a value that
//                              close to n / d gives one of the two floats that bracket n / d (n / d
//                              itself when it is a float): q1 is a FAITHFUL quotient
//   e1 = n - d q1              EXACTLY: |q1 - n / d| < ulp(q1) makes it an integer k 2^(ed + eq - 46)
//                              with |k| < 2^24 (the exact-remainder property of an FMA), and no part
//                              of it is lost to underflow, see (W2)
//   q2 = fl(q1 + e1 r)         = fl(n / d): Markstein's theorem (P. Markstein, "Computation of
//                              elementary functions on the IBM RISC System/6000 processor", 1990;
//                              Muller et al., Handbook of Floating-Point Arithmetic, "division with
//                              an FMA"): a faithful q, its exact remainder and the CORRECTLY ROUNDED
//                              reciprocal give the correctly rounded quotient in one step, for every
//                              n and d when nothing under- or overflows
// The first correction only makes the quotient faithful -- the compiler's own expansion of the division
// refines twice after its scaling for the same reason.
//
// ---- the window --------------------------------------------------------------------------------
//   (W)  2^-40 <= |n| <= 2^40  and  2^-40 <= |d| <= 2^40          (kSetupDivLo, kSetupDivHi)
// (W1) r, q0, q1, q2 are normal: 2^-41 < |r| < 2^41, 2^-81 < |q| < 2^81.  No overflow, no
//      subnormal quotient or reciprocal; NaN, inf and zero fail (W).
// (W2) with 2^en <= |n| < 2^(en + 1) (likewise ed, eq): d q is a multiple of 2^(ed + eq - 46), n of
//      2^(en - 23), and ed + eq >= en - 2, so a remainder is zero or at least 2^(en - 48) >= 2^-88 in
//      magnitude: far above the subnormals, nothing of it is lost.  e r is then zero or above
//      2^(-88 - 41), and every FMA rounds once, in the normal range.
// (W3) n = 0 is outside (W) on purpose: q0 = +-0 keeps the sign of n / d, but the correction
//      (+0) r + q0 would turn a -0 quotient into +0.
// Outside (W) -- a zero, denormal, huge, infinite or NaN operand; an axis-parallel ray has d = 0 --
// the caller divides (a wave-uniform vote in dda_setup, built like rtd::rcp_exact's: the common
// wave pays only the compares).  The scenes' coordinates and cell widths are O(2^-10 .. 2^10), and a
// normalised direction component below 2^-40 means a ray within 10^-12 of axis-parallel.
// tests/test_setup_div.py: every (n, d) of dda_setup over four scenes' frames and 7 x 10^7 crafted
// pairs, bit for bit, and every pair outside (W) must report the fall-back.
#pragma once

#if defined(__HIPCC__)
#define RT_SDIV_HD __host__ __device__ __forceinline__
#else
#define RT_SDIV_HD inline
#endif

namespace rtk {

constexpr float kSetupDivLo = 0x1p-40f, kSetupDivHi = 0x1p40f;

// (W) for one operand (NaN fails every compare)
RT_SDIV_HD bool setup_div_operand_ok(float x)
{
    const float a = __builtin_fabsf(x);
    return a >= kSetupDivLo && a <= kSetupDivHi;
}

#if defined(__HIPCC__)
// The wave's lanes whose x fails (W), for dda_setup's vote: the two compares of setup_div_operand_ok
// as two ballots (a single compare's lane mask IS its ballot; a combined predicate would be
// materialised in a VGPR and compared back, rt_wave.h wave_all).
__device__ __forceinline__ unsigned long long setup_div_bad_lanes(float x)
{
    const float a = __builtin_fabsf(x);
    return __builtin_amdgcn_ballot_w64(!(a >= kSetupDivLo)) | __builtin_amdgcn_ballot_w64(!(a <= kSetupDivHi));
}
#endif

// n / d from r = the correctly rounded 1.0f / d, for (n, d) inside (W)
RT_SDIV_HD float setup_div(float n, float d, float r)
{
    float q = n * r;
    float e = __builtin_fmaf(-d, q, n);
    q = __builtin_fmaf(e, r, q);
    e = __builtin_fmaf(-d, q, n);
    return __builtin_fmaf(e, r, q);
}

}  // namespace rtk
