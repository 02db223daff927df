// Normalisation of the winner's NCC matrix: the specification's route and the shortened one, as plain arithmetic that the
// kernels (through pm_kernel_base.h) and the host check (tests/cpp/ncc_norm_check.cpp) both compile.
// Everything here counts IEEE roundings: build with -ffp-contract=off; the fused operations are written out as __builtin_fma.
//
// Inputs of one placement (all integers, re-centred int8 domain w' = w - 128, t' = t - 128 ... see DESIGN.md section 3):
//   p    = sum w' t'      swp = sum w'      siiv = sum w'^2      nd = N = side^2      sT = sum t'      rTd = 1 / sqrt(dT)
// Bounds: nd <= 255^2 < 2^16, siiv <= nd 2^14, |swp| and |sT| <= 128 nd, |p| <= nd 2^14.  Hence nd siiv, swp^2, nd p and swp sT
// are integers below 2^46: every product below is exact in double, and so is each difference of two of them (< 2^53).
#ifndef SID_NCC_NORM_H
#define SID_NCC_NORM_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SID_NCC_HD __host__ __device__ __forceinline__
#else
#define SID_NCC_HD inline
#endif

namespace ncc_norm {

// guard band around the float32 rounding midpoints of q (bit 28 of the 29 discarded mantissa bits): +- 64 ulps of double
constexpr uint32_t kBandLo = 0x10000000u - 64u, kBandWidth = 128u;
// |q| >= kEdge: the lane does not take the plain conversion (clamp thresholds 1 and 1.125, each with a 1e-13 neighbourhood
// that the specification's own route decides)
constexpr double kNear = 1e-13, kEdge = 1.0 - 1e-13;

SID_NCC_HD uint32_t lo32(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return (uint32_t)u; }

// ---- the specification: IEEE double, 1 / sqrt with two roundings, no fused operation ----
SID_NCC_HD float spec_ncc(double numer, double dI, double rTd, bool constT, bool lowvar)
{
    if (constT) return 1.0f;
    if (lowvar) return 0.0f;
    const double rI = 1.0 / sqrt(dI);
    double q = numer * rI;
    q = q * rTd;
    const double aq = __builtin_fabs(q);
    return aq < 1.0 ? (float)q : (aq < 1.125 ? (q > 0.0 ? 1.0f : -1.0f) : 0.0f);
}

SID_NCC_HD float spec_from_sums(int p, int swp, uint32_t siiv, double nd, double sT, double rTd, bool cT)
{
    const double swd = (double)swp, siid = (double)siiv;
    const double dI = nd * siid - swd * swd;                           // exact
    const double s2 = siid + 256.0 * swd + 16384.0 * nd;               // S_II in the uint8 domain
    const bool lowvar = (2.0 * dI <= nd) && (dI * 8388608.0 <= 10.0 * nd * s2);
    const double numer = nd * (double)p - swd * sT;                    // exact
    return spec_ncc(numer, dI, rTd, cT, lowvar);
}

// ---- the shortened route ----
// What a batch of placements shares (hoisted by the caller): N / 2 and 2 / sqrt(dT), both exact scalings.
struct Hoisted {
    double nd, half_nd, sT, rT2;
    static SID_NCC_HD Hoisted make(double nd, double sT, double rTd) { Hoisted h; h.nd = nd; h.half_nd = 0.5 * nd; h.sT = sT; h.rT2 = 2.0 * rTd; return h; }
};

// The value of a lane that is not flagged, and the double q' it came from.  dI and numer: one product is rounded (exactly,
// see the bounds above), the other rides in the fma, whose single rounding is exact as well - the same integers as the
// specification's two-rounding forms.  1 / (2 sqrt(dI)) from the seed rsq(dI) and two coupled Newton steps: |q' - q| < 2^-49 |q|
// for any seed good to 2^-20 or so.  dI feeds the seed as it is: a lane with dI <= N / 2 (zero and negative included; its q'
// may be inf or NaN) is flagged by one compare and its value is discarded.  Every flag is written so that a NaN sets it.
//   flagged <=> dI <= N / 2, or q' within 64 ulps of a float32 rounding midpoint, or not |q'| < 1 - 1e-13
template <class Rsq>
SID_NCC_HD float lean(int p, int swp, uint32_t siiv, const Hoisted &c, Rsq rsq, bool &flagged, double &q_out)
{
    const double swd = (double)swp, siid = (double)siiv;
    const double dI = __builtin_fma(-swd, swd, c.nd * siid);           // exact
    const double numer = __builtin_fma(-swd, c.sT, c.nd * (double)p);  // exact
    const double y0 = rsq(dI);
    double g = dI * y0, h = 0.5 * y0;
    double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g); h = __builtin_fma(h, r, h);
    r = __builtin_fma(-h, g, 0.5);
    h = __builtin_fma(h, r, h);                                        // 1 / (2 sqrt(dI))
    const double q = (numer * h) * c.rT2;
    const uint32_t lo29 = lo32(q) & 0x1fffffffu;
    bool fl = !(dI > c.half_nd);                                       // the low-variance rule needs a second look
    fl |= (lo29 - kBandLo) <= kBandWidth;
    fl |= !(__builtin_fabs(q) < kEdge);
    flagged = fl;
    q_out = q;
    return (float)q;
}

// A flagged lane (rare; callers branch here behind the batch).  An edge lane with |q'| >= 1 and dI > N / 2 that is not
// within 1e-13 of a threshold lies on its side of both thresholds by far more than q' is off (2^-49 |q|): the clamp is
// decided without the specification's route.  Everything else (low variance, rounding midpoints, the thresholds'
// neighbourhoods, NaN) takes the specification.
// spec_route: whether it did.
SID_NCC_HD float flagged_value(int p, int swp, uint32_t siiv, const Hoisted &c, double rTd, double q, bool &spec_route)
{
    const double swd = (double)swp, siid = (double)siiv;
    const double dI = __builtin_fma(-swd, swd, c.nd * siid);
    const double aq = __builtin_fabs(q);
    const bool nearthr = __builtin_fabs(aq - 1.0) < kNear || __builtin_fabs(aq - 1.125) < kNear;
    const bool clamp = dI > c.half_nd && aq >= 1.0 && !nearthr;        // (false for NaN)
    spec_route = !clamp;
    if (clamp) return aq < 1.125 ? (q > 0.0 ? 1.0f : -1.0f) : 0.0f;
    return spec_from_sums(p, swp, siiv, c.nd, c.sT, rTd, false);
}

// One value, start to end (the selftest kernel and the host check; the kernels batch `lean` and branch once per batch).
// A constant template gives 1 whatever the window.
template <class Rsq>
SID_NCC_HD float from_sums_fast(int p, int swp, uint32_t siiv, double nd, double sT, double rTd, bool cT, Rsq rsq, bool &spec_route)
{
    spec_route = false;
    if (cT) return 1.0f;
    const Hoisted c = Hoisted::make(nd, sT, rTd);
    bool fl; double q;
    float out = lean(p, swp, siiv, c, rsq, fl, q);
    if (fl) out = flagged_value(p, swp, siiv, c, rTd, q, spec_route);
    return out;
}

}  // namespace ncc_norm

#endif
