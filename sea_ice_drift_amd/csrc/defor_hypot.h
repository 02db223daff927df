// defor_hypot.h - float64 hypot restated from glibc's dbl-64 __hypot (glibc 2.35, sysdeps/ieee754/dbl-64/e_hypot.c), the
// libm function NumPy's float64 np.hypot calls.  One source for the deformation kernel and its host check (DESIGN.md
// section 15): compiled for the device inside defor.hip and for the host by the same translation unit, both with
// -ffp-contract=off, so every operation below is one IEEE float64 rounding, as in glibc built without __FP_FAST_FMA (the
// x86-64 baseline).
//
// The algorithm: sort |x|, |y| into ax >= ay; scale both by 2^-600 / 2^600 when ax > 2^511 or ay < 2^-511 (no overflow or
// underflow in the squares); return ax + ay when ay is below ax * 2^-54 (ay cannot change the correctly rounded result);
// otherwise h = sqrt(ax^2 + ay^2) corrected by one step of C. F. Borges, "An improved algorithm for hypot(a, b)" (2019).
// inf in either argument gives +inf (also with a quiet NaN in the other), any other NaN gives x + y.
#ifndef SID_DEFOR_HYPOT_H
#define SID_DEFOR_HYPOT_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SID_HD __host__ __device__
#else
#define SID_HD
#endif

namespace sid_defor {

SID_HD inline bool is_signaling(double x)
{
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return (b & 0x7ff0000000000000ull) == 0x7ff0000000000000ull && (b & 0x000fffffffffffffull) != 0 &&
           (b & 0x0008000000000000ull) == 0;
}

// ax >= ay >= 0, and squaring ax, ay and ax - ay neither overflows nor underflows
SID_HD inline double hypot_kernel(double ax, double ay)
{
    double t1, t2;
    double h = sqrt(ax * ax + ay * ay);
    if (h <= 2.0 * ay) {
        const double delta = h - ay;
        t1 = ax * (2.0 * delta - ax);
        t2 = (delta - 2.0 * (ax - ay)) * delta;
    } else {
        const double delta = h - ax;
        t1 = 2.0 * delta * (ax - 2.0 * ay);
        t2 = (4.0 * delta - ay) * ay + delta * delta;
    }
    h -= (t1 + t2) / (2.0 * h);
    return h;
}

SID_HD inline double hypot64(double x, double y)
{
    const double kScale = 0x1p-600, kLarge = 0x1p+511, kTiny = 0x1p-459, kEps = 0x1p-54;
    if (!isfinite(x) || !isfinite(y)) {
        if ((isinf(x) || isinf(y)) && !is_signaling(x) && !is_signaling(y)) return INFINITY;
        return x + y;
    }
    x = fabs(x);
    y = fabs(y);
    double ax = x < y ? y : x;
    const double ay = x < y ? x : y;
    if (ax > kLarge) {
        if (ay <= ax * kEps) return ax + ay;
        return hypot_kernel(ax * kScale, ay * kScale) / kScale;
    }
    if (ay < kTiny) {
        if (ax >= ay / kEps) return ax + ay;
        ax = hypot_kernel(ax / kScale, ay / kScale) * kScale;
        return ax;
    }
    if (ay <= ax * kEps) return ax + ay;
    return hypot_kernel(ax, ay);
}

}  // namespace sid_defor

#endif
