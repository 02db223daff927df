// prep_pixel.h - the per-pixel function of the sigma0 preparation (include/sid_prep.h: dB, HH correction, mask, detrend),
// shared by prep.hip (which writes the pixel), landmask.hip (which asks whether it is finite) and resize.hip (which averages the
// full-resolution planes first): one text, one result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace {

// float32(log10(double(x))) for a float32 x > 0.  A short float64 evaluation - log10(x) =
// e log10(2) + 2 log10(e) atanh(s), s = (m - 1) / (m + 1), x = 2^e m with m in (sqrt(1/2), sqrt(2)], atanh by its series to
// s^17 (remainder 2^-50 of the result), a dozen roundings of 2^-53 each: relative error below 2^-45 - decides the float32
// value whenever both ends of a 2^-40 relative interval around it round to the same float32; the other pixels (one in
// 45 770 of all float32: the interval straddles a rounding boundary) take the library's float64 log10.  sid_prep_debug_log10 compares
// the two routes on any range of float32 bit patterns; tests/test_gpu_prepare.py runs it over every positive float32.
__device__ __forceinline__ float log10_f32(float x, bool *slow = nullptr)
{
    if (slow) *slow = false;
    if (x > 3.402823466e38f) return x;                                     // +inf
    const double xd = (double)x;                                           // exact; normal for every positive float32
    const long long b = __double_as_longlong(xd);
    int e = (int)(b >> 52) - 1023;
    double m = __longlong_as_double((b & 0x000fffffffffffffLL) | 0x3ff0000000000000LL);   // [1, 2)
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }                   // exact
    const double f = m - 1.0, d = 2.0 + f;                                 // f exact; d in [1.70, 2.42]
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    double s = f * r;
    s = fma(fma(-d, s, f), r, s);                                          // f / d to an ulp; |s| <= 0.1716
    const double z = s * s;
    double p = 1.0 / 17.0;
    p = fma(p, z, 1.0 / 15.0); p = fma(p, z, 1.0 / 13.0); p = fma(p, z, 1.0 / 11.0); p = fma(p, z, 1.0 / 9.0);
    p = fma(p, z, 1.0 / 7.0); p = fma(p, z, 1.0 / 5.0); p = fma(p, z, 1.0 / 3.0);
    const double at = fma(s, z * p, s);                                    // atanh(s)
    const double L = fma((double)e, 0.30102999566398119521, at * 0.86858896380650365530);   // log10(2), 2 log10(e)
    const double w = fabs(L) * 9.094947017729282e-13;                      // 2^-40
    const float lo = (float)(L - w), hi = (float)(L + w);
    if (lo == hi) return lo;
    if (slow) *slow = true;
    return (float)log10(xd);
}

__device__ __forceinline__ float prep_pixel(bool db, bool hh, bool msk, bool mean, float x, float ia, uint32_t m, float f, double mu)
{
    const float nan = __int_as_float(0x7fc00000);
    float v = x;
    if (db) v = x > 0.0f ? 10.0f * log10_f32(x) : nan;                     // (NaN fails the comparison)
    if (hh) { const float t = ia * f; v = v - t; }
    if (msk) v = m ? nan : v;
    if (mean) v = (float)((double)v - mu);
    return v;
}

struct Coef { double c[6]; };            // x[0] of the reference's lstsq: col, col^2, row, row^2, col*row, 1

// the polynomial at (row, col) in the reference's order of operations (lib.py:248-253); c2r = c[2] * row and
// c3r2 = c[3] * row^2 are the same for a whole row
__device__ __forceinline__ double spatial_mean(const Coef &K, int64_t col, double dr, double c2r, double c3r2)
{
    const double dc = (double)col, dc2 = (double)(col * col);
    double m = K.c[0] * dc;
    m = m + K.c[1] * dc2;
    m = m + c2r;
    m = m + c3r2;
    m = m + (K.c[4] * dc) * dr;
    m = m + K.c[5];
    return m;
}

}  // namespace
