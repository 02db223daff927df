// corr_window.h - the per-window arithmetic of include/sid_corr.h, one source for the kernels of
// local_corr.hip and for their host instance (device = -1): where a node's centre lies, how its window is clipped, and the
// finalisation from the integer sums to r.  Every float64 operation is one IEEE rounding in the order of tests/corr_spec.py
// (-ffp-contract=off on both sides).
#ifndef SID_CORR_WINDOW_H
#define SID_CORR_WINDOW_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SID_CORR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SID_CORR_HD inline
#endif

namespace sid_corr {

enum { kTileRows = 8, kTileCols = 64 };               // SID_CORR_TILE_ROWS, SID_CORR_TILE_COLS of sid_corr.h

constexpr int64_t kFar = (int64_t)1 << 40;            // a centre beyond +-kFar counts as +-kFar: its window is empty either way

// The six integer sums of a window
struct Sums {
    int64_t n, sa, sb, saa, sbb, sab;
};

// Centre of lattice node i along one axis: origin + i * step (i >= 0, step >= 1), saturated at +-kFar without overflow
SID_CORR_HD int64_t centre(int64_t origin, int64_t i, int64_t step)
{
    int64_t p, c;
    if (__builtin_mul_overflow(i, step, &p)) return kFar;                  // (i * step >= 2^63, origin >= -2^63: beyond kFar)
    if (__builtin_add_overflow(origin, p, &c)) return kFar;                // (p >= 0: only upwards)
    return c < -kFar ? -kFar : c > kFar ? kFar : c;
}

// The window of side w around centre cc, clipped to [0, size): lo <= hi, empty when lo == hi
SID_CORR_HD void clip(int64_t cc, int w, int64_t size, int64_t &lo, int64_t &hi)
{
    lo = cc - w / 2;
    hi = lo + w;
    if (lo < 0) lo = 0;
    if (hi > size) hi = size;
    if (hi < lo) hi = lo;
}

SID_CORR_HD double quiet_nan()
{
    const uint64_t bits = 0x7ff8000000000000ull;
    double d;
    memcpy(&d, &bits, 8);
    return d;
}

// Sums -> r
SID_CORR_HD double finalise(const Sums &s, int64_t min_count)
{
    const int64_t va = s.n * s.saa - s.sa * s.sa, vb = s.n * s.sbb - s.sb * s.sb, cab = s.n * s.sab - s.sa * s.sb;
    if (s.n < min_count || va <= 0 || vb <= 0) return quiet_nan();
    const double prod = (double)va * (double)vb;
    const double r = (double)cab / sqrt(prod);
    return r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r;
}

// What a node writes (each output may be absent)
SID_CORR_HD void store(const Sums &s, int64_t min_count, int64_t node, double *corr, int32_t *count, int64_t *sums)
{
    if (corr) corr[node] = finalise(s, min_count);
    if (count) count[node] = (int32_t)s.n;
    if (sums) {
        int64_t *q = sums + 5 * node;
        q[0] = s.sa; q[1] = s.sb; q[2] = s.saa; q[3] = s.sbb; q[4] = s.sab;
    }
}

// One pixel pair into the sums
SID_CORR_HD void add_pixel(Sums &s, unsigned pa, unsigned pb)
{
    if (pa == 0 || pb == 0) return;
    s.n += 1; s.sa += pa; s.sb += pb;
    s.saa += (int64_t)(pa * pa); s.sbb += (int64_t)(pb * pb); s.sab += (int64_t)(pa * pb);
}

}  // namespace sid_corr
#endif
