// track_bucket.h - the bucket index of the point search of include/sid_track.h.  Plain C++ (no HIP), so
// that tests/cpp/track_bucket_check.cpp compiles it alone.  The search lays n buckets per axis over [lo, hi], the bounding box
// of the boxes of the usable cells.  A cell is entered into the buckets bucket(box_lo) .. bucket(box_hi) when the buckets are
// built, and a point looks into bucket(p).  Both use the ONE function below, and it is monotone in p: subtracting x0, scaling
// by inv >= 0, floor and the clamp each keep an order (an IEEE rounding does).  So box_lo <= p <= box_hi puts bucket(p)
// inside the cell's range whatever the roundings were - the search can be slow on a strange grid but never misses a cell.
#ifndef SID_TRACK_BUCKET_H
#define SID_TRACK_BUCKET_H

#include <math.h>
#include <stdint.h>

#ifndef SID_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SID_HD __host__ __device__
#else
#define SID_HD
#endif
#endif
#ifndef SID_HD_INLINE
#define SID_HD_INLINE SID_HD inline __attribute__((always_inline))
#endif

namespace sid_track {

// One axis of the bucket grid
struct Axis {
    double x0, inv;                                    // bucket = floor((p - x0) * inv), clamped to 0 .. n - 1
    int32_t n;
};

// n >= 1 buckets over [lo, hi].  A span that is empty, zero, not finite or so small that n / span overflows gives inv = 0:
// everything falls into bucket 0, which is still monotone.
SID_HD_INLINE Axis make_axis(double lo, double hi, int32_t n)
{
    Axis a;
    a.n = n < 1 ? 1 : n;
    a.x0 = 0.0;
    a.inv = 0.0;
    if (!(lo <= hi) || !isfinite(lo)) return a;
    a.x0 = lo;
    const double span = hi - lo;
    const double inv = (double)a.n / span;
    if (span > 0.0 && isfinite(inv)) a.inv = inv;
    return a;
}

// Not a number (only inf * 0 and a NaN p get there) goes to bucket 0 with everything else that is not above it.
SID_HD_INLINE int32_t bucket(const Axis &a, double p)
{
    const double t = floor((p - a.x0) * a.inv);
    if (!(t > 0.0)) return 0;
    if (t >= (double)(a.n - 1)) return a.n - 1;
    return (int32_t)t;
}

}  // namespace sid_track

#endif
