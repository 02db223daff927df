// fg_knn.h - the arithmetic of sid_fg_knn (include/sid_fg.h): the sorted list of the k nearest seeds and
// the median of their values, one source for the kernels of first_guess.hip and for their host instance (device = -1).  Every
// float64 operation is one IEEE rounding in the order of tests/fg_knn_spec.py (-ffp-contract=off on both sides).
#ifndef SID_FG_KNN_H
#define SID_FG_KNN_H

#include <math.h>
#include <stdint.h>

#include "defor_hypot.h"                               // SID_HD

#ifndef SID_HD_INLINE
#define SID_HD_INLINE SID_HD inline __attribute__((always_inline))
#endif

namespace sid_knn {

constexpr int kMaxK = 16;
constexpr int32_t kEmpty = 0x7fffffff;                 // index of an empty slot: above every seed index (n_seeds < 2^31)

// The K best (d2, index) pairs seen so far in ascending lexicographic order; empty slots hold (+inf, kEmpty) and so sort
// behind every real pair, one with d2 = +inf included.  Every slot is addressed by a compile-time index (the loops over K
// unroll), so the device keeps the list in registers: an array indexed at run time would live in scratch.
template <int K>
struct List { double d[K]; int32_t i[K]; };

template <int K>
SID_HD_INLINE void clear(List<K> &l)
{
#pragma unroll
    for (int j = 0; j < K; ++j) { l.d[j] = INFINITY; l.i[j] = kEmpty; }
}

SID_HD_INLINE double dist2(double q0, double q1, double s0, double s1)
{
    const double dx = q0 - s0, dy = q1 - s1;
    return dx * dx + dy * dy;
}

// Offer seed `idx` at squared distance d2: dropped when it is not admissible (d2 <= m2) or not before the last slot; else one
// carry-and-swap pass puts it in its place and pushes the last pair out.
template <int K>
SID_HD_INLINE void offer(List<K> &l, double d2, int32_t idx, double m2)
{
    if (!(d2 <= m2)) return;
    if (!(d2 < l.d[K - 1] || (d2 == l.d[K - 1] && idx < l.i[K - 1]))) return;
    double cd = d2;
    int32_t ci = idx;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool lt = cd < l.d[j] || (cd == l.d[j] && ci < l.i[j]);
        const double td = lt ? l.d[j] : cd;
        const int32_t ti = lt ? l.i[j] : ci;
        l.d[j] = lt ? cd : l.d[j];
        l.i[j] = lt ? ci : l.i[j];
        cd = td;
        ci = ti;
    }
}

// slot k - 1 is taken and its d2 <= bound: the first k slots cannot change through any seed whose d2 exceeds `bound`
template <int K>
SID_HD_INLINE bool full_within(const List<K> &l, int k, double bound)
{
    bool r = false;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j == k - 1) r = l.i[j] != kEmpty && l.d[j] <= bound;
    return r;
}

// Median of the m values of a[] that are not NaN (the others are padding), by rank selection: a candidate c is the r-th
// smallest when (#values < c) <= r < (#values <= c).  m odd: the middle value; m even: (s[m/2-1] + s[m/2]) / 2; m = 0: NaN.
template <int K>
SID_HD_INLINE double median(const double a[K], int m)
{
    const int r2 = m / 2, r1 = (m & 1) ? r2 : r2 - 1;
    double v1 = NAN, v2 = NAN;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double c = a[j];
        int lt = 0, le = 0;
#pragma unroll
        for (int t = 0; t < K; ++t) { lt += a[t] < c; le += a[t] <= c; }
        if (lt <= r1 && r1 < le) v1 = c;
        if (lt <= r2 && r2 < le) v2 = c;
    }
    return (m & 1) ? v2 : (v1 + v2) / 2.0;
}

// The result of one query from its finished list: the first m = min(k, pairs in the list) are the neighbours; out2 = the
// medians of their two value columns (NaN, NaN for m = 0), *cnt = m, idx[0..k) = their seed indices, padded with -1.
template <int K>
SID_HD_INLINE void finish(const List<K> &l, const double *values, int k, double *out2, int32_t *cnt, int32_t *idx)
{
    double a[K], b[K];
    int m = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool on = j < k && l.i[j] != kEmpty;
        m += on;
        a[j] = on ? values[2 * (int64_t)l.i[j]] : NAN;
        b[j] = on ? values[2 * (int64_t)l.i[j] + 1] : NAN;
        if (j < k) idx[j] = on ? l.i[j] : -1;
    }
    out2[0] = median<K>(a, m);
    out2[1] = median<K>(b, m);
    *cnt = m;
}

// One query against every seed in index order: the host instance, and the definition the kernels are held to.
SID_HD_INLINE void brute(const double *seeds, const double *values, int64_t ns, double q0, double q1, int k, double m2,
                         double *out2, int32_t *cnt, int32_t *idx)
{
    List<kMaxK> l;
    clear(l);
    if (isfinite(q0) && isfinite(q1))
        for (int64_t s = 0; s < ns; ++s) offer(l, dist2(q0, q1, seeds[2 * s], seeds[2 * s + 1]), (int32_t)s, m2);
    finish<kMaxK>(l, values, k, out2, cnt, idx);
}

}  // namespace sid_knn

#endif
