// grid_cell.h - the per-cell triangle rule, the per-node normalised median test and the per-node gap
// fill and smoothing (section 23) of include/sid_grid.h, one source for the kernels of drift_grid.hip and for their host
// instance (device = -1).  Every float64 operation is one IEEE rounding in the order of tests/grid_spec.py and
// tests/grid_fill_spec.py (-ffp-contract=off on both sides).
#ifndef SID_GRID_CELL_H
#define SID_GRID_CELL_H

#include <math.h>
#include <stdint.h>

#include "defor_elem.h"

namespace sid_grid {

enum { kShorter = 0, kMain = 1, kAnti = 2 };          // SID_GRID_DIAG_* of sid_grid.h

// q[k] for a run-time k in 0..3 without indexing an array by it (that would put the array into scratch on the device)
SID_HD_INLINE double pick(const double q[4], int k) { return k == 0 ? q[0] : k == 1 ? q[1] : k == 2 ? q[2] : q[3]; }

// The triangle slots of one grid cell, before orientation.  Ring nodes 0..3 = A, B, E, D (A = (i, j), B = (i, j + 1),
// E = (i + 1, j + 1), D = (i + 1, j)); bit k of `usable` is set when ring node k is usable; x, y hold the four nodes in ring
// order.  Slot s is the ring nodes (ta[s], tb[s], tc[s]), or ta[s] = -1 when it holds no triangle.  (Also the cells of
// warp_pixel.h.)
SID_HD_INLINE void split(const double x[4], const double y[4], unsigned usable, int diagonal, int ta[2], int tb[2], int tc[2])
{
    ta[0] = ta[1] = tb[0] = tb[1] = tc[0] = tc[1] = -1;
    const int n = (int)(usable & 1) + (int)((usable >> 1) & 1) + (int)((usable >> 2) & 1) + (int)((usable >> 3) & 1);
    if (n == 4) {
        const double mx = x[2] - x[0], my = y[2] - y[0], ax = x[3] - x[1], ay = y[3] - y[1];
        const double dm = mx * mx + my * my, da = ax * ax + ay * ay;
        const bool anti = diagonal == kAnti || (diagonal == kShorter && da < dm);
        ta[0] = 0; tb[0] = 1; tc[0] = anti ? 3 : 2;                 // main: (A, B, E), (A, E, D); anti: (A, B, D), (B, E, D)
        ta[1] = anti ? 1 : 0; tb[1] = 2; tc[1] = 3;
    } else if (n == 3) {                                            // the three usable nodes in ring order
        const int gone = !(usable & 1) ? 0 : !(usable & 2) ? 1 : !(usable & 4) ? 2 : 3;
        ta[0] = gone == 0 ? 1 : 0; tb[0] = gone <= 1 ? 2 : 1; tc[0] = gone == 3 ? 2 : 3;
    }
}

// One grid cell: x, y, u, v hold the four nodes in ring order (anything where not usable: never read into a result).  `ids`
// are the flat node numbers of the ring.  Writes slot s = 0, 1 to out[5][2] (e1, e2, e3, a, p) and t[2][3]: NaN and -1 where
// the slot holds no triangle.
SID_HD_INLINE void cell(const double x[4], const double y[4], const double u[4], const double v[4], unsigned usable, int diagonal,
                        const int32_t ids[4], double out[5][2], int32_t t[2][3])
{
    int ta[2], tb[2], tc[2];
    split(x, y, usable, diagonal, ta, tb, tc);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (ta[s] < 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) out[k][s] = NAN;
            t[s][0] = -1; t[s][1] = -1; t[s][2] = -1;
            continue;
        }
        int a = ta[s], b = tb[s], c = tc[s];
        const double xa = pick(x, a), ya = pick(y, a);
        const double cr = (pick(x, b) - xa) * (pick(y, c) - ya) - (pick(x, c) - xa) * (pick(y, b) - ya);
        if (cr < 0.0) { const int w = b; b = c; c = w; }             // counter-clockwise, as matplotlib's triangles are
        const double xs[3] = {xa, pick(x, b), pick(x, c)}, ys[3] = {ya, pick(y, b), pick(y, c)};
        const double us[3] = {pick(u, a), pick(u, b), pick(u, c)}, vs[3] = {pick(v, a), pick(v, b), pick(v, c)};
        sid_defor::triangle(xs, ys, us, vs, out[0][s], out[1][s], out[2][s], out[3][s], out[4][s]);
        t[s][0] = a == 0 ? ids[0] : a == 1 ? ids[1] : a == 2 ? ids[2] : ids[3];
        t[s][1] = b == 0 ? ids[0] : b == 1 ? ids[1] : b == 2 ? ids[2] : ids[3];
        t[s][2] = c == 0 ? ids[0] : c == 1 ? ids[1] : c == 2 ? ids[2] : ids[3];
    }
}

// The filter's view of one node's window.  `Get` is a functor: get(di, dj, a, b) gives the neighbour at (row + di, col + dj)
// as two values, NaN in both when that node is unusable or outside the grid (a NaN compares false with everything, so it is
// never counted and never a candidate).

// Medians of the a's and of the b's of the window (centre excluded), n values each, by rank selection: a candidate c is the
// k-th smallest when (#values < c) <= k < (#values <= c).  n odd: the middle value; n even: (s[n/2-1] + s[n/2]) / 2.
// The window's side is a template argument: the loop over the values is then unrolled, and since the values do not depend on
// the candidate the device keeps them in registers (static indices) instead of reading them once per candidate.
template <int radius, class Get>
SID_HD_INLINE void medians(const Get &get, int n, double &ma, double &mb)
{
    const int k2 = n / 2, k1 = (n & 1) ? k2 : k2 - 1;
    double a1 = NAN, a2 = NAN, b1 = NAN, b2 = NAN;
    for (int pi = -radius; pi <= radius; ++pi)
        for (int pj = -radius; pj <= radius; ++pj) {
            if (pi == 0 && pj == 0) continue;
            double ca, cb;
            get(pi, pj, ca, cb);
            if (!(ca == ca)) continue;
            int la = 0, ea = 0, lb = 0, eb = 0;
#pragma unroll
            for (int qi = -radius; qi <= radius; ++qi)
#pragma unroll
                for (int qj = -radius; qj <= radius; ++qj) {
                    if (qi == 0 && qj == 0) continue;
                    double qa, qb;
                    get(qi, qj, qa, qb);
                    la += qa < ca; ea += qa <= ca;
                    lb += qb < cb; eb += qb <= cb;
                }
            if (la <= k1 && k1 < ea) a1 = ca;
            if (la <= k2 && k2 < ea) a2 = ca;
            if (lb <= k1 && k1 < eb) b1 = cb;
            if (lb <= k2 && k2 < eb) b2 = cb;
        }
    ma = (n & 1) ? a2 : (a1 + a2) / 2.0;
    mb = (n & 1) ? b2 : (b1 + b2) / 2.0;
}

// |value - median| of a window, as a Get of its own (NaN stays NaN)
template <class Get>
struct Deviation {
    const Get &get;
    double ma, mb;
    SID_HD_INLINE void operator()(int di, int dj, double &a, double &b) const
    {
        get(di, dj, a, b);
        a = fabs(a - ma);
        b = fabs(b - mb);
    }
};

// The normalised median test of one node whose own values are (uc, vc), NaN in both when it is unusable.
template <int radius, class Get>
SID_HD_INLINE void filter_node_r(const Get &get, double uc, double vc, double eps, double threshold, int min_neighbours,
                                 uint8_t &keep, double &res)
{
    keep = 0;
    res = NAN;
    if (!(uc == uc)) return;
    int n = 0;
#pragma unroll
    for (int di = -radius; di <= radius; ++di)
#pragma unroll
        for (int dj = -radius; dj <= radius; ++dj) {
            if (di == 0 && dj == 0) continue;
            double a, b;
            get(di, dj, a, b);
            n += a == a;
        }
    if (n < min_neighbours) return;
    double um, vm, mu, mv;
    medians<radius>(get, n, um, vm);
    const Deviation<Get> dev = {get, um, vm};
    medians<radius>(dev, n, mu, mv);
    const double ru = fabs(uc - um) / (mu + eps);
    const double rv = fabs(vc - vm) / (mv + eps);
    res = sqrt(ru * ru + rv * rv);
    keep = res <= threshold ? 1 : 0;
}

template <class Get>
SID_HD_INLINE void filter_node(const Get &get, int radius, double uc, double vc, double eps, double threshold, int min_neighbours,
                               uint8_t &keep, double &res)
{
    if (radius == 1) filter_node_r<1>(get, uc, vc, eps, threshold, min_neighbours, keep, res);
    else filter_node_r<2>(get, uc, vc, eps, threshold, min_neighbours, keep, res);
}

// usable node of the filter: valid (or no mask) and finite u, v
SID_HD_INLINE bool usable_uv(const uint8_t *valid, int64_t k, double u, double v)
{
    return (!valid || valid[k] != 0) && isfinite(u) && isfinite(v);
}

// ---------------------------------------------------------------- gap filling and smoothing
// One candidate of one fill pass: `get` gives the neighbours that count in this pass (a generation below the pass, finite
// values) and NaN in both for every other node.  True when the node is filled: uf, vf = the medians of the neighbours, + 0.0
// (rank selection may pick either of two tied signed zeros; the sum is +0.0 for both).
template <int radius, class Get>
SID_HD_INLINE bool fill_node_r(const Get &get, int min_neighbours, double &uf, double &vf)
{
    int n = 0;
#pragma unroll
    for (int di = -radius; di <= radius; ++di)
#pragma unroll
        for (int dj = -radius; dj <= radius; ++dj) {
            if (di == 0 && dj == 0) continue;
            double a, b;
            get(di, dj, a, b);
            n += a == a;
        }
    if (n < min_neighbours) return false;                          // (min_neighbours >= 1: a median has n >= 1 values)
    double um, vm;
    medians<radius>(get, n, um, vm);
    uf = um + 0.0;
    vf = vm + 0.0;
    return true;
}

template <class Get>
SID_HD_INLINE bool fill_node(const Get &get, int radius, int min_neighbours, double &uf, double &vf)
{
    return radius == 1 ? fill_node_r<1>(get, min_neighbours, uf, vf) : fill_node_r<2>(get, min_neighbours, uf, vf);
}

// The weight table of the smoothing, row-major (2 radius + 1)^2, by value: a kernel argument, read with static indices
struct Weights { double w[25]; };

// Normalised convolution at one node: `get` gives the usable nodes, the centre at (0, 0) included, NaN in both elsewhere.
template <int radius, class Get>
SID_HD_INLINE void smooth_node_r(const Get &get, const Weights &wt, double &us, double &vs)
{
    us = NAN;
    vs = NAN;
    double a, b;
    get(0, 0, a, b);
    if (!(a == a)) return;
    double sw = 0.0, su = 0.0, sv = 0.0;
#pragma unroll
    for (int di = -radius; di <= radius; ++di)
#pragma unroll
        for (int dj = -radius; dj <= radius; ++dj) {
            get(di, dj, a, b);
            if (!(a == a)) continue;
            const double w = wt.w[(di + radius) * (2 * radius + 1) + (dj + radius)];
            sw = sw + w;
            su = su + w * a;
            sv = sv + w * b;
        }
    us = su / sw;
    vs = sv / sw;
}

template <class Get>
SID_HD_INLINE void smooth_node(const Get &get, int radius, const Weights &wt, double &us, double &vs)
{
    if (radius == 1) smooth_node_r<1>(get, wt, us, vs);
    else smooth_node_r<2>(get, wt, us, vs);
}

}  // namespace sid_grid

#endif
