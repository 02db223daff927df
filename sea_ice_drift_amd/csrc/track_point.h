// track_point.h - the per-cell and per-point steps of include/sid_track.h, one source for the kernels of
// track.hip and for their host instance (device = -1).  Triangles, edges and the interpolant are warp_pixel.h's own functions:
// a point at a pixel centre gets the image warp's answer because it runs the image warp's arithmetic.  Every float64
// operation is one IEEE rounding in the order of tests/track_spec.py (-ffp-contract=off on both sides).
#ifndef SID_TRACK_POINT_H
#define SID_TRACK_POINT_H

#include <math.h>
#include <stdint.h>

#include "track_bucket.h"
#include "warp_pixel.h"

namespace sid_track {

enum { kClosed = 1 };                                  // SID_TRACK_CLOSED of sid_track.h
enum { kBruteCells = 64 };                             // SID_TRACK_BRUTE_CELLS

using sid_warp::Cell;
using sid_warp::Nodes;
using sid_warp::Tri;

// The points a cell is examined for, xl <= px <= xh and yl <= py <= yh; no point at all: xl > xh
struct Box {
    double xl, xh, yl, yh;
};

// The cells a bucket sends its points to: rows i_lo..i_hi and columns j_lo..j_hi of cells; none: i_lo > i_hi
struct Rect {
    int32_t i_lo, i_hi, j_lo, j_hi;
};

SID_HD_INLINE Box no_box() { const Box b = {INFINITY, -INFINITY, INFINITY, -INFINITY}; return b; }
SID_HD_INLINE Rect no_rect() { const Rect r = {0x7fffffff, -1, 0x7fffffff, -1}; return r; }

SID_HD_INLINE void merge(Box &a, const Box &b)
{
    a.xl = fmin(a.xl, b.xl); a.xh = fmax(a.xh, b.xh);
    a.yl = fmin(a.yl, b.yl); a.yh = fmax(a.yh, b.yh);
}

// The extent of cell k (the warp's box without the clip), no_box() for a cell with fewer than three usable nodes
SID_HD_INLINE Box cell_box(const Nodes &g, int64_t k)
{
    double X[4], Y[4], XS[4], YS[4];
    int32_t ids[4];
    const unsigned usable = sid_warp::ring(g, k, X, Y, XS, YS, ids);
    Box b;
    return sid_warp::extent(X, Y, usable, b.xl, b.xh, b.yl, b.yh) ? b : no_box();
}

SID_HD_INLINE bool examined(const Box &b, double px, double py)
{
    return b.xl <= px && px <= b.xh && b.yl <= py && py <= b.yh;
}

// Cell k = i across + j with the box `b` enters the rectangle of every bucket its box touches.  `lower(p, v)` and
// `raise(p, v)` make *p the minimum / maximum of itself and v: atomics on the device, plain code on the host.
template <class Lower, class Raise>
SID_HD_INLINE void enter(const Box &b, int64_t k, int64_t across, const Axis &ax, const Axis &ay, Rect *rects, Lower lower, Raise raise)
{
    if (!(b.xl <= b.xh)) return;
    const int32_t i = (int32_t)(k / across), j = (int32_t)(k - (int64_t)i * across);
    const int32_t bx0 = bucket(ax, b.xl), bx1 = bucket(ax, b.xh), by0 = bucket(ay, b.yl), by1 = bucket(ay, b.yh);
    for (int32_t by = by0; by <= by1; ++by)
        for (int32_t bx = bx0; bx <= bx1; ++bx) {
            Rect &r = rects[(int64_t)by * ax.n + bx];
            lower(&r.i_lo, i); raise(&r.i_hi, i);
            lower(&r.j_lo, j); raise(&r.j_hi, j);
        }
}

// 2: triangle `t` owns the point (inside all three edges, the warp's half-open rule); 1: it only has it closed (Ed >= 0 on all
// three); 0: neither
SID_HD_INLINE int classify(const Tri &t, double px, double py)
{
    const double d0 = sid_warp::edge_side(t.e0, px, py), d1 = sid_warp::edge_side(t.e1, px, py), d2 = sid_warp::edge_side(t.e2, px, py);
    const bool i0 = d0 > 0.0 || (d0 == 0.0 && t.e0.tie), i1 = d1 > 0.0 || (d1 == 0.0 && t.e1.tie), i2 = d2 > 0.0 || (d2 == 0.0 && t.e2.tie);
    if (i0 && i1 && i2) return 2;
    return d0 >= 0.0 && d1 >= 0.0 && d2 >= 0.0 ? 1 : 0;
}

SID_HD_INLINE double quiet(double v) { return v == v ? v : __builtin_nan(""); }

// What a point has found so far: its owner (the walk ends), or the first triangle that has it closed
struct Found {
    double sx, sy;
    int64_t tri;
};

// The triangles of the examined cell k in slot order.  True when one owns the point: `own` is the result.  Else `shut` keeps
// the first triangle (over the whole walk) that has the point closed, when the caller wants one.
SID_HD_INLINE bool visit(const Nodes &g, int64_t k, double px, double py, bool closed, Found &own, Found &shut)
{
    Cell cs;
    const unsigned usable = sid_warp::ring(g, k, cs.X, cs.Y, cs.XS, cs.YS, cs.ids);
    sid_grid::split(cs.X, cs.Y, usable, g.diagonal, cs.ta, cs.tb, cs.tc);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        Tri t;
        if (!sid_warp::setup_tri(cs, s, t)) continue;
        const int c = classify(t, px, py);
        if (c == 2) {
            sid_warp::position(t, px, py, own.sx, own.sy);
            own.tri = 2 * k + s;
            return true;
        }
        if (c == 1 && closed && shut.tri < 0) {
            sid_warp::position(t, px, py, shut.sx, shut.sy);
            shut.tri = 2 * k + s;
        }
    }
    return false;
}

// One point.  `axes` = the two axes of the bucket grid (x, then y) and `rects` its rectangles, or axes == nullptr: every cell.
// `boxes` holds cell_box of every cell.  Cells are visited in ascending number, so the first owner is the lowest-numbered one.
SID_HD_INLINE void point(const Nodes &g, const Box *boxes, const Axis *axes, const Rect *rects, unsigned flags, double px, double py,
                         double &sx, double &sy, int32_t &tri)
{
    sx = sy = __builtin_nan("");
    tri = -1;
    if (!isfinite(px) || !isfinite(py) || g.rows < 2 || g.cols < 2) return;
    Rect r = {0, (int32_t)(g.rows - 2), 0, (int32_t)(g.cols - 2)};
    if (axes) r = rects[(int64_t)bucket(axes[1], py) * axes[0].n + bucket(axes[0], px)];
    const int64_t across = g.cols - 1;
    Found own = {0.0, 0.0, -1}, shut = {0.0, 0.0, -1};
    bool done = false;
    for (int64_t i = r.i_lo; i <= r.i_hi && !done; ++i)
        for (int64_t j = r.j_lo; j <= r.j_hi && !done; ++j) {
            const int64_t k = i * across + j;
            if (examined(boxes[k], px, py)) done = visit(g, k, px, py, (flags & kClosed) != 0, own, shut);
        }
    const Found &f = done ? own : shut;
    if (f.tri < 0) return;
    sx = quiet(f.sx);
    sy = quiet(f.sy);
    tri = (int32_t)f.tri;
}

}  // namespace sid_track

#endif
