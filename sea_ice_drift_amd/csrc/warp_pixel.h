// warp_pixel.h - the per-cell constants and the per-pixel arithmetic of include/sid_warp.h, one source
// for the kernels of warp.hip and for their host instance (device = -1).  Every float64 operation is one IEEE rounding in the
// order of tests/warp_spec.py (-ffp-contract=off on both sides).
#ifndef SID_WARP_PIXEL_H
#define SID_WARP_PIXEL_H

#include <math.h>
#include <stdint.h>

#include "grid_cell.h"

namespace sid_warp {

enum { kU8 = 0, kF32 = 1, kKeepZero = 1 };             // SID_WARP_U8, SID_WARP_F32, SID_WARP_KEEP_ZERO of sid_warp.h
enum { kTileRows = 16, kTileCols = 64 };              // SID_WARP_TILE_ROWS, SID_WARP_TILE_COLS

// The node grids of a call
struct Nodes {
    const double *x, *y, *xs, *ys;
    const uint8_t *valid;
    int64_t rows, cols;
    int diagonal;
};

// The images of a call
struct Images {
    const void *src;
    int64_t rows_s, cols_s, src_stride;
    int64_t rows_o, cols_o;
    int order;
    unsigned flags;
    void *out;
    int64_t out_stride;
    uint8_t *covered;
    float *map_x, *map_y;
};

// One edge p -> q of a triangle: the lower-numbered endpoint, the vector to the other one, whether the edge runs from the
// higher-numbered node (E changes sign) and whether a pixel on it is inside
struct Edge {
    double lox, loy, ex, ey;
    bool flip, tie;
};

// One triangle (a, b, c), counter-clockwise: its edges a -> b, b -> c, c -> a, then what the source position needs
struct Tri {
    Edge e0, e1, e2;
    double xa, ya, bx, by, cx, cy, det;               // b - a, c - a, their cross product
    double sxa, sxb, sxc, sya, syb, syc;              // xs_a, xs_b - xs_a, xs_c - xs_a; the same of ys
};

// One cell: its ring in both frames, its triangle slots before orientation (ta[s] = -1: none) and the pixels it is examined
// over (rows r_lo..r_hi, columns c_lo..c_hi, never empty)
struct Cell {
    double X[4], Y[4], XS[4], YS[4];
    int32_t ids[4];
    int ta[2], tb[2], tc[2];
    int64_t r_lo, r_hi, c_lo, c_hi;
};

SID_HD_INLINE int32_t pick_id(const int32_t q[4], int k) { return k == 0 ? q[0] : k == 1 ? q[1] : k == 2 ? q[2] : q[3]; }

// The ring A, B, E, D of cell k = i (cols - 1) + j: positions in both frames, flat node numbers; returns the usable bits
SID_HD_INLINE unsigned ring(const Nodes &g, int64_t k, double X[4], double Y[4], double XS[4], double YS[4], int32_t ids[4])
{
    const int64_t i = k / (g.cols - 1), j = k - i * (g.cols - 1), A = i * g.cols + j;
    ids[0] = (int32_t)A; ids[1] = (int32_t)(A + 1); ids[2] = (int32_t)(A + g.cols + 1); ids[3] = (int32_t)(A + g.cols);
    unsigned usable = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t n = ids[q];
        X[q] = g.x[n]; Y[q] = g.y[n]; XS[q] = g.xs[n]; YS[q] = g.ys[n];
        if ((!g.valid || g.valid[n] != 0) && isfinite(X[q]) && isfinite(Y[q]) && isfinite(XS[q]) && isfinite(YS[q])) usable |= 1u << q;
    }
    return usable;
}

// floor(min) - 1 .. ceil(max) + 1 of a cell's usable nodes, per axis, before any clip (track_point.h examines a cell for the
// points in there).  False when the cell has fewer than three usable nodes.
SID_HD_INLINE bool extent(const double X[4], const double Y[4], unsigned usable, double &cl, double &ch, double &rl, double &rh)
{
    const int n = (int)(usable & 1) + (int)((usable >> 1) & 1) + (int)((usable >> 2) & 1) + (int)((usable >> 3) & 1);
    if (n < 3) return false;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (usable & (1u << q)) {
            x0 = fmin(x0, X[q]); x1 = fmax(x1, X[q]);
            y0 = fmin(y0, Y[q]); y1 = fmax(y1, Y[q]);
        }
    cl = floor(x0) - 1.0; ch = ceil(x1) + 1.0; rl = floor(y0) - 1.0; rh = ceil(y1) + 1.0;
    return true;
}

// The pixels a cell is examined over: its extent clipped to the output.  False when the cell has fewer than three usable nodes
// or the box is empty.
SID_HD_INLINE bool box(const double X[4], const double Y[4], unsigned usable, int64_t rows_o, int64_t cols_o,
                       int64_t &r_lo, int64_t &r_hi, int64_t &c_lo, int64_t &c_hi)
{
    double cl, ch, rl, rh;
    if (!extent(X, Y, usable, cl, ch, rl, rh)) return false;
    if (cl < 0.0) cl = 0.0;
    if (rl < 0.0) rl = 0.0;
    if (ch > (double)(cols_o - 1)) ch = (double)(cols_o - 1);
    if (rh > (double)(rows_o - 1)) rh = (double)(rows_o - 1);
    if (!(cl <= ch) || !(rl <= rh)) return false;
    c_lo = (int64_t)cl; c_hi = (int64_t)ch; r_lo = (int64_t)rl; r_hi = (int64_t)rh;
    return true;
}

// Work items (tiles of kTileRows x kTileCols pixels, anchored at (r_lo, c_lo)) of a box
SID_HD_INLINE int64_t tiles_across(int64_t c_lo, int64_t c_hi) { return (c_hi - c_lo) / kTileCols + 1; }
SID_HD_INLINE int64_t tiles(int64_t r_lo, int64_t r_hi, int64_t c_lo, int64_t c_hi)
{
    return ((r_hi - r_lo) / kTileRows + 1) * tiles_across(c_lo, c_hi);
}

// Edge p -> q of a triangle (ring positions)
SID_HD_INLINE void edge(const Cell &cs, int p, int q, Edge &e)
{
    const double xp = sid_grid::pick(cs.X, p), yp = sid_grid::pick(cs.Y, p), xq = sid_grid::pick(cs.X, q), yq = sid_grid::pick(cs.Y, q);
    const bool plo = pick_id(cs.ids, p) < pick_id(cs.ids, q);
    e.lox = plo ? xp : xq;
    e.loy = plo ? yp : yq;
    e.ex = (plo ? xq : xp) - e.lox;
    e.ey = (plo ? yq : yp) - e.loy;
    e.flip = !plo;
    const double dx = xq - xp, dy = yq - yp;
    e.tie = dy > 0.0 || (dy == 0.0 && dx > 0.0);
}

// What the triangles of cell k share.  False when the cell has no pixel to examine.
SID_HD_INLINE bool setup(const Nodes &g, int64_t k, int64_t rows_o, int64_t cols_o, Cell &cs)
{
    const unsigned usable = ring(g, k, cs.X, cs.Y, cs.XS, cs.YS, cs.ids);
    if (!box(cs.X, cs.Y, usable, rows_o, cols_o, cs.r_lo, cs.r_hi, cs.c_lo, cs.c_hi)) return false;
    sid_grid::split(cs.X, cs.Y, usable, g.diagonal, cs.ta, cs.tb, cs.tc);
    return true;
}

// What the pixels of the triangle in slot s (a constant) share.  False when the slot holds no triangle that can own a pixel.
SID_HD_INLINE bool setup_tri(const Cell &cs, int s, Tri &t)
{
    if (cs.ta[s] < 0) return false;
    const int a = cs.ta[s];
    int b = cs.tb[s], c = cs.tc[s];
    t.xa = sid_grid::pick(cs.X, a); t.ya = sid_grid::pick(cs.Y, a);
    const double cr = (sid_grid::pick(cs.X, b) - t.xa) * (sid_grid::pick(cs.Y, c) - t.ya)
                    - (sid_grid::pick(cs.X, c) - t.xa) * (sid_grid::pick(cs.Y, b) - t.ya);
    if (cr < 0.0) { const int w = b; b = c; c = w; }
    t.bx = sid_grid::pick(cs.X, b) - t.xa; t.by = sid_grid::pick(cs.Y, b) - t.ya;
    t.cx = sid_grid::pick(cs.X, c) - t.xa; t.cy = sid_grid::pick(cs.Y, c) - t.ya;
    t.det = t.bx * t.cy - t.cx * t.by;
    if (!(t.det > 0.0)) return false;
    edge(cs, a, b, t.e0);
    edge(cs, b, c, t.e1);
    edge(cs, c, a, t.e2);
    t.sxa = sid_grid::pick(cs.XS, a); t.sxb = sid_grid::pick(cs.XS, b) - t.sxa; t.sxc = sid_grid::pick(cs.XS, c) - t.sxa;
    t.sya = sid_grid::pick(cs.YS, a); t.syb = sid_grid::pick(cs.YS, b) - t.sya; t.syc = sid_grid::pick(cs.YS, c) - t.sya;
    return true;
}

// Ed of sid_warp.h: positive on the triangle's side of the edge
SID_HD_INLINE double edge_side(const Edge &e, double px, double py)
{
    const double E = e.ex * (py - e.loy) - e.ey * (px - e.lox);
    return e.flip ? -E : E;
}

SID_HD_INLINE bool inside(const Edge &e, double px, double py)
{
    const double Ed = edge_side(e, px, py);
    return Ed > 0.0 || (Ed == 0.0 && e.tie);
}

SID_HD_INLINE bool owns(const Tri &t, double px, double py)
{
    const bool i0 = inside(t.e0, px, py), i1 = inside(t.e1, px, py), i2 = inside(t.e2, px, py);
    return i0 && i1 && i2;
}

// The linear interpolant of triangle `t` at (px, py), whoever owns the point (track_point.h asks on its own)
SID_HD_INLINE void position(const Tri &t, double px, double py, double &sx, double &sy)
{
    const double ax = px - t.xa, ay = py - t.ya;
    const double l1 = (ax * t.cy - t.cx * ay) / t.det;
    const double l2 = (t.bx * ay - ax * t.by) / t.det;
    sx = t.sxa + l1 * t.sxb + l2 * t.sxc;
    sy = t.sya + l1 * t.syb + l2 * t.syc;
}

// The source position of pixel centre (px, py) when triangle `t` owns it; false (sx, sy untouched) when it does not
SID_HD_INLINE bool source(const Tri &t, double px, double py, double &sx, double &sy)
{
    if (!owns(t, px, py)) return false;
    position(t, px, py, sx, sy);
    return true;
}

// Where a source position reads the image: in range or not, the element offset of the tap (order 0) or of p00 (order 1), the
// steps from p00 to p01 and to p10 (0 on the last column / row) and the two weights
struct Tap {
    bool in;
    int64_t o00, down;
    int right;
    double fx, fy;
};

SID_HD_INLINE void locate(const Images &im, double sx, double sy, Tap &tp)
{
    const double cmax = (double)(im.cols_s - 1), rmax = (double)(im.rows_s - 1);
    tp.in = false; tp.o00 = 0; tp.down = 0; tp.right = 0; tp.fx = 0.0; tp.fy = 0.0;
    if (im.order == 0) {
        const double jc = rint(sx), jr = rint(sy);
        if (!(jc >= 0.0 && jc <= cmax && jr >= 0.0 && jr <= rmax)) return;
        tp.in = true;
        tp.o00 = (int64_t)jr * im.src_stride + (int64_t)jc;
        return;
    }
    if (!(sx >= 0.0 && sx <= cmax && sy >= 0.0 && sy <= rmax)) return;
    tp.in = true;
    const double c0 = floor(sx), r0 = floor(sy);
    tp.fx = sx - c0; tp.fy = sy - r0;
    const int64_t ic0 = (int64_t)c0, ir0 = (int64_t)r0;
    tp.o00 = ir0 * im.src_stride + ic0;
    tp.right = ic0 + 1 < im.cols_s ? 1 : 0;
    tp.down = ir0 + 1 < im.rows_s ? im.src_stride : 0;
}

// The taps themselves: q[0] alone for order 0; p00, p01, p10, p11 for order 1 (zeros when out of range or without an image)
template <class T>
SID_HD_INLINE void fetch(const Images &im, const Tap &tp, T q[4])
{
    const T *src = static_cast<const T *>(im.src);
    q[0] = q[1] = q[2] = q[3] = T(0);
    if (!tp.in || !src) return;
    q[0] = src[tp.o00];
    if (im.order == 0) return;
    q[1] = src[tp.o00 + tp.right];
    q[2] = src[tp.o00 + tp.down];
    q[3] = src[tp.o00 + tp.down + tp.right];
}

SID_HD_INLINE uint8_t to_pixel(double v, uint8_t) { return (uint8_t)rint(v); }
SID_HD_INLINE float to_pixel(double v, float) { return (float)v; }

template <class T>
SID_HD_INLINE T combine(const Images &im, const Tap &tp, const T q[4])
{
    if (im.order == 0) return q[0];
    const double p00 = (double)q[0], p01 = (double)q[1], p10 = (double)q[2], p11 = (double)q[3];
    const double fx = tp.fx, fy = tp.fy, wx = 1.0 - fx, wy = 1.0 - fy;
    const double v = wy * (wx * p00 + fx * p01) + fy * (wx * p10 + fx * p11);
    // 1 - fx and 1 - fy are never zero (fx, fy < 1): the tap p00 always counts
    if ((im.flags & kKeepZero)
        && (p00 == 0.0 || (fx != 0.0 && p01 == 0.0) || (fy != 0.0 && p10 == 0.0) || (fx != 0.0 && fy != 0.0 && p11 == 0.0)))
        return T(0);
    return to_pixel(v, T());
}

SID_HD_INLINE float map_value(double s)
{
    return s == s ? (float)s : __builtin_nanf("");
}

// The outputs of an owned pixel (an unowned one keeps what the fill wrote)
template <class T>
SID_HD_INLINE void store(const Images &im, int64_t r, int64_t c, double sx, double sy, const Tap &tp, T val)
{
    const int64_t o = r * im.cols_o + c;
    if (im.map_x) im.map_x[o] = map_value(sx);
    if (im.map_y) im.map_y[o] = map_value(sy);
    if (!tp.in) return;
    if (im.out) static_cast<T *>(im.out)[r * im.out_stride + c] = val;
    if (im.covered) im.covered[o] = 1;
}

// Pixel (r, c) of the output as triangle `t` sees it, all steps in one go (the host instance; the kernel runs the same steps
// on several rows at a time)
template <class T>
SID_HD_INLINE void pixel(const Tri &t, const Images &im, int64_t r, int64_t c)
{
    double sx, sy;
    if (!source(t, (double)c, (double)r, sx, sy)) return;
    Tap tp;
    T q[4];
    locate(im, sx, sy, tp);
    fetch<T>(im, tp, q);
    store<T>(im, r, c, sx, sy, tp, combine<T>(im, tp, q));
}

}  // namespace sid_warp

#endif
