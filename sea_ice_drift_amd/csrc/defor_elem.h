// defor_elem.h - the arithmetic of one deformation element (the reference's libdefor.py), one source for
// the kernels of defor.hip and drift_grid.hip and for the host instance of the latter.  Every operation is one IEEE float64
// rounding in NumPy's order (-ffp-contract=off on both sides).
#ifndef SID_DEFOR_ELEM_H
#define SID_DEFOR_ELEM_H

#include <math.h>

#include "defor_hypot.h"

#define SID_HD_INLINE SID_HD inline __attribute__((always_inline))

namespace sid_defor {

// libdefor.get_deformation_elems for one element: corners c = 0, 1, 2 of x, y, u, v and the area a.
// The sums start from Python's integer 0 (0 + first term, 0 - first term: a -0.0 term gives +0.0).
SID_HD_INLINE void elem(const double x[3], const double y[3], const double u[3], const double v[3], double a,
                        double &e1, double &e2, double &e3)
{
    double ux = 0.0, uy = 0.0, vx = 0.0, vy = 0.0;
    const int i0s[3] = {1, 2, 0}, i1s[3] = {0, 1, 2};
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int i0 = i0s[s], i1 = i1s[s];
        ux = ux + (u[i0] + u[i1]) * (y[i0] - y[i1]);
        uy = uy - (u[i0] + u[i1]) * (x[i0] - x[i1]);
        vx = vx + (v[i0] + v[i1]) * (y[i0] - y[i1]);
        vy = vy - (v[i0] + v[i1]) * (x[i0] - x[i1]);
    }
    const double a2 = 2.0 * a;
    ux = ux / a2; uy = uy / a2; vx = vx / a2; vy = vy / a2;
    e1 = ux + vy;
    const double d = ux - vy, s = uy + vx;
    e2 = sqrt(d * d + s * s);                  // ** 2 is x * x, ** 0.5 is sqrt in NumPy
    e3 = vx - uy;
}

// libdefor.get_deformation_on_triangulation for one triangle whose corners are gathered already: sides
// (np.diff(np.vstack([xt, xt[0]]), axis=0): corner1 - corner0, corner2 - corner1, corner0 - corner2), perimeter, Heron's
// area, then elem.
SID_HD_INLINE void triangle(const double xs[3], const double ys[3], const double us[3], const double vs[3],
                            double &e1, double &e2, double &e3, double &a, double &p)
{
    const double s0 = hypot64(xs[1] - xs[0], ys[1] - ys[0]);
    const double s1 = hypot64(xs[2] - xs[1], ys[2] - ys[1]);
    const double s2 = hypot64(xs[0] - xs[2], ys[0] - ys[2]);
    p = (s0 + s1) + s2;
    const double h = p / 2.0;
    a = sqrt(((h * (h - s0)) * (h - s1)) * (h - s2));
    elem(xs, ys, us, vs, a, e1, e2, e3);
}

}  // namespace sid_defor

#endif
