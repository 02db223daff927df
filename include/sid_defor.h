/* sid_defor.h - C ABI of the sea-ice deformation on MI355X (gfx950): the reference's libdefor (sea_ice_drift v0.7.1,
 * libdefor.py) on a given triangulation.
 *
 * Replaces, element for element:
 *
 *   sid_defor_triangulation   libdefor.get_deformation_on_triangulation(x, y, u, v, t): the corners of every triangle
 *                             t[k] = (i0, i1, i2), side vectors corner1 - corner0, corner2 - corner1, corner0 - corner2,
 *                             side lengths (hypot), perimeter p = (s0 + s1) + s2, Heron's area
 *                             a = sqrt(((h (h - s0)) (h - s1)) (h - s2)), h = p / 2, then the element deformation below.
 *   sid_defor_elems           libdefor.get_deformation_elems(x, y, u, v, a): contour integrals over the three sides,
 *                             (i0, i1) = (1, 0), (2, 1), (0, 2):  ux = 0 + sum (u[i0] + u[i1]) (y[i0] - y[i1]),
 *                             uy = 0 - sum (u[i0] + u[i1]) (x[i0] - x[i1]) (vx, vy: the same with v), each divided by 2 a;
 *                             e1 = ux + vy, e2 = sqrt((ux - vy)^2 + (uy + vx)^2), e3 = vx - uy.
 *
 * Every operation is one IEEE float64 rounding in the order written (NumPy's order; built with -ffp-contract=off); the
 * side lengths use a restatement of glibc's hypot, which NumPy's float64 np.hypot calls.  DESIGN.md section 15.
 *
 * Arrays: x, y, u, v of the nodes [n]; t [m][3] node indices (int32, or int64 with t_int64 = 1), NumPy's indexing:
 * an index i < 0 stands for n + i, and one outside [-n, n) is SID_DEFOR_ERR_INDEX (the outputs are then undefined).
 * For sid_defor_elems: x, y, u, v [3][m] (row k: corner k of every element), a [m].  Outputs [m] each (structure of arrays).
 * m = 0 is a valid call that does nothing.  0 on success, a negative SID_PM_ERR_* code (sid_pm.h) or SID_DEFOR_ERR_INDEX
 * otherwise; sid_defor_last_error() has the message.
 */
#ifndef SID_DEFOR_H
#define SID_DEFOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SID_DEFOR_ERR_INDEX -32   /* an index of t lies outside [-n, n) */

/* Host buffers in, host buffers out; `device` is the HIP device index.  The call returns when the outputs are written. */
int sid_defor_triangulation(int device, const double *x, const double *y, const double *u, const double *v, int64_t n,
                            const void *t, int t_int64, int64_t m,
                            double *e1, double *e2, double *e3, double *a, double *p);
int sid_defor_elems(int device, const double *x, const double *y, const double *u, const double *v, const double *a, int64_t m,
                    double *e1, double *e2, double *e3);

/* Device pointers in and out, on the current HIP device, work queued on `hip_stream` (a hipStream_t; may be NULL).  No data
 * crosses to the host; the call waits for the stream once, to read the out-of-range flag of the indices (4 bytes). */
int sid_defor_triangulation_device(const double *x, const double *y, const double *u, const double *v, int64_t n,
                                   const void *t, int t_int64, int64_t m,
                                   double *e1, double *e2, double *e3, double *a, double *p, void *hip_stream);
int sid_defor_elems_device(const double *x, const double *y, const double *u, const double *v, const double *a, int64_t m,
                           double *e1, double *e2, double *e3, void *hip_stream);

/* out[i] = hypot(x[i], y[i]) as the kernels evaluate it: on HIP device `device`, or with the same source on the host
 * (device = -1).  Host buffers.  The float64 counterpart of sid_pm_debug_hypot_selftest: tests compare it with libm. */
int sid_defor_debug_hypot(int device, const double *x, const double *y, int64_t n, double *out);

const char *sid_defor_last_error(void);
/* Free the grow-only device scratch block and the index flag of `device` (every device: -1).  No call on that device may be
 * in flight. */
int sid_defor_release(int device);

#ifdef __cplusplus
}
#endif
#endif
