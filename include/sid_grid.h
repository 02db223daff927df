/* sid_grid.h - C ABI of the two steps between a grid of drift vectors and a deformation map on MI355X (gfx950): an outlier
 * filter and the deformation on the grid's own triangles.  Not the reference's: it has no filter beyond a threshold on r * h, and
 * triangulates with Qhull.  Both steps work on the 2-D grids as get_drift_PM returns them, NaN where there is no result.
 * DESIGN.md section 19; NumPy restatement: tests/grid_spec.py.
 *
 * Arrays are row-major [rows][cols], float64; `valid` is uint8 [rows][cols] (0 = leave the node out) and may be NULL.
 * A node is USABLE for the filter when (valid == NULL or valid != 0) and u, v are finite; for the deformation x and y must be
 * finite as well.  Every float64 operation below is one IEEE rounding in the order written (built with -ffp-contract=off).
 *
 *   filter        The normalised median test of PIV practice (Westerweel and Scarano 2005), one pass.  For a usable node, N = the
 *                 usable nodes of the (2 radius + 1)^2 window around it, centre excluded, clipped at the grid's edges.  With
 *                 fewer than min_neighbours of them: res = NaN, keep = 0.  Otherwise, median(s) of n sorted values being
 *                 s[(n-1)/2] for odd n and (s[n/2-1] + s[n/2]) / 2.0 for even n:
 *                     um = median(u_N) ; mu = median(|u_N - um|) ; ru = |u - um| / (mu + eps)     (rv: the same with v)
 *                     res = sqrt(ru * ru + rv * rv) ; keep = res <= threshold
 *                 Unusable nodes: res = NaN, keep = 0.  `eps` is the noise of a good vector, in the unit of u.
 *   deformation   Cell (i, j) has the nodes A = i cols + j, B = A + 1, D = A + cols, E = D + 1 (ring A, B, E, D) and two
 *                 triangle slots.  Four usable nodes: dm = (xE-xA)(xE-xA) + (yE-yA)(yE-yA), da = (xD-xB)(xD-xB) + (yD-yB)(yD-yB);
 *                 the anti split, slots (A, B, D), (B, E, D), for SID_GRID_DIAG_ANTI or for SID_GRID_DIAG_SHORTER with da < dm,
 *                 else the main split (A, B, E), (A, E, D).  Three usable nodes: slot 0 = those three in ring order.  Fewer: no
 *                 triangle.  Each triangle (a, b, c) with (xb-xa)(yc-ya) - (xc-xa)(yb-ya) < 0 has b and c swapped (counter-
 *                 clockwise, as matplotlib's).  Its e1, e2, e3, a, p are those of sid_defor_triangulation (sid_defor.h) on
 *                 (a, b, c).  Outputs [rows-1][cols-1][2] each, t [rows-1][cols-1][2][3] flat node numbers; a slot without a
 *                 triangle holds NaN and -1.
 *
 * Every output element is written; callers clear nothing.  rows * cols = 0, rows < 2 or cols < 2 are valid calls (the
 * deformation then writes nothing).  Returns 0, or a negative SID_PM_ERR_* code of sid_pm.h: SID_PM_ERR_ARG for a null pointer,
 * negative sizes, eps or threshold not finite or <= 0, radius outside 1..2, min_neighbours outside 1..(2 radius + 1)^2 - 1, an
 * unknown diagonal code; SID_PM_ERR_UNSUPPORTED for rows * cols >= 2^31.  All of these are found before any device call.
 */
#ifndef SID_GRID_H
#define SID_GRID_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SID_GRID_DIAG_SHORTER 0
#define SID_GRID_DIAG_MAIN    1
#define SID_GRID_DIAG_ANTI    2

/* workgroup tile of the filter kernel (rows x cols of nodes); tests straddle it */
#define SID_GRID_TILE_ROWS 8
#define SID_GRID_TILE_COLS 32

/* Host buffers in, host buffers out; `device` is the HIP device index.  The call returns when the outputs are written.
 * device = -1 runs the same source in a host loop, without a GPU (for tests). */
int sid_grid_filter(int device, const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols,
                    double eps, double threshold, int radius, int min_neighbours, uint8_t *keep, double *res);
int sid_grid_deformation(int device, const double *x, const double *y, const double *u, const double *v, const uint8_t *valid,
                         int64_t rows, int64_t cols, int diagonal,
                         double *e1, double *e2, double *e3, double *a, double *p, int32_t *t);

/* Device pointers in and out, on the current HIP device, work queued on `hip_stream` (a hipStream_t; may be NULL).  The call
 * allocates nothing, copies nothing and waits for nothing. */
int sid_grid_filter_device(const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols,
                           double eps, double threshold, int radius, int min_neighbours, uint8_t *keep, double *res,
                           void *hip_stream);
int sid_grid_deformation_device(const double *x, const double *y, const double *u, const double *v, const uint8_t *valid,
                                int64_t rows, int64_t cols, int diagonal,
                                double *e1, double *e2, double *e3, double *a, double *p, int32_t *t, void *hip_stream);

const char *sid_grid_last_error(void);
/* Free the grow-only device scratch block of `device` (every device: -1).  No call on that device may be in flight. */
int sid_grid_release(int device);

#ifdef __cplusplus
}
#endif
#endif
