/* sid_grid.h - C ABI of the steps between a grid of drift vectors and a deformation map on MI355X (gfx950): an outlier
 * filter, the replacement of what it rejected, a smoothing, and the deformation on the grid's own triangles.  Not the
 * reference's: it has no filter beyond a threshold on r * h, replaces and smooths nothing, and triangulates with Qhull.  All
 * steps work on the 2-D grids as get_drift_PM returns them, NaN where there is no result.
 * DESIGN.md sections 19 and 23; NumPy restatements: tests/grid_spec.py, tests/grid_fill_spec.py.
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
 *   fill          Replaces what the filter rejected (NumPy restatement: tests/grid_fill_spec.py).  `domain` is
 *                 uint8 [rows][cols] like `valid` (0 = never fill the node) and may be NULL.  Generation 0 = the filter's usable
 *                 nodes: u_out, v_out = the inputs bit for bit, gen = 0.  Pass p = 1..max_passes: the candidates are the nodes
 *                 without a generation that have (domain == NULL or domain != 0); a candidate's N = the nodes of its
 *                 (2 radius + 1)^2 window, centre excluded, clipped at the edges, that have a generation in 0..p-1 and finite
 *                 u_out, v_out.  With |N| >= min_neighbours: u_out = median(u_N) + 0.0, v_out = median(v_N) + 0.0, gen = p (the
 *                 filter's median; the sum makes a zero +0.0 whichever of two tied signed zeros the selection picked).  A pass
 *                 reads only generations below its own (Jacobi order).  Nodes never filled: NaN, NaN, gen = -1.  A pass that
 *                 fills nothing ends the process: later passes are no-ops.  gen is int32; max_passes is in 1..256.
 *   smooth        Normalised convolution over the usable nodes.  `weights` is a HOST array [2 radius + 1][2 radius + 1] in both
 *                 entry points (it is checked, and travels as a kernel argument): every entry finite and >= 0, the centre > 0.
 *                 For a usable node: sw = su = sv = 0.0; for di = -radius..radius, for dj = -radius..radius, in that order,
 *                 for a usable node (row + di, col + dj) inside the grid, the centre included, with w = weights[di + radius]
 *                 [dj + radius]: sw = sw + w ; su = su + w * u ; sv = sv + w * v.  u_out = su / sw, v_out = sv / sw.  Unusable
 *                 nodes: NaN in both.
 *
 * Every output element is written; callers clear nothing.  rows * cols = 0, rows < 2 or cols < 2 are valid calls (the
 * deformation then writes nothing).  The outputs of fill and smooth may not overlap their inputs or each other
 * (SID_PM_ERR_ARG): other nodes read the inputs while a node's result is written.  Returns 0, or a negative SID_PM_ERR_* code of sid_pm.h: SID_PM_ERR_ARG for a null pointer,
 * negative sizes, eps or threshold not finite or <= 0, radius outside 1..2, min_neighbours outside 1..(2 radius + 1)^2 - 1, an
 * unknown diagonal code, max_passes outside 1..256, a weight that is not finite or negative, a centre weight that is not > 0,
 * overlapping inputs and outputs; SID_PM_ERR_UNSUPPORTED for rows * cols >= 2^31.  All of these are found before any device call.
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
int sid_grid_fill(int device, const double *u, const double *v, const uint8_t *valid, const uint8_t *domain, int64_t rows,
                  int64_t cols, int radius, int min_neighbours, int max_passes, double *u_out, double *v_out, int32_t *gen);
int sid_grid_smooth(int device, const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols,
                    const double *weights, int radius, double *u_out, double *v_out);

/* Device pointers in and out, on the current HIP device, work queued on `hip_stream` (a hipStream_t; may be NULL).  The call
 * allocates nothing, copies nothing and waits for nothing. */
int sid_grid_filter_device(const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols,
                           double eps, double threshold, int radius, int min_neighbours, uint8_t *keep, double *res,
                           void *hip_stream);
int sid_grid_deformation_device(const double *x, const double *y, const double *u, const double *v, const uint8_t *valid,
                                int64_t rows, int64_t cols, int diagonal,
                                double *e1, double *e2, double *e3, double *a, double *p, int32_t *t, void *hip_stream);
/* max_passes launches, one per pass, all of them queued: nothing comes back to the host to end the series early. */
int sid_grid_fill_device(const double *u, const double *v, const uint8_t *valid, const uint8_t *domain, int64_t rows, int64_t cols,
                         int radius, int min_neighbours, int max_passes, double *u_out, double *v_out, int32_t *gen,
                         void *hip_stream);
/* `weights` is a host pointer here as well. */
int sid_grid_smooth_device(const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols,
                           const double *weights, int radius, double *u_out, double *v_out, void *hip_stream);

const char *sid_grid_last_error(void);
/* Free the grow-only device scratch block of `device` (every device: -1).  No call on that device may be in flight. */
int sid_grid_release(int device);

#ifdef __cplusplus
}
#endif
#endif
