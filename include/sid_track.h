/* sid_track.h - C ABI of the point map of a drift grid on MI355X (gfx950): where do arbitrary points of one frame lie in the
 * other?  Not the reference's.  It is the field of sid_warp.h - a grid of nodes known in two frames, (x, y) and (xs, ys), cut
 * into the triangles of sid_grid.h, linear inside each - evaluated at scattered points instead of at every pixel of an output.
 * DESIGN.md section 25; NumPy restatement: tests/track_spec.py.
 *
 * Node grids x, y, xs, ys, `valid` and `diagonal` are exactly those of sid_warp.h: row-major float64 [grid_rows][grid_cols] in
 * pixel units (x = column, y = row), valid uint8 or NULL, a node USABLE when (valid == NULL or valid != 0) and x, y, xs, ys
 * are finite.  Points px, py are float64 [n] in the frame of (x, y).  Every float64 operation below is one IEEE rounding in
 * the order written (built with -ffp-contract=off).
 *
 *   triangles   As in sid_warp.h: cell (i, j) has the number i (grid_cols - 1) + j and the ring A, B, E, D; four usable nodes
 *               give two triangles (slots 0, 1) by `diagonal`, three give one (slot 0), fewer none; (a, b, c) is made
 *               counter-clockwise; only a triangle with det = (xb-xa)(yc-ya) - (xc-xa)(yb-ya) > 0 can have a point.
 *   examined    A cell with at least three usable nodes is examined for the point (px, py) iff
 *                   floor(min) - 1 <= p <= ceil(max) + 1        on both axes (min, max over its usable nodes)
 *               compared as doubles: the box of sid_warp.h without the clip to an output.
 *   owner       For each directed edge p -> q of a -> b, b -> c, c -> a the warp's
 *                   E  = (x_hi - x_lo)(py - y_lo) - (y_hi - y_lo)(px - x_lo) ;  Ed = E if p is lo, else -E
 *                   inside the edge  iff  Ed > 0, or Ed == 0 and (dy > 0, or dy == 0 and dx > 0)
 *               (lo, hi by flat node number; dx = x_q - x_p, dy = y_q - y_p).  A triangle owns the point iff the point is inside
 *               all three edges.  Among the owning triangles of examined cells THE OWNER is the one with the lowest number
 *               2 cell + slot.  A mesh that does not fold has at most one; on a folded mesh the rule makes the result a
 *               function of the inputs alone, whatever the search.
 *   closed      With SID_TRACK_CLOSED: when no triangle owns the point, the lowest-numbered triangle of an examined cell with
 *               Ed >= 0 on all three edges has it.  (The half-open rule leaves the first column and the last row of nodes of a
 *               regular grid to nobody; this brings the rim of the mesh back, and nothing else: without the flag the results at
 *               pixel centres are the warp's, with it they are the warp's wherever the warp owns the pixel, and every point it
 *               adds has an edge with Ed == 0.)
 *   result      Of the triangle (a, b, c) that has the point, det as above:
 *                   l1 = ((px-xa)(yc-ya) - (xc-xa)(py-ya)) / det ;  l2 = ((xb-xa)(py-ya) - (px-xa)(yb-ya)) / det
 *                   sx = xs_a + l1 (xs_b - xs_a) + l2 (xs_c - xs_a) ;  sy = ys_a + l1 (ys_b - ys_a) + l2 (ys_c - ys_a)
 *               and tri = 2 cell + slot.  sx = sy = the quiet NaN 0x7ff8000000000000 and tri = -1 when no triangle has the point
 *               or px or py is not finite.  A sum that is not a number (overflow) is stored as that NaN too.
 *
 * Every element of sx, sy and tri is written; callers clear nothing.  `tri` may be NULL (not wanted).  n = 0, grid_rows < 2 and
 * grid_cols < 2 are valid calls (with n = 0 the point arrays are not looked at).
 * Returns 0, or a negative SID_PM_ERR_* code of sid_pm.h, found before any device call:
 *   SID_PM_ERR_ARG          a null node grid; n > 0 and px, py, sx or sy null; negative sizes; an unknown diagonal or flag; an
 *                           output overlapping an input or another output
 *   SID_PM_ERR_UNSUPPORTED  grid_rows * grid_cols >= 2^31; `tri` wanted with 2^30 cells or more (2 cell + slot is an int32)
 *
 * The search (csrc/track.hip, track_point.h, track_bucket.h) never reaches the result: one bucket per cell over the bounding
 * box of the cells' boxes, every bucket holding the index rectangle of the cells whose box touches it, every point walking
 * its bucket's rectangle in ascending cell number.  Grids of fewer than SID_TRACK_BRUTE_CELLS cells, and every grid when the
 * environment holds SID_TRACK_NO_GRID, look at every cell for every point instead.
 */
#ifndef SID_TRACK_H
#define SID_TRACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SID_TRACK_CLOSED 1u

/* grids with fewer cells than this run every (point, cell) pair; tests cross it */
#define SID_TRACK_BRUTE_CELLS 64

/* Host buffers in, host buffers out; `device` is the HIP device index.  The call returns when the outputs are written.
 * device = -1 runs the same source in a host loop, buckets included, without a GPU (for tests). */
int sid_track_points(int device, const double *x, const double *y, const double *xs, const double *ys, const uint8_t *valid,
                     int64_t grid_rows, int64_t grid_cols, int diagonal, uint32_t flags,
                     const double *px, const double *py, int64_t n, double *sx, double *sy, int32_t *tri);

/* Device pointers in and out, on the current HIP device, work queued on `hip_stream` (a hipStream_t; may be NULL).  The call
 * copies nothing to the host and waits for nothing, and allocates nothing beyond the module's grow-only scratch of that device
 * (48 bytes per grid cell and less than 34 KiB: a function of the grid's shape alone; it grows on the first call and when a larger grid
 * comes).  The scratch is one per device: calls on one device must be ordered among themselves (one stream, or events between
 * streams). */
int sid_track_points_device(const double *x, const double *y, const double *xs, const double *ys, const uint8_t *valid,
                            int64_t grid_rows, int64_t grid_cols, int diagonal, uint32_t flags,
                            const double *px, const double *py, int64_t n, double *sx, double *sy, int32_t *tri, void *hip_stream);

const char *sid_track_last_error(void);
/* Free the grow-only device scratch of `device` (every device: -1).  No call on that device may be in flight. */
int sid_track_release(int device);

#ifdef __cplusplus
}
#endif
#endif
