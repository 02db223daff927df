/* sid_warp.h - C ABI of the piecewise-affine warp of an image along a drift grid on MI355X (gfx950).  Not the reference's: it
 * has no resampling step.  A grid of nodes known in two frames - the destination's (x, y) and the source's (xs, ys) - is cut
 * into the triangles of sid_grid.h; inside a triangle the source position is the linear interpolant of its three nodes, the
 * field whose gradient sid_grid_deformation reports.  DESIGN.md section 21; NumPy restatement: tests/warp_spec.py.
 *
 * Node grids x, y, xs, ys are row-major float64 [grid_rows][grid_cols] in pixel units (x = column, y = row; an integer is a
 * pixel centre); `valid` is uint8 [grid_rows][grid_cols] (0 = leave the node out) and may be NULL.  A node is USABLE when
 * (valid == NULL or valid != 0) and x, y, xs, ys are finite.  Every float64 operation below is one IEEE rounding in the order
 * written (built with -ffp-contract=off).
 *
 *   triangles   Those of sid_grid.h on (x, y): cell (i, j) has the ring A, B, E, D; four usable nodes give two triangles by
 *               `diagonal` (a SID_GRID_DIAG_* code), three give one, fewer none; (a, b, c) with
 *               cr = (xb-xa)(yc-ya) - (xc-xa)(yb-ya) < 0 has b and c swapped.  A triangle with cr == 0 (or cr not a number)
 *               owns no pixel.
 *   ownership   Pixel (r, c) has the centre px = c, py = r.  For each directed edge p -> q of a -> b, b -> c, c -> a, with
 *               lo, hi its endpoints ordered by flat node number (row * grid_cols + column):
 *                   E  = (x_hi - x_lo)(py - y_lo) - (y_hi - y_lo)(px - x_lo) ;  Ed = E if p is lo, else -E
 *                   dx = x_q - x_p ; dy = y_q - y_p
 *                   inside the edge  iff  Ed > 0, or Ed == 0 and (dy > 0, or dy == 0 and dx > 0)
 *               The triangle owns the pixel iff it is inside all three edges.  Both triangles at a shared edge compute the
 *               same E, so one of them exactly has the pixel: a mesh whose cells do not fold is watertight and single-owner,
 *               pixel centres on nodes and edges included.  A cell is examined only over the pixels of
 *                   floor(min) - 1 .. ceil(max) + 1     (min, max over its usable nodes, per axis; clipped to the output)
 *               which holds every pixel its triangles can own unless rounding errors exceed a pixel.  Where triangles overlap
 *               (a folded mesh) a covered pixel gets the values of one of the covering triangles, unspecified which, and not
 *               necessarily the same one in every output.
 *   source      Of a pixel owned by (a, b, c), det = cr:
 *                   l1 = ((px-xa)(yc-ya) - (xc-xa)(py-ya)) / det ;  l2 = ((xb-xa)(py-ya) - (px-xa)(yb-ya)) / det
 *                   sx = xs_a + l1 (xs_b - xs_a) + l2 (xs_c - xs_a) ;  sy = ys_a + l1 (ys_b - ys_a) + l2 (ys_c - ys_a)
 *   sampling    order 0: jc = rint(sx), jr = rint(sy) (half to even); in range iff 0 <= jc <= cols_s - 1 and
 *               0 <= jr <= rows_s - 1, compared as doubles; the value is src[jr][jc].
 *               order 1: in range iff 0 <= sx <= cols_s - 1 and 0 <= sy <= rows_s - 1; c0 = floor(sx), r0 = floor(sy),
 *               fx = sx - c0, fy = sy - r0, c1 = min(c0 + 1, cols_s - 1), r1 = min(r0 + 1, rows_s - 1),
 *                   v = (1-fy)((1-fx) p00 + fx p01) + fy ((1-fx) p10 + fx p11)       in float64, p.. = src[r.][c.]
 *               uint8 takes rint(v), float32 the cast of v.  With SID_WARP_KEEP_ZERO (uint8, order 1; ignored with order 0):
 *               if a tap whose two weights are both non-zero holds 0 (the project's invalid value), the result is 0.
 *   outputs     Each may be NULL (not wanted); at least one must be given.  out [rows_o][cols_o] of the source's type with
 *               its own row stride, covered uint8 [rows_o][cols_o], map_x, map_y float32 [rows_o][cols_o].
 *               A pixel no triangle owns, or whose source is out of range: out = fill (cast to the image type),
 *               covered = 0.  An owned pixel in range: covered = 1.  map_x, map_y = (float)sx, (float)sy for every owned
 *               pixel, in range or not (the quiet NaN 0x7fc00000 when sx or sy is not a number), and that NaN elsewhere.
 *               `src` may be NULL when `out` is; rows_s, cols_s then still say what is in range for `covered`.
 *
 * Every output element is written (the bytes between cols_o and out_stride are not); callers clear nothing.  grid_rows < 2,
 * grid_cols < 2 or an empty output are valid calls.  Strides are in elements, the inner stride is 1.
 * Returns 0, or a negative SID_PM_ERR_* code of sid_pm.h, found before any device call:
 *   SID_PM_ERR_ARG          a null node grid; no output; `out` without `src`; negative sizes; a stride below the row length; an
 *                           unknown dtype, order, diagonal or flag; SID_WARP_KEEP_ZERO with float32; a fill that uint8 cannot
 *                           hold (uint8 images); `out` overlapping `src`
 *   SID_PM_ERR_UNSUPPORTED  grid_rows * grid_cols >= 2^31, or an image axis >= 2^31
 */
#ifndef SID_WARP_H
#define SID_WARP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SID_WARP_U8  0
#define SID_WARP_F32 1

#define SID_WARP_KEEP_ZERO 1u

/* pixels of one work item of the warp kernel (rows x cols, anchored at the corner of a cell's pixel box); tests straddle it */
#define SID_WARP_TILE_ROWS 16
#define SID_WARP_TILE_COLS 64

/* Host buffers in, host buffers out; `device` is the HIP device index.  The call returns when the outputs are written.
 * device = -1 runs the same source in a host loop, without a GPU (for tests). */
int sid_warp_image(int device, const double *x, const double *y, const double *xs, const double *ys, const uint8_t *valid,
                   int64_t grid_rows, int64_t grid_cols,
                   const void *src, int dtype, int64_t rows_s, int64_t cols_s, int64_t src_stride,
                   int64_t rows_o, int64_t cols_o, int order, double fill, int diagonal, uint32_t flags,
                   void *out, int64_t out_stride, uint8_t *covered, float *map_x, float *map_y);

/* Device pointers in and out, on the current HIP device, work queued on `hip_stream` (a hipStream_t; may be NULL).  The call
 * copies nothing and waits for nothing, and allocates nothing beyond the module's grow-only scratch of that device (8 bytes
 * per grid cell; it grows on the first call and when a larger grid comes).  The scratch is one per device: calls on one device
 * must be ordered among themselves (one stream, or events between streams). */
int sid_warp_image_device(const double *x, const double *y, const double *xs, const double *ys, const uint8_t *valid,
                          int64_t grid_rows, int64_t grid_cols,
                          const void *src, int dtype, int64_t rows_s, int64_t cols_s, int64_t src_stride,
                          int64_t rows_o, int64_t cols_o, int order, double fill, int diagonal, uint32_t flags,
                          void *out, int64_t out_stride, uint8_t *covered, float *map_x, float *map_y, void *hip_stream);

const char *sid_warp_last_error(void);
/* Free the grow-only device scratch of `device` (every device: -1).  No call on that device may be in flight. */
int sid_warp_release(int device);

#ifdef __cplusplus
}
#endif
#endif
