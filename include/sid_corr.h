/* sid_corr.h - C ABI of the local correlation of two uint8 images on MI355X (gfx950): the zero-mean normalised correlation of
 * image `a` against image `b` over a square window around each node - per point of a grid, or as a map.  Not the reference's:
 * it has no such step.  The use is the quality of a warp (image 1 against image 2 warped onto it, include/sid_warp.h) and the
 * detection of change between the scenes.  DESIGN.md section 24; NumPy restatement: tests/corr_spec.py.
 *
 * Images a, b are uint8 [rows][cols] of one shape, each with its own row stride in elements (the inner stride is 1); 0 is the
 * project's invalid value.  `w` is the window side, 1 <= w <= 255.
 *
 *   window      A node centred at the integer (rc, cc) has the rows rc - w/2 .. rc - w/2 + w - 1 (integer division) and the
 *               columns cc - w/2 .. cc - w/2 + w - 1, clipped to the image as NumPy slicing clips: it may be empty, and
 *               centres may lie anywhere outside the image.
 *   usable      A pixel of the clipped window is usable iff a != 0 and b != 0 there.
 *   sums        Over the usable pixels, exact in integers: n (their number), Sa, Sb, Saa, Sbb, Sab, and
 *                   va = n*Saa - Sa*Sa ;  vb = n*Sbb - Sb*Sb ;  cab = n*Sab - Sa*Sb
 *               All fit int64 (n*Saa <= 65025 * 65025 * 65025 < 2^53); a whole window of 255s has Saa = 4 228 250 625 > 2^31.
 *   result      If n < min_count, va <= 0 or vb <= 0: r is the quiet NaN 0x7ff8000000000000.  Otherwise
 *                   r = (double)cab / sqrt((double)va * (double)vb)
 *               every float64 operation one IEEE rounding in the order written (built with -ffp-contract=off; the three
 *               conversions are exact), then r > 1 becomes 1 and r < -1 becomes -1.
 *   outputs     Each may be NULL (not wanted); at least one must be given.  corr float64 per node, count int32 (n) per node,
 *               sums int64 [node][5] = Sa, Sb, Saa, Sbb, Sab.  Every element of a given output is written; callers clear
 *               nothing.
 *
 * sid_corr_lattice: node (i, j), i < nr, j < nc, has the centre (r0 + i*sr, c0 + j*sc); sr, sc >= 1; r0, c0 are any int64.
 * A centre beyond +-2^40 counts as 2^40 of that sign (its window is empty either way).  Outputs are [nr][nc].
 * sid_corr_points: node k < npts has the centre (r[k], c[k]), int32.  `valid` (uint8 [npts], may be NULL): a node with
 * valid == 0 gets n = 0, zero sums and r = NaN, and its centre is not read.
 *
 * nr * nc == 0, npts == 0 and an empty image are valid calls (with an empty image every node is empty).
 * Returns 0, or a negative SID_PM_ERR_* code of sid_pm.h, found before any device call:
 *   SID_PM_ERR_ARG          a null image; no output; negative sizes; a stride below the row length; sr or sc below 1;
 *                           min_count below 1; null centres with npts > 0; an output overlapping an image
 *   SID_PM_ERR_UNSUPPORTED  w outside 1..255; an image axis >= 2^31; nr * nc or npts >= 2^31
 */
#ifndef SID_CORR_H
#define SID_CORR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* nodes of one workgroup of the lattice kernel (rows x cols); tests straddle it */
#define SID_CORR_TILE_ROWS 8
#define SID_CORR_TILE_COLS 64

/* Host buffers in, host buffers out; `device` is the HIP device index.  The call returns when the outputs are written.
 * device = -1 runs the same source in a host loop, without a GPU (for tests). */
int sid_corr_lattice(int device, const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t rows, int64_t cols,
                     int w, int64_t r0, int64_t c0, int64_t sr, int64_t sc, int64_t nr, int64_t nc, int64_t min_count,
                     double *corr, int32_t *count, int64_t *sums);
int sid_corr_points(int device, const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t rows, int64_t cols,
                    int w, const int32_t *c, const int32_t *r, const uint8_t *valid, int64_t npts, int64_t min_count,
                    double *corr, int32_t *count, int64_t *sums);

/* Device pointers in and out, on the current HIP device, work queued on `hip_stream` (a hipStream_t; may be NULL).  The calls
 * copy nothing, wait for nothing and allocate nothing: the kernels need no scratch. */
int sid_corr_lattice_device(const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t rows, int64_t cols,
                            int w, int64_t r0, int64_t c0, int64_t sr, int64_t sc, int64_t nr, int64_t nc, int64_t min_count,
                            double *corr, int32_t *count, int64_t *sums, void *hip_stream);
int sid_corr_points_device(const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t rows, int64_t cols,
                           int w, const int32_t *c, const int32_t *r, const uint8_t *valid, int64_t npts, int64_t min_count,
                           double *corr, int32_t *count, int64_t *sums, void *hip_stream);

const char *sid_corr_last_error(void);
/* Free the grow-only staging block of the host-buffer entry points on `device` (every device: -1).  No call on that device
 * may be in flight. */
int sid_corr_release(int device);

#ifdef __cplusplus
}
#endif
#endif
