/* sid_resize.h - C ABI of the area-average downsampling step on MI355X (gfx950): DESIGN.md section 22.
 *
 * Replaces, in the reference (sea_ice_drift v0.7.1), the first line of get_n(): n.resize(factor, resample_alg=-1)
 * (lib.py:256-257, 314-316; -1 is GDAL's average resampling), for a caller who holds the full-resolution band as an array.
 * Only the whole-ratio case (rows and columns divide evenly: the k x k block mean) is claimed to agree with what an average
 * resampler computes, and only as real numbers; the roundings below are this project's.  Downsampling only.
 *
 * Shapes.  Input rows x cols, output out_rows x out_cols, 1 <= out_rows <= rows, 1 <= out_cols <= cols, every dimension at
 * most 2^24 (SID_RESIZE_MAX_DIM).
 *
 * Weights, per axis (n the input length, m the output length): g = gcd(n, m), a = n / g, b = m / g.  Output index j covers
 * [j * a, (j + 1) * a), source index i covers [i * b, (i + 1) * b) of a common fine axis of n * b = m * a cells; the weight of i
 * in j is the integer length of the overlap.  The sources of j are i = (j * a) / b .. ceil((j + 1) * a / b) - 1, every weight
 * lies in 1..b, and the weights of one j sum to a.  When m divides n (b = 1) every weight is 1 and the windows are disjoint
 * blocks of k = n / m pixels; otherwise this is the exact area-weighted mean.
 *
 * float32 result.  acc = 0.0 in float64; over the window in row-major order (source rows ascending, within a row the columns
 * ascending): acc = acc + double(wr * wc) * double(x) - the integer product converted once, one rounding for the product and
 * one for the sum, no fused multiply-add; result float(acc / double(a_r * a_c)).  NaN and +-inf take part as IEEE arithmetic
 * has them (a window of -0.0 gives +0.0).  nan_omit != 0: source pixels that are NaN are left out of the sum and of the
 * divisor, which is then the integer sum of the products wr * wc that were used, converted once; a window with no pixel left
 * gives NaN; +-inf still take part.
 *
 * uint8 result.  S = sum of wr * wc * x (int64), T = a_r * a_c, result (2 * S + T) / (2 * T): round half up, exact integer
 * arithmetic.  zero_invalid != 0 (0 means invalid throughout this project): the output pixel is 0 exactly when some source
 * pixel of positive weight is 0 (a mean of values >= 1 is >= 1, so no other pixel becomes 0).
 *
 * All image pointers are device pointers; strides are in elements of the array they belong to; `hip_stream` is a hipStream_t
 * (may be NULL); the calls enqueue and return.  Arguments are checked on the host before any device call: a null pointer, a
 * dimension below 1, out > in or a stride below the columns is SID_PM_ERR_ARG, a dimension above SID_RESIZE_MAX_DIM
 * SID_PM_ERR_UNSUPPORTED (sid_pm.h); sid_resize_last_error() has the message.  A destination that overlaps a source is
 * undefined.  float32: whole ratios of 2 and 4 on both axes whose rows start 16-byte aligned in both arrays and whose output
 * rows are whole 16-byte words are moved with 16-byte accesses.  uint8: the ratio 2 with source rows that start 16-byte
 * aligned and output rows that start 8-byte aligned is loaded in 16-byte and stored in 8-byte words.  Every other layout or
 * ratio takes one output pixel per lane.  Both routes compute the sum above in the order above: the same bits.
 */
#ifndef SID_RESIZE_H
#define SID_RESIZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SID_RESIZE_MAX_DIM 16777216   /* 2^24 */

int sid_resize_f32(const float *d_src, int64_t rows, int64_t cols, int64_t stride,
                   float *d_dst, int64_t out_rows, int64_t out_cols, int64_t dst_stride, int nan_omit, void *hip_stream);

int sid_resize_u8(const uint8_t *d_src, int64_t rows, int64_t cols, int64_t stride,
                  uint8_t *d_dst, int64_t out_rows, int64_t out_cols, int64_t dst_stride, int zero_invalid, void *hip_stream);

/* The fused front of the sigma0 preparation (sid_prep.h): d_out[r][c] (out_rows x out_cols) = the pixel of sid_prep_apply at
 * (r, c) of the images sid_resize_f32 (nan_omit = 0) makes of d_img and d_ia (both rows x cols) - the same bits, without the
 * reduced float images ever being written.  d_mask (may be NULL) is out_rows x out_cols: it refers to the reduced image.
 * d_ia, d_mask, coeffs, dB, hh_factor as in sid_prep_apply. */
int sid_resize_prep_apply(const float *d_img, int64_t rows, int64_t cols, int64_t stride,
                          const float *d_ia, int64_t ia_stride, const uint8_t *d_mask, int64_t mask_stride,
                          int dB, float hh_factor, const double *coeffs,
                          float *d_out, int64_t out_rows, int64_t out_cols, int64_t out_stride, void *hip_stream);

/* d_sub[i][j] (float32, contiguous, [(out_rows + step - 1) / step][(out_cols + step - 1) / step]) = sid_prep_subsample of the
 * same reduced images at the reduced pixel (i * step, j * step). */
int sid_resize_prep_subsample(const float *d_img, int64_t rows, int64_t cols, int64_t stride,
                              const float *d_ia, int64_t ia_stride, const uint8_t *d_mask, int64_t mask_stride,
                              int dB, float hh_factor, int64_t step, int64_t out_rows, int64_t out_cols,
                              float *d_sub, void *hip_stream);

const char *sid_resize_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
