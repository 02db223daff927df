/* sid_prep.h - C ABI of the sigma0 preparation step on MI355X (gfx950): DESIGN.md section 16.
 *
 * Replaces, in the reference (sea_ice_drift v0.7.1), the array half of lib.py:318-331 get_n():
 *
 *     img[img <= 0] = nan ; img = 10 * log10(img)          dB               (lib.py:320-322)
 *     img = img - incidence_angle * correct_hh_factor      HH correction    (lib.py:203-223)
 *     img[mask] = nan                                      invalid pixels   (lib.py:325-327)
 *     img -= get_spatial_mean(img)                         detrend          (lib.py:225-254, 328-329)
 *
 * in that order, each step optional; the result is the float32 working image that sid_stage_* (sid_stage.h) turns into
 * uint8.  Per pixel, with every operation rounded as NumPy rounds it and no fused multiply-add:
 *
 *     dB      v = x > 0 ? float(10) * float(log10(double(x))) : NaN      (x <= 0 and NaN give NaN; +inf stays +inf;
 *                                                                          sid_prep_debug_log10 below)
 *     HH      v = v - ia * hh_factor                                     (two float32 operations)
 *     mask    v = mask != 0 ? NaN : v
 *     mean    m = ((((c0*col + c1*col^2) + c2*row) + c3*row^2) + (c4*col)*row) + c5     (float64; col^2, row^2 exact integers)
 *     detrend v = float(double(v) - m)
 *
 * The six coefficients come from the caller (sea_ice_drift_amd/lib.py fits them on the host with the reference's own NumPy
 * calls on the [::step, ::step] subsample that sid_prep_subsample delivers).
 *
 * All image pointers are device pointers; strides are in elements of the array they belong to; `coeffs` is a HOST pointer to
 * six doubles (passed to the kernel by value).  d_ia == NULL: no HH correction; d_mask == NULL: no mask; coeffs == NULL: no
 * detrend.  `hip_stream` is a hipStream_t (may be NULL); the calls enqueue and return.  Rows whose start is 16-byte aligned in
 * every array (and 4-byte aligned in the mask) are moved with 16-byte accesses, any other layout one pixel per lane.
 * 0 on success, a negative SID_PM_ERR_* code otherwise (sid_pm.h); sid_prep_last_error() has the message.
 */
#ifndef SID_PREP_H
#define SID_PREP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* d_sub[i][j] (float32, contiguous, [(rows + step - 1) / step][(cols + step - 1) / step]) = the image after dB / HH / mask at
 * pixel (i * step, j * step): what the reference's get_spatial_mean reads of it (step = 50 there). */
int sid_prep_subsample(const float *d_img, int64_t rows, int64_t cols, int64_t stride,
                       const float *d_ia, int64_t ia_stride, const uint8_t *d_mask, int64_t mask_stride,
                       int dB, float hh_factor, int64_t step, float *d_sub, void *hip_stream);

/* One pass over the image: d_out[r][c] = the pixel after dB / HH / mask / detrend.  d_out may be d_img itself (every lane reads its
 * pixels before it writes them); any other overlap is undefined. */
int sid_prep_apply(const float *d_img, int64_t rows, int64_t cols, int64_t stride,
                   const float *d_ia, int64_t ia_stride, const uint8_t *d_mask, int64_t mask_stride,
                   int dB, float hh_factor, const double *coeffs, float *d_out, int64_t out_stride, void *hip_stream);

/* d_out[r][c] (float64) = m(r, c) above: the reference's get_spatial_mean for given coefficients. */
int sid_prep_spatial_mean(int64_t rows, int64_t cols, const double *coeffs, double *d_out, int64_t out_stride,
                          void *hip_stream);

/* The dB step's float32 logarithm takes a short float64 evaluation wherever that decides the rounding, the library's float64
 * log10 elsewhere.  For the n float32 bit patterns from first_bits on (those that are not > 0 are skipped), on the current
 * device: counts[0] (host) = how many give another float32 than float(log10(double(x))), counts[1] = how many took the
 * library route.  Synchronous. */
int sid_prep_debug_log10(uint32_t first_bits, uint64_t n, uint64_t *counts);

const char *sid_prep_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
