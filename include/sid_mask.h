/* sid_mask.h - C ABI of the invalid-pixel mask on MI355X (gfx950): DESIGN.md section 17.
 *
 * Replaces, in the reference (sea_ice_drift v0.7.1), the array half of lib.py:342-373 get_invalid_mask():
 *
 *     mask = isnan(img) + isinf(img)
 *     wm[wm > 2] = 2 ; wmf = maximum_filter(wm, 3)          on the small water-mask raster (h x w, uint8)
 *     wmz = zoom(wmf, img.shape / wm.shape)                 cubic spline to the image's H x W, uint8
 *     mask[wmz == 2] = True
 *
 * bit for bit (SciPy 1.15: ndimage.zoom with order 3, mode 'constant', cval 0, prefilter, output dtype uint8).  Per axis
 * (n_in -> n_out): z = (n_in - 1) / (n_out - 1) in float64 (1 when n_out == 1); output index k reads the coordinate
 * cc = double(k) * z; cc < 0 or cc > n_in - 1 gives the constant 0 (no tolerance: (n_out - 1) * z may round one ulp above
 * n_in - 1, and the whole last row or column is then 0); otherwise four taps from floor(cc) - 1 on, each index through SciPy's
 * mirror mapping, weighted with SciPy's cubic B-spline weights of cc.  A pixel is
 *
 *     t = sum over a (axis 0, outer), b (axis 1, inner) of (coef[ia][ib] * w0[a]) * w1[b]      float64, from 0.0, no fused multiply-add
 *     wmz = uint8(min(t > 0 ? t + 0.5 : 0, 255))
 *
 * over the float64 spline coefficients of wmf (prefilter along axis 0, then axis 1, mirror boundary).  The land plane is
 * wmz == 2 - the spline overshoots, and a pixel it takes to 3 is not land: the reference's behaviour, kept.
 *
 * All image pointers are device pointers; strides are in elements of the array they belong to; `hip_stream` is a hipStream_t
 * (may be NULL); the calls enqueue and return.  d_work: sid_mask_workspace_bytes(h, w) bytes of device scratch, 256-byte
 * aligned, which must stay untouched until the call's kernels have run.  2 <= h, w (SciPy does not filter an axis of length 1:
 * refused), 1 <= H, W, all below 2^31.  Rows whose start is 16-byte aligned in the image and the incidence angle and 4-byte
 * aligned in the byte planes (and W % 4 == 0) are moved four pixels per lane, any other layout one pixel per lane.
 * 0 on success, a negative SID_PM_ERR_* code otherwise (sid_pm.h); sid_mask_last_error() has the message.
 */
#ifndef SID_MASK_H
#define SID_MASK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* device scratch for a water mask of h x w: the filtered raster and two float64 planes of the spline prefilter; 0 for a bad shape */
int64_t sid_mask_workspace_bytes(int64_t h, int64_t w);

/* d_mask[r][c] (uint8, H x W) = 1 where wmz == 2, else 0; d_wmz (may be NULL) receives the wmz bytes themselves.  d_mask may be
 * NULL when d_wmz is given. */
int sid_mask_landmask(const uint8_t *d_wm, int64_t h, int64_t w, int64_t wm_stride, int64_t H, int64_t W, void *d_work,
                      uint8_t *d_mask, int64_t mask_stride, uint8_t *d_wmz, int64_t wmz_stride, void *hip_stream);

/* d_mask[r][c] = land (as above; d_wm == NULL: no land, h, w and d_work are ignored) OR "the pixel of d_img (float32, H x W) is
 * NaN or +-inf after the dB / HH steps of sid_prep_apply" - the same per-pixel code (dB != 0: the dB step; d_ia != NULL: the HH
 * correction with hh_factor).  dB == 0 and d_ia == NULL: isnan | isinf of the image itself. */
int sid_mask_invalid(const uint8_t *d_wm, int64_t h, int64_t w, int64_t wm_stride, int64_t H, int64_t W, void *d_work,
                     const float *d_img, int64_t img_stride, int dB, const float *d_ia, int64_t ia_stride, float hh_factor,
                     uint8_t *d_mask, int64_t mask_stride, uint8_t *d_wmz, int64_t wmz_stride, void *hip_stream);

const char *sid_mask_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
