// landmask.hip - the invalid-pixel mask of get_invalid_mask (reference lib.py:342-373) on gfx950 (C ABI: include/sid_mask.h):
// the water-mask raster is clipped to 2 and dilated (maximum_filter of size 3), prefiltered (lw_spline_prefilter of
// pm_large.hip: SciPy's, operation for operation) and zoomed to the image's resolution with SciPy's cubic-spline arithmetic;
// the pixels the zoom takes to exactly 2 are land; pixels of the image that are not finite are ORed in.
//   clip_max3_kernel   min(wm, 2) and its 3 x 3 maximum with clamped indices, on the small raster
//   zoom_mask_kernel   a workgroup owns kRows output rows x (256 * PX) output columns.  A lane keeps the weights and the first
//                      tap of its PX columns in registers for all its rows (a column's are the same down the column); the rows'
//                      weights and first taps are worked out once, one row per lane, and read from LDS (a row's are the same
//                      across the row); the patch of spline coefficients the tile's taps reach - a few rows of a few dozen float64
//                      at the reference's zoom of 20 - is staged in LDS with the mirror mapping applied.  A patch beyond the LDS
//                      budget (zooms near 1 and below) is read from global memory instead: the same operands, the same
//                      operations.  -ffp-contract=off: every product and sum is a rounding of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <limits.h>
#include <algorithm>

#include "../../include/sid_mask.h"
#include "host_util.h"
#include "pm_large.h"
#include "prep_pixel.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 64;                // output rows per workgroup
constexpr int kTileCap = 4096;           // float64 coefficients staged per workgroup at the most (32 KiB)
constexpr int kOutside = INT_MIN;        // first tap of a row / column whose coordinate lies outside the raster
constexpr size_t kRowBytes = kRows * 4 * sizeof(double) + kRows * sizeof(int);   // LDS in front of the coefficient patch

__global__ __launch_bounds__(kThreads) void clip_max3_kernel(const uint8_t *wm, int h, int w, int64_t stride, uint8_t *out)
{
    const int64_t n = (int64_t)h * w;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int i = (int)(idx / w), j = (int)(idx - (int64_t)i * w);
        unsigned m = 0;
        for (int di = -1; di <= 1; ++di) {
            const int ii = min(max(i + di, 0), h - 1);
            for (int dj = -1; dj <= 1; ++dj) {
                const int jj = min(max(j + dj, 0), w - 1);
                const unsigned v = wm[(int64_t)ii * stride + jj];
                m = max(m, min(v, 2u));
            }
        }
        out[idx] = (uint8_t)m;
    }
}

struct Zoom {
    const double *coef;                  // [h][w] spline coefficients (null: no land)
    int h, w, H, W;
    double z0, z1;                       // (n_in - 1) / (n_out - 1) per axis
    int cap;                             // coefficients the launch's LDS patch can hold
};

// weights and first tap of output index k of an axis n_in -> n_out (scipy ni_interpolation.c NI_ZoomShift, mode 'constant')
__device__ __forceinline__ int axis_taps(int k, double z, int n_in, double *w)
{
    const double cc = (double)k * z;
    sid::lw_spline_weights(cc, 3, w);
    if (cc < 0.0 || cc > (double)(n_in - 1)) return kOutside;
    return (int)floor(cc) - 1;
}
__device__ __forceinline__ int first_tap(int k, double z) { return (int)floor((double)k * z) - 1; }   // (also of an outside index)

__device__ __forceinline__ uint32_t zoom_byte(double t)
{
    t = t > 0.0 ? t + 0.5 : 0.0;
    t = t > 255.0 ? 255.0 : t;
    return (uint32_t)(int)t;
}

template <int PX, bool IMG, bool LAND>
__global__ __launch_bounds__(kThreads) void zoom_mask_kernel(Zoom Z, const float *img, int64_t img_stride, bool db, const float *ia, int64_t ia_stride,
                                                             float f, uint8_t *mask, int64_t mask_stride, uint8_t *wmz, int64_t wmz_stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    double *rw = reinterpret_cast<double *>(lds);                         // [kRows][4] row weights
    int *rs = reinterpret_cast<int *>(lds + kRows * 4 * sizeof(double));  // [kRows] first row tap or kOutside
    double *tile = reinterpret_cast<double *>(lds + kRowBytes);           // [RL][LL] coefficients, mirrored

    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * kRows, nrows = min(kRows, Z.H - r0);
    const int c0 = blockIdx.x * (kThreads * PX), cend = min(c0 + kThreads * PX, Z.W);   // (c0 < W by the grid)
    const int c = c0 + tid * PX;

    double w1[PX][4];
    int cs[PX];
    int smin0 = 0, smin1 = 0, LL = 0;
    bool staged = false;
    if (LAND) {
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            cs[j] = kOutside;
            w1[j][0] = w1[j][1] = w1[j][2] = w1[j][3] = 0.0;
            if (c + j < Z.W) cs[j] = axis_taps(c + j, Z.z1, Z.w, w1[j]);
        }
        if (tid < nrows) {
            double w0[4];
            rs[tid] = axis_taps(r0 + tid, Z.z0, Z.h, w0);
            rw[4 * tid + 0] = w0[0]; rw[4 * tid + 1] = w0[1]; rw[4 * tid + 2] = w0[2]; rw[4 * tid + 3] = w0[3];
        }
        // the taps of the tile: rows first_tap(r0) .. first_tap(r0 + nrows - 1) + 3, likewise the columns (the coordinate grows with the index)
        smin0 = first_tap(r0, Z.z0);
        smin1 = first_tap(c0, Z.z1);
        const long long RL = (long long)first_tap(r0 + nrows - 1, Z.z0) - smin0 + 4;
        const long long LLw = (long long)first_tap(cend - 1, Z.z1) - smin1 + 4;
        staged = RL * LLw <= (long long)Z.cap;                            // (the same in every lane)
        if (staged) {
            LL = (int)LLw;
            const int n = (int)(RL * LLw);
            for (int idx = tid; idx < n; idx += kThreads) {
                const int i = idx / LL, j = idx - i * LL;
                tile[idx] = Z.coef[sid::lw_spline_mirror((long long)smin0 + i, Z.h) * Z.w + sid::lw_spline_mirror((long long)smin1 + j, Z.w)];
            }
        }
        __syncthreads();
    }

    for (int t = 0; t < nrows; ++t) {
        const int64_t r = r0 + t;
        float x[PX], a[PX];
        if (IMG) {
            if constexpr (PX == 4) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f), u = v;
                if (c < Z.W) {
                    v = *reinterpret_cast<const float4 *>(img + r * img_stride + c);
                    if (ia) u = *reinterpret_cast<const float4 *>(ia + r * ia_stride + c);
                }
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
                a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w;
            } else {
                x[0] = a[0] = 0.f;
                if (c < Z.W) {
                    x[0] = img[r * img_stride + c];
                    if (ia) a[0] = ia[r * ia_stride + c];
                }
            }
        }
        uint32_t zb[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) zb[j] = 0;
        if (LAND) {
            const int s0 = rs[t];
            if (s0 != kOutside) {
                const double w0[4] = {rw[4 * t], rw[4 * t + 1], rw[4 * t + 2], rw[4 * t + 3]};
#pragma unroll
                for (int j = 0; j < PX; ++j) {
                    if (cs[j] == kOutside) continue;
                    double acc = 0.0;
                    if (staged) {
                        const double *p = tile + (s0 - smin0) * LL + (cs[j] - smin1);
#pragma unroll
                        for (int ta = 0; ta < 4; ++ta)
#pragma unroll
                            for (int tb = 0; tb < 4; ++tb) acc = acc + (p[ta * LL + tb] * w0[ta]) * w1[j][tb];
                    } else {
                        long long ib[4];
#pragma unroll
                        for (int tb = 0; tb < 4; ++tb) ib[tb] = sid::lw_spline_mirror((long long)cs[j] + tb, Z.w);
#pragma unroll 1
                        for (int ta = 0; ta < 4; ++ta) {                  // (rolled: this path is the exception, and its registers would be the kernel's)
                            const double *row = Z.coef + sid::lw_spline_mirror((long long)s0 + ta, Z.h) * Z.w;
                            const double wa = rw[4 * t + ta];
#pragma unroll
                            for (int tb = 0; tb < 4; ++tb) acc = acc + (row[ib[tb]] * wa) * w1[j][tb];
                        }
                    }
                    zb[j] = zoom_byte(acc);
                }
            }
        }
        uint32_t mb[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            mb[j] = zb[j] == 2u ? 1u : 0u;
            if (IMG) {
                const float v = prep_pixel(db, ia != nullptr, false, false, x[j], a[j], 0u, f, 0.0);
                if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) mb[j] = 1u;      // NaN or +-inf
            }
        }
        if (c < Z.W) {
            if constexpr (PX == 4) {                                  // (W % 4 == 0: all four pixels exist)
                if (mask) *reinterpret_cast<uint32_t *>(mask + r * mask_stride + c) = mb[0] | (mb[1] << 8) | (mb[2] << 16) | (mb[3] << 24);
                if (wmz) *reinterpret_cast<uint32_t *>(wmz + r * wmz_stride + c) = zb[0] | (zb[1] << 8) | (zb[2] << 16) | (zb[3] << 24);
            } else {
                if (mask) mask[r * mask_stride + c] = (uint8_t)mb[0];
                if (wmz) wmz[r * wmz_stride + c] = (uint8_t)zb[0];
            }
        }
    }
}

bool aligned(const void *p, int64_t stride, int64_t item, uintptr_t bytes)
{
    return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0 && ((uintptr_t)(stride * item) & (bytes - 1)) == 0;
}

int check_plane(const void *p, int64_t cols, int64_t stride, const char *what)
{
    if (!p) return fail(SID_PM_ERR_ARG, "null %s pointer", what);
    if (stride < cols) return fail(SID_PM_ERR_ARG, "%s: row stride %lld below the %lld columns", what, (long long)stride, (long long)cols);
    return SID_PM_OK;
}

// coefficients the taps of `n` consecutive output indices reach along an axis with zoom step z, at the most
long long taps_bound(int n, double z) { return (long long)ceil((double)(n - 1) * z) + 5; }

template <int PX>
void launch_zoom(bool with_img, bool land, dim3 grid, size_t lds, hipStream_t st, const Zoom &Z, const float *img, int64_t img_stride, bool db,
                 const float *ia, int64_t ia_stride, float f, uint8_t *mask, int64_t mask_stride, uint8_t *wmz, int64_t wmz_stride)
{
#define SID_MASK_LAUNCH(I, L) hipLaunchKernelGGL((zoom_mask_kernel<PX, I, L>), grid, dim3(kThreads), lds, st, Z, img, img_stride, db, ia, ia_stride, f, \
                                                 mask, mask_stride, wmz, wmz_stride)
    if (with_img && land) SID_MASK_LAUNCH(true, true);
    else if (with_img) SID_MASK_LAUNCH(true, false);
    else SID_MASK_LAUNCH(false, true);
#undef SID_MASK_LAUNCH
}

int run(const uint8_t *d_wm, int64_t h, int64_t w, int64_t wm_stride, int64_t H, int64_t W, void *d_work, const float *d_img, int64_t img_stride,
        int dB, const float *d_ia, int64_t ia_stride, float hh_factor, uint8_t *d_mask, int64_t mask_stride, uint8_t *d_wmz, int64_t wmz_stride,
        void *hip_stream)
{
    if (H < 1 || W < 1 || H > INT_MAX || W > INT_MAX) return fail(SID_PM_ERR_ARG, "bad image shape");
    if (!d_wm && !d_img) return fail(SID_PM_ERR_ARG, "neither a water mask nor an image");
    if (!d_mask && !d_wmz) return fail(SID_PM_ERR_ARG, "null output");
    if (d_mask) { if (int rc = check_plane(d_mask, W, mask_stride, "mask")) return rc; }
    if (d_wmz) { if (int rc = check_plane(d_wmz, W, wmz_stride, "zoomed water mask")) return rc; }
    if (d_img) { if (int rc = check_plane(d_img, W, img_stride, "image")) return rc; }
    if (d_ia) {
        if (!d_img) return fail(SID_PM_ERR_ARG, "an incidence angle without an image");
        if (int rc = check_plane(d_ia, W, ia_stride, "incidence angle")) return rc;
    }
    if (d_wm) {
        if (h < 2 || w < 2 || h > INT_MAX || w > INT_MAX || h * w > (int64_t)1 << 40)
            return fail(SID_PM_ERR_ARG, "water mask of %lld x %lld: both axes need at least 2 elements (SciPy does not prefilter an axis of length 1)",
                        (long long)h, (long long)w);
        if (int rc = check_plane(d_wm, w, wm_stride, "water mask")) return rc;
        if (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 255u)) return fail(SID_PM_ERR_ARG, "workspace: null or not 256-byte aligned");
    }
    if ((H + kRows - 1) / kRows > 65535) return fail(SID_PM_ERR_UNSUPPORTED, "more than %d rows", 65535 * kRows);
    DeviceOf guard(d_mask ? d_mask : d_wmz);
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);

    Zoom Z = {};
    Z.h = (int)h; Z.w = (int)w; Z.H = (int)H; Z.W = (int)W;
    const bool vec = (W & 3) == 0 && (!d_img || aligned(d_img, img_stride, 4, 16)) && (!d_ia || aligned(d_ia, ia_stride, 4, 16)) &&
                     (!d_mask || aligned(d_mask, mask_stride, 1, 4)) && (!d_wmz || aligned(d_wmz, wmz_stride, 1, 4));
    const int px = vec ? 4 : 1;
    size_t lds = 0;
    if (d_wm) {
        const size_t plane = up((size_t)h * (size_t)w * sizeof(double));
        double *buf0 = static_cast<double *>(d_work), *buf1 = reinterpret_cast<double *>(static_cast<char *>(d_work) + plane);
        uint8_t *wmf = reinterpret_cast<uint8_t *>(static_cast<char *>(d_work) + 2 * plane);
        const int64_t blocks = std::min<int64_t>((h * w + kThreads - 1) / kThreads, 2048);
        hipLaunchKernelGGL(clip_max3_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, d_wm, (int)h, (int)w, wm_stride, wmf);
        if (hipGetLastError() != hipSuccess) return fail(SID_PM_ERR_HIP, "water-mask filter: launch failed");
        const int rc = sid::lw_spline_prefilter(wmf, h, w, w, 3, buf0, buf1, st);
        if (rc != 0) return fail(SID_PM_ERR_HIP, "spline prefilter: %s", hipGetErrorString((hipError_t)rc));
        Z.coef = buf1;
        Z.z0 = H > 1 ? (double)(h - 1) / (double)(H - 1) : 1.0;
        Z.z1 = W > 1 ? (double)(w - 1) / (double)(W - 1) : 1.0;
        const long long patch = taps_bound((int)std::min<int64_t>(kRows, H), Z.z0) * taps_bound((int)std::min<int64_t>((int64_t)kThreads * px, W), Z.z1);
        Z.cap = patch <= kTileCap ? (int)patch : 0;
        lds = kRowBytes + (size_t)Z.cap * sizeof(double);
    }
    const dim3 grid((unsigned)((W + (int64_t)kThreads * px - 1) / ((int64_t)kThreads * px)), (unsigned)((H + kRows - 1) / kRows));
    if (vec) launch_zoom<4>(d_img != nullptr, d_wm != nullptr, grid, lds, st, Z, d_img, img_stride, dB != 0, d_ia, ia_stride, hh_factor, d_mask, mask_stride, d_wmz, wmz_stride);
    else launch_zoom<1>(d_img != nullptr, d_wm != nullptr, grid, lds, st, Z, d_img, img_stride, dB != 0, d_ia, ia_stride, hh_factor, d_mask, mask_stride, d_wmz, wmz_stride);
    return launched("zoom");
}

}  // namespace

SID_EXPORT const char *sid_mask_last_error(void) { return g_err; }

SID_EXPORT int64_t sid_mask_workspace_bytes(int64_t h, int64_t w)
{
    if (h < 2 || w < 2 || h > INT_MAX || w > INT_MAX || h * w > (int64_t)1 << 40) return 0;
    return (int64_t)(2 * up((size_t)h * (size_t)w * sizeof(double)) + up((size_t)h * (size_t)w));
}

SID_EXPORT int sid_mask_landmask(const uint8_t *d_wm, int64_t h, int64_t w, int64_t wm_stride, int64_t H, int64_t W, void *d_work,
                                 uint8_t *d_mask, int64_t mask_stride, uint8_t *d_wmz, int64_t wmz_stride, void *hip_stream)
{
    if (!d_wm) return fail(SID_PM_ERR_ARG, "null water mask pointer");
    return run(d_wm, h, w, wm_stride, H, W, d_work, nullptr, 0, 0, nullptr, 0, 0.f, d_mask, mask_stride, d_wmz, wmz_stride, hip_stream);
}

SID_EXPORT int sid_mask_invalid(const uint8_t *d_wm, int64_t h, int64_t w, int64_t wm_stride, int64_t H, int64_t W, void *d_work,
                                const float *d_img, int64_t img_stride, int dB, const float *d_ia, int64_t ia_stride, float hh_factor,
                                uint8_t *d_mask, int64_t mask_stride, uint8_t *d_wmz, int64_t wmz_stride, void *hip_stream)
{
    if (!d_img) return fail(SID_PM_ERR_ARG, "null image pointer");
    if (!d_mask) return fail(SID_PM_ERR_ARG, "null mask pointer");
    return run(d_wm, h, w, wm_stride, H, W, d_work, d_img, img_stride, dB, d_ia, ia_stride, hh_factor, d_mask, mask_stride, d_wmz, wmz_stride, hip_stream);
}
