// prep.hip - sigma0 preparation on gfx950 (C ABI: include/sid_prep.h; the array half of get_n, lib.py:318-331):
// dB, HH angular correction, invalid-pixel mask and the removal of the second-order spatial mean in ONE streaming pass
// that writes the float32 working image of the uint8 staging step (stage.hip).  Steps that are switched off are compiled
// out (template parameters), so the pass moves 4 B in + 4 B out per pixel plus 4 B of incidence angle and 1 B of mask when
// those are used.  Arithmetic: NumPy's, operation for operation (the Makefile's -ffp-contract=off keeps every product and
// sum a rounding of its own; the fma calls below are written out); the float32 logarithm is float64 log10 rounded once
// (DESIGN.md section 16).
//   apply_kernel      one workgroup per row (grid-stride over rows), 16-byte words across the row, two in flight per lane
//   subsample_kernel  the same per-pixel function at the [::step, ::step] positions only (input of the host's fit)
//   mean_kernel       the float64 polynomial image alone (get_spatial_mean)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>

#include "../../include/sid_prep.h"
#include "host_util.h"
#include "prep_pixel.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 2;               // 16-byte words in flight per lane and array

template <bool DB, bool HH, bool MASK, bool MEAN, bool VEC>
__global__ __launch_bounds__(kThreads) void apply_kernel(const float *img, int64_t rows, int64_t cols, int64_t stride,
                                                         const float *ia, int64_t ia_stride, const uint8_t *mask, int64_t mask_stride,
                                                         float f, Coef K, float *out, int64_t out_stride)
{
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const float *row = img + r * stride;
        const float *iarow = HH ? ia + r * ia_stride : nullptr;
        const uint8_t *mrow = MASK ? mask + r * mask_stride : nullptr;
        float *orow = out + r * out_stride;
        const double dr = (double)r, c2r = MEAN ? K.c[2] * dr : 0.0, c3r2 = MEAN ? K.c[3] * (double)(r * r) : 0.0;
        if (VEC) {                                           // cols % 4 == 0 and every row start aligned (host check)
            const float4 *row4 = reinterpret_cast<const float4 *>(row);
            const float4 *ia4 = reinterpret_cast<const float4 *>(iarow);
            const uint32_t *m4 = reinterpret_cast<const uint32_t *>(mrow);
            float4 *o4 = reinterpret_cast<float4 *>(orow);
            const int64_t n4 = cols >> 2;
            for (int64_t base = 0; base < n4; base += kThreads * kUnroll) {
                float4 v[kUnroll], a[kUnroll];
                uint32_t m[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int64_t x = base + u * kThreads + threadIdx.x;
                    v[u] = a[u] = make_float4(0.f, 0.f, 0.f, 0.f); m[u] = 0;
                    if (x < n4) {
                        v[u] = row4[x];
                        if (HH) a[u] = ia4[x];
                        if (MASK) m[u] = m4[x];
                    }
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int64_t x = base + u * kThreads + threadIdx.x;
                    if (x >= n4) continue;
                    const int64_t c = x << 2;
                    double mu[4] = {0.0, 0.0, 0.0, 0.0};
                    if (MEAN) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) mu[k] = spatial_mean(K, c + k, dr, c2r, c3r2);
                    }
                    float4 o;
                    o.x = prep_pixel(DB, HH, MASK, MEAN, v[u].x, a[u].x, m[u] & 0xffu, f, mu[0]);
                    o.y = prep_pixel(DB, HH, MASK, MEAN, v[u].y, a[u].y, m[u] & 0xff00u, f, mu[1]);
                    o.z = prep_pixel(DB, HH, MASK, MEAN, v[u].z, a[u].z, m[u] & 0xff0000u, f, mu[2]);
                    o.w = prep_pixel(DB, HH, MASK, MEAN, v[u].w, a[u].w, m[u] & 0xff000000u, f, mu[3]);
                    o4[x] = o;
                }
            }
        } else {
            for (int64_t c = threadIdx.x; c < cols; c += kThreads) {
                const double mu = MEAN ? spatial_mean(K, c, dr, c2r, c3r2) : 0.0;
                orow[c] = prep_pixel(DB, HH, MASK, MEAN, row[c], HH ? iarow[c] : 0.f, MASK ? (uint32_t)mrow[c] : 0u, f, mu);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void subsample_kernel(const float *img, int64_t stride, const float *ia, int64_t ia_stride,
                                                             const uint8_t *mask, int64_t mask_stride, bool db, float f,
                                                             int64_t step, int64_t nrs, int64_t ncs, float *sub)
{
    const int64_t n = nrs * ncs;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int64_t r = (i / ncs) * step, c = (i % ncs) * step;           // (r < rows, c < cols: nrs = ceil(rows / step))
        sub[i] = prep_pixel(db, ia != nullptr, mask != nullptr, false, img[r * stride + c], ia ? ia[r * ia_stride + c] : 0.f,
                            mask ? (uint32_t)mask[r * mask_stride + c] : 0u, f, 0.0);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void mean_kernel(int64_t rows, int64_t cols, Coef K, double *out, int64_t out_stride)
{
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        double *orow = out + r * out_stride;
        const double dr = (double)r, c2r = K.c[2] * dr, c3r2 = K.c[3] * (double)(r * r);
        if (VEC) {                                           // 16-byte stores: two float64 per lane, the odd last column alone
            double2 *o2 = reinterpret_cast<double2 *>(orow);
            const int64_t n2 = cols >> 1;
            for (int64_t x = threadIdx.x; x < n2; x += kThreads)
                o2[x] = make_double2(spatial_mean(K, 2 * x, dr, c2r, c3r2), spatial_mean(K, 2 * x + 1, dr, c2r, c3r2));
            if ((cols & 1) && threadIdx.x == 0) orow[cols - 1] = spatial_mean(K, cols - 1, dr, c2r, c3r2);
        } else {
            for (int64_t c = threadIdx.x; c < cols; c += kThreads) orow[c] = spatial_mean(K, c, dr, c2r, c3r2);
        }
    }
}

// counts[0] += bit patterns in [first, first + n) whose short evaluation differs from float(log10(double(x))),
// counts[1] += those that took the library route
__global__ __launch_bounds__(kThreads) void log10_sweep_kernel(uint32_t first, uint64_t n, unsigned long long *counts)
{
    unsigned long long bad = 0, slow_n = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const float x = __uint_as_float(first + (uint32_t)i);
        if (!(x > 0.0f)) continue;
        bool slow;
        const float a = log10_f32(x, &slow), ref = (float)log10((double)x);
        bad += __float_as_uint(a) != __float_as_uint(ref) ? 1ull : 0ull;
        slow_n += slow ? 1ull : 0ull;
    }
    if (bad) atomicAdd(&counts[0], bad);
    if (slow_n) atomicAdd(&counts[1], slow_n);
}

int grid_rows(int64_t rows) { return (int)std::max<int64_t>(1, std::min<int64_t>(rows, 256 * 16)); }

int check_plane(const void *p, int64_t cols, int64_t stride, const char *what)
{
    if (!p) return fail(SID_PM_ERR_ARG, "null %s pointer", what);
    if (stride < cols) return fail(SID_PM_ERR_ARG, "%s: row stride %lld below the %lld columns", what, (long long)stride, (long long)cols);
    return SID_PM_OK;
}

bool aligned(const void *p, int64_t stride, int64_t item, uintptr_t bytes)
{
    return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0 && ((uintptr_t)(stride * item) & (bytes - 1)) == 0;
}

template <bool VEC>
void launch_apply(int steps, dim3 grid, hipStream_t st, const float *img, int64_t rows, int64_t cols, int64_t stride,
                  const float *ia, int64_t ia_stride, const uint8_t *mask, int64_t mask_stride, float f, const Coef &K,
                  float *out, int64_t out_stride)
{
#define SID_PREP_CASE(b) case b: hipLaunchKernelGGL((apply_kernel<((b) & 1) != 0, ((b) & 2) != 0, ((b) & 4) != 0, ((b) & 8) != 0, VEC>), \
        grid, dim3(kThreads), 0, st, img, rows, cols, stride, ia, ia_stride, mask, mask_stride, f, K, out, out_stride); break;
    switch (steps) {                                         // bit 0 dB, bit 1 HH, bit 2 mask, bit 3 detrend
        SID_PREP_CASE(0) SID_PREP_CASE(1) SID_PREP_CASE(2) SID_PREP_CASE(3) SID_PREP_CASE(4) SID_PREP_CASE(5) SID_PREP_CASE(6) SID_PREP_CASE(7)
        SID_PREP_CASE(8) SID_PREP_CASE(9) SID_PREP_CASE(10) SID_PREP_CASE(11) SID_PREP_CASE(12) SID_PREP_CASE(13) SID_PREP_CASE(14) SID_PREP_CASE(15)
    }
#undef SID_PREP_CASE
}

}  // namespace

SID_EXPORT const char *sid_prep_last_error(void) { return g_err; }

SID_EXPORT int sid_prep_subsample(const float *d_img, int64_t rows, int64_t cols, int64_t stride,
                                  const float *d_ia, int64_t ia_stride, const uint8_t *d_mask, int64_t mask_stride,
                                  int dB, float hh_factor, int64_t step, float *d_sub, void *hip_stream)
{
    if (rows < 1 || cols < 1) return fail(SID_PM_ERR_ARG, "bad image shape");
    if (step < 1) return fail(SID_PM_ERR_ARG, "step must be positive");
    if (int rc = check_plane(d_img, cols, stride, "image")) return rc;
    if (d_ia) { if (int rc = check_plane(d_ia, cols, ia_stride, "incidence angle")) return rc; }
    if (d_mask) { if (int rc = check_plane(d_mask, cols, mask_stride, "mask")) return rc; }
    if (!d_sub) return fail(SID_PM_ERR_ARG, "null output");
    DeviceOf guard(d_img);
    const int64_t nrs = (rows + step - 1) / step, ncs = (cols + step - 1) / step;
    const int64_t blocks = std::min<int64_t>((nrs * ncs + kThreads - 1) / kThreads, 2048);
    hipLaunchKernelGGL(subsample_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(hip_stream),
                       d_img, stride, d_ia, ia_stride, d_mask, mask_stride, dB != 0, hh_factor, step, nrs, ncs, d_sub);
    return launched("subsample");
}

SID_EXPORT int sid_prep_apply(const float *d_img, int64_t rows, int64_t cols, int64_t stride,
                              const float *d_ia, int64_t ia_stride, const uint8_t *d_mask, int64_t mask_stride,
                              int dB, float hh_factor, const double *coeffs, float *d_out, int64_t out_stride, void *hip_stream)
{
    if (rows < 1 || cols < 1) return fail(SID_PM_ERR_ARG, "bad image shape");
    if (int rc = check_plane(d_img, cols, stride, "image")) return rc;
    if (d_ia) { if (int rc = check_plane(d_ia, cols, ia_stride, "incidence angle")) return rc; }
    if (d_mask) { if (int rc = check_plane(d_mask, cols, mask_stride, "mask")) return rc; }
    if (int rc = check_plane(d_out, cols, out_stride, "output")) return rc;
    DeviceOf guard(d_img);
    Coef K;
    for (int k = 0; k < 6; ++k) K.c[k] = coeffs ? coeffs[k] : 0.0;
    const int steps = (dB ? 1 : 0) | (d_ia ? 2 : 0) | (d_mask ? 4 : 0) | (coeffs ? 8 : 0);
    const bool vec = (cols & 3) == 0 && aligned(d_img, stride, 4, 16) && aligned(d_out, out_stride, 4, 16) &&
                     (!d_ia || aligned(d_ia, ia_stride, 4, 16)) && (!d_mask || aligned(d_mask, mask_stride, 1, 4));
    const dim3 grid((unsigned)grid_rows(rows));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (vec) launch_apply<true>(steps, grid, st, d_img, rows, cols, stride, d_ia, ia_stride, d_mask, mask_stride, hh_factor, K, d_out, out_stride);
    else launch_apply<false>(steps, grid, st, d_img, rows, cols, stride, d_ia, ia_stride, d_mask, mask_stride, hh_factor, K, d_out, out_stride);
    return launched("apply");
}

SID_EXPORT int sid_prep_spatial_mean(int64_t rows, int64_t cols, const double *coeffs, double *d_out, int64_t out_stride,
                                     void *hip_stream)
{
    if (rows < 1 || cols < 1) return fail(SID_PM_ERR_ARG, "bad image shape");
    if (!coeffs) return fail(SID_PM_ERR_ARG, "null coefficients");
    if (int rc = check_plane(d_out, cols, out_stride, "output")) return rc;
    DeviceOf guard(d_out);
    Coef K;
    for (int k = 0; k < 6; ++k) K.c[k] = coeffs[k];
    const dim3 grid((unsigned)grid_rows(rows));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (aligned(d_out, out_stride, 8, 16)) hipLaunchKernelGGL(mean_kernel<true>, grid, dim3(kThreads), 0, st, rows, cols, K, d_out, out_stride);
    else hipLaunchKernelGGL(mean_kernel<false>, grid, dim3(kThreads), 0, st, rows, cols, K, d_out, out_stride);
    return launched("spatial mean");
}

SID_EXPORT int sid_prep_debug_log10(uint32_t first_bits, uint64_t n, uint64_t *counts)
{
    if (!counts) return fail(SID_PM_ERR_ARG, "null output");
    if ((uint64_t)first_bits + n > 0x100000000ull) return fail(SID_PM_ERR_ARG, "range beyond the float32 bit patterns");
    unsigned long long *d = nullptr, h[2] = {0, 0};
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), sizeof h);
    if (e == hipSuccess) e = hipMemset(d, 0, sizeof h);
    if (e == hipSuccess && n > 0) {
        const uint64_t blocks = std::min<uint64_t>((n + kThreads - 1) / kThreads, 256 * 32);
        hipLaunchKernelGGL(log10_sweep_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, nullptr, first_bits, n, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SID_PM_ERR_HIP, "log10 sweep: %s", hipGetErrorString(e));
    counts[0] = h[0]; counts[1] = h[1];
    return SID_PM_OK;
}
