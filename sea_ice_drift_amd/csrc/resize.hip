// resize.hip - downsampling by area average on gfx950 (C ABI and specification: include/sid_resize.h; the first line of get_n,
// n.resize(factor, resample_alg=-1), lib.py:314-316) and the same average as the fused front of the sigma0 preparation
// (prep_pixel.h: dB, HH correction, mask, detrend at the reduced pixel).  A streaming pass: 4 B in per source pixel, 4 B out per
// output pixel (1 B each for uint8).  Every kernel takes one workgroup per output row (grid-stride over rows), so row and
// column are known without a division and any row stride works.
//   *_vec_kernel      whole ratios 2 and 4 (uint8: 2) with aligned rows: a lane loads the 16-byte words of the K source rows
//                     that make one 16-byte word of output (uint8: one word per row, 8 bytes of output), all loads of its
//                     words issued before the first sum
//   *_kernel          any ratio and layout: one output pixel per lane, adjacent lanes on adjacent columns, the weights from
//                     a, b of the header in integer arithmetic
// Both compute the header's sum in the header's order (float64, row-major, no fused multiply-add: -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <numeric>

#include "../../include/sid_resize.h"
#include "host_util.h"
#include "prep_pixel.h"

namespace {

constexpr int kThreads = 256;

struct Axis { int64_t a, b; };           // input length / gcd, output length / gcd

// x / d for 0 <= x < 2^50, 1 <= d <= 2^24: in 32 bits whenever the numerator fits
__device__ __forceinline__ int64_t udiv(int64_t x, int64_t d)
{
    if (d == 1) return x;
    if ((uint64_t)x <= 0xffffffffull) return (int64_t)((uint32_t)x / (uint32_t)d);
    return (int64_t)((uint64_t)x / (uint64_t)d);
}

// Output index j of an axis: [s, e) its span of the fine axis, i0..i1 its source indices
struct Span { int64_t s, e, i0, i1; };
__device__ __forceinline__ Span span_of(int64_t j, Axis A)
{
    Span p;
    p.s = j * A.a; p.e = p.s + A.a;
    p.i0 = udiv(p.s, A.b); p.i1 = udiv(p.e + A.b - 1, A.b) - 1;
    return p;
}
__device__ __forceinline__ int64_t weight(int64_t i, int64_t b, const Span &p)
{
    const int64_t lo = i * b, hi = lo + b;
    return (hi < p.e ? hi : p.e) - (lo > p.s ? lo : p.s);
}

// The float32 result of one output pixel (header: acc = acc + double(wr * wc) * double(x), row-major)
template <bool OMIT>
__device__ __forceinline__ float window_mean(const float *src, int64_t stride, const Span &R, int64_t br, const Span &C, int64_t bc, double total)
{
    double acc = 0.0;
    int64_t used = 0;
    if (br == 1 && bc == 1) {                                // whole ratio: every weight is 1
        for (int64_t i = R.i0; i <= R.i1; ++i) {
            const float *row = src + i * stride;
            for (int64_t k = C.i0; k <= C.i1; ++k) {
                const float x = row[k];
                if (OMIT && x != x) continue;
                acc = acc + (double)x;
                used += 1;
            }
        }
    } else {
        for (int64_t i = R.i0; i <= R.i1; ++i) {
            const float *row = src + i * stride;
            const int64_t wr = weight(i, br, R);
            for (int64_t k = C.i0; k <= C.i1; ++k) {
                const float x = row[k];
                if (OMIT && x != x) continue;
                const int64_t w = wr * weight(k, bc, C);
                const double t = (double)w * (double)x;
                acc = acc + t;
                used += w;
            }
        }
    }
    if (OMIT) return used ? (float)(acc / (double)used) : __int_as_float(0x7fc00000);
    return (float)(acc / total);
}

__device__ __forceinline__ uint8_t window_u8(const uint8_t *src, int64_t stride, const Span &R, int64_t br, const Span &C, int64_t bc,
                                             int64_t total, bool zero_invalid)
{
    int64_t S = 0;
    bool zero = false;
    for (int64_t i = R.i0; i <= R.i1; ++i) {
        const uint8_t *row = src + i * stride;
        const int64_t wr = br == 1 ? 1 : weight(i, br, R);
        for (int64_t k = C.i0; k <= C.i1; ++k) {
            const int64_t x = row[k];
            zero |= x == 0;
            S += wr * (bc == 1 ? 1 : weight(k, bc, C)) * x;
        }
    }
    if (zero_invalid && zero) return 0;
    return (uint8_t)udiv(2 * S + total, 2 * total);          // (S <= 255 total, total <= 2^48)
}

template <bool OMIT>
__global__ __launch_bounds__(kThreads) void resize_f32_kernel(const float *src, int64_t stride, float *dst, int64_t out_rows, int64_t out_cols,
                                                              int64_t dst_stride, Axis AR, Axis AC)
{
    const double total = (double)(AR.a * AC.a);
    for (int64_t r = blockIdx.x; r < out_rows; r += gridDim.x) {
        const Span R = span_of(r, AR);
        float *orow = dst + r * dst_stride;
        for (int64_t c = threadIdx.x; c < out_cols; c += kThreads)
            orow[c] = window_mean<OMIT>(src, stride, R, AR.b, span_of(c, AC), AC.b, total);
    }
}

__global__ __launch_bounds__(kThreads) void resize_u8_kernel(const uint8_t *src, int64_t stride, uint8_t *dst, int64_t out_rows, int64_t out_cols,
                                                             int64_t dst_stride, Axis AR, Axis AC, bool zero_invalid)
{
    const int64_t total = AR.a * AC.a;
    for (int64_t r = blockIdx.x; r < out_rows; r += gridDim.x) {
        const Span R = span_of(r, AR);
        uint8_t *orow = dst + r * dst_stride;
        for (int64_t c = threadIdx.x; c < out_cols; c += kThreads)
            orow[c] = window_u8(src, stride, R, AR.b, span_of(c, AC), AC.b, total, zero_invalid);
    }
}

// ---- whole ratio K on both axes, aligned rows: the K x K float4 words under output word x of output row r
template <int K>
__device__ __forceinline__ void load_block(const float *src, int64_t stride, int64_t r, int64_t x, float4 (&v)[K][K])
{
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float4 *p = reinterpret_cast<const float4 *>(src + (r * K + i) * stride) + x * K;
#pragma unroll
        for (int t = 0; t < K; ++t) v[i][t] = p[t];
    }
}

// the four output pixels of such a block: the header's sum with every weight 1 (acc * 2^-n is acc / 2^n exactly)
template <int K>
__device__ __forceinline__ void mean_block(const float4 (&v)[K][K], float (&o)[4])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const float *f = reinterpret_cast<const float *>(&v[i][0]);
#pragma unroll
            for (int t = 0; t < K; ++t) acc = acc + (double)f[q * K + t];
        }
        o[q] = (float)(acc * (1.0 / (K * K)));
    }
}

template <int K>
__global__ __launch_bounds__(kThreads) void resize_f32_vec_kernel(const float *src, int64_t stride, float *dst, int64_t out_rows, int64_t n4,
                                                                  int64_t dst_stride)
{
    constexpr int U = K == 2 ? 2 : 1;                        // output words per lane and step: 8 (K = 2), 16 (K = 4) loads in flight
    for (int64_t r = blockIdx.x; r < out_rows; r += gridDim.x) {
        float4 *o4 = reinterpret_cast<float4 *>(dst + r * dst_stride);
        for (int64_t base = 0; base < n4; base += kThreads * U) {
            float4 v[U][K][K];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t x = base + u * kThreads + threadIdx.x;
                if (x < n4) load_block<K>(src, stride, r, x, v[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t x = base + u * kThreads + threadIdx.x;
                if (x >= n4) continue;
                float o[4];
                mean_block<K>(v[u], o);
                o4[x] = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    }
}

// uint8, ratio 2: (2 S + T) / (2 T) with T = 4, and the zero rule
__device__ __forceinline__ uint32_t mean_u8_2x2(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, bool zero_invalid)
{
    if (zero_invalid && (p0 == 0 || p1 == 0 || p2 == 0 || p3 == 0)) return 0;
    return (2u * (p0 + p1 + p2 + p3) + 4u) >> 3;
}

// the four bytes of one output dword from two dwords of each of the two source rows
__device__ __forceinline__ uint32_t mean_u8x4(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, bool zero_invalid)
{
    uint32_t o = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t a = q < 2 ? a0 : a1, b = q < 2 ? b0 : b1;
        const int sh = (q & 1) * 16;
        o |= mean_u8_2x2((a >> sh) & 0xffu, (a >> (sh + 8)) & 0xffu, (b >> sh) & 0xffu, (b >> (sh + 8)) & 0xffu, zero_invalid) << (8 * q);
    }
    return o;
}

// A lane loads one 16-byte word of each of the two source rows (adjacent lanes, adjacent words) and stores the 8 bytes they
// make: output rows of an image of 10000 x 10000 bytes start 8-byte aligned, not 16.  The out_cols % 8 last columns one per lane.
__global__ __launch_bounds__(kThreads) void resize_u8_vec_kernel(const uint8_t *src, int64_t stride, uint8_t *dst, int64_t out_rows, int64_t out_cols,
                                                                 int64_t dst_stride, bool zero_invalid)
{
    constexpr int U = 2;                                     // output words per lane and step: 4 loads in flight
    const int64_t n8 = out_cols >> 3;
    for (int64_t r = blockIdx.x; r < out_rows; r += gridDim.x) {
        const uint8_t *s0 = src + (2 * r) * stride, *s1 = s0 + stride;
        const uint4 *r0 = reinterpret_cast<const uint4 *>(s0), *r1 = reinterpret_cast<const uint4 *>(s1);
        uint8_t *orow = dst + r * dst_stride;
        uint2 *o8 = reinterpret_cast<uint2 *>(orow);
        for (int64_t base = 0; base < n8; base += kThreads * U) {
            uint4 a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t x = base + u * kThreads + threadIdx.x;
                if (x < n8) { a[u] = r0[x]; b[u] = r1[x]; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t x = base + u * kThreads + threadIdx.x;
                if (x >= n8) continue;
                o8[x] = make_uint2(mean_u8x4(a[u].x, a[u].y, b[u].x, b[u].y, zero_invalid), mean_u8x4(a[u].z, a[u].w, b[u].z, b[u].w, zero_invalid));
            }
        }
        for (int64_t c = (n8 << 3) + threadIdx.x; c < out_cols; c += kThreads)
            orow[c] = (uint8_t)mean_u8_2x2(s0[2 * c], s0[2 * c + 1], s1[2 * c], s1[2 * c + 1], zero_invalid);
    }
}

// ---- the fused front of the preparation: prep_pixel at the reduced pixel (r, c) of the averaged image and incidence angle
template <bool DB, bool HH, bool MASK, bool MEAN, bool VEC>
__global__ __launch_bounds__(kThreads) void prep_kernel(const float *img, int64_t stride, const float *ia, int64_t ia_stride,
                                                        const uint8_t *mask, int64_t mask_stride, float f, Coef K,
                                                        float *out, int64_t out_rows, int64_t out_cols, int64_t out_stride, Axis AR, Axis AC)
{
    const double total = (double)(AR.a * AC.a);
    for (int64_t r = blockIdx.x; r < out_rows; r += gridDim.x) {
        const uint8_t *mrow = MASK ? mask + r * mask_stride : nullptr;
        float *orow = out + r * out_stride;
        const double dr = (double)r, c2r = MEAN ? K.c[2] * dr : 0.0, c3r2 = MEAN ? K.c[3] * (double)(r * r) : 0.0;
        if (VEC) {                                           // ratio 2 on both axes, out_cols % 4 == 0, every row start aligned (host check)
            const uint32_t *m4 = reinterpret_cast<const uint32_t *>(mrow);
            float4 *o4 = reinterpret_cast<float4 *>(orow);
            const int64_t n4 = out_cols >> 2;
            for (int64_t x = threadIdx.x; x < n4; x += kThreads) {
                float4 v[2][2], a[2][2];
                load_block<2>(img, stride, r, x, v);
                if (HH) load_block<2>(ia, ia_stride, r, x, a);
                const uint32_t m = MASK ? m4[x] : 0u;
                float p[4], q[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
                mean_block<2>(v, p);
                if (HH) mean_block<2>(a, q);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double mu = MEAN ? spatial_mean(K, (x << 2) + k, dr, c2r, c3r2) : 0.0;
                    o[k] = prep_pixel(DB, HH, MASK, MEAN, p[k], q[k], m & (0xffu << (8 * k)), f, mu);
                }
                o4[x] = make_float4(o[0], o[1], o[2], o[3]);
            }
        } else {
            const Span R = span_of(r, AR);
            for (int64_t c = threadIdx.x; c < out_cols; c += kThreads) {
                const Span C = span_of(c, AC);
                const float p = window_mean<false>(img, stride, R, AR.b, C, AC.b, total);
                const float q = HH ? window_mean<false>(ia, ia_stride, R, AR.b, C, AC.b, total) : 0.f;
                const double mu = MEAN ? spatial_mean(K, c, dr, c2r, c3r2) : 0.0;
                orow[c] = prep_pixel(DB, HH, MASK, MEAN, p, q, MASK ? (uint32_t)mrow[c] : 0u, f, mu);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void prep_subsample_kernel(const float *img, int64_t stride, const float *ia, int64_t ia_stride,
                                                                  const uint8_t *mask, int64_t mask_stride, bool db, float f,
                                                                  int64_t step, int64_t nrs, int64_t ncs, Axis AR, Axis AC, float *sub)
{
    const int64_t n = nrs * ncs;
    const double total = (double)(AR.a * AC.a);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int64_t r = (i / ncs) * step, c = (i % ncs) * step;           // (r < out_rows, c < out_cols: nrs = ceil(out_rows / step))
        const Span R = span_of(r, AR), C = span_of(c, AC);
        const float p = window_mean<false>(img, stride, R, AR.b, C, AC.b, total);
        const float q = ia ? window_mean<false>(ia, ia_stride, R, AR.b, C, AC.b, total) : 0.f;
        sub[i] = prep_pixel(db, ia != nullptr, mask != nullptr, false, p, q, mask ? (uint32_t)mask[r * mask_stride + c] : 0u, f, 0.0);
    }
}

// ---- host
int grid_rows(int64_t rows) { return (int)std::max<int64_t>(1, std::min<int64_t>(rows, 256 * 16)); }

Axis axis_of(int64_t n, int64_t m)
{
    const int64_t g = std::gcd(n, m);
    return Axis{n / g, m / g};
}

int check_shapes(int64_t rows, int64_t cols, int64_t out_rows, int64_t out_cols)
{
    if (rows < 1 || cols < 1) return fail(SID_PM_ERR_ARG, "bad image shape %lld x %lld", (long long)rows, (long long)cols);
    if (out_rows < 1 || out_cols < 1) return fail(SID_PM_ERR_ARG, "bad output shape %lld x %lld", (long long)out_rows, (long long)out_cols);
    if (out_rows > rows || out_cols > cols)
        return fail(SID_PM_ERR_ARG, "output %lld x %lld exceeds the input %lld x %lld (downsampling only)", (long long)out_rows,
                    (long long)out_cols, (long long)rows, (long long)cols);
    if (rows > SID_RESIZE_MAX_DIM || cols > SID_RESIZE_MAX_DIM)
        return fail(SID_PM_ERR_UNSUPPORTED, "image %lld x %lld: a dimension above 2^24", (long long)rows, (long long)cols);
    return SID_PM_OK;
}

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

// the whole ratio K (2 or 4) shared by both axes, else 0
int whole_ratio(int64_t rows, int64_t cols, int64_t out_rows, int64_t out_cols)
{
    for (int k : {2, 4})
        if (rows == k * out_rows && cols == k * out_cols) return k;
    return 0;
}

template <bool VEC>
void launch_prep(int steps, dim3 grid, hipStream_t st, const float *img, int64_t stride, const float *ia, int64_t ia_stride,
                 const uint8_t *mask, int64_t mask_stride, float f, const Coef &K, float *out, int64_t out_rows, int64_t out_cols,
                 int64_t out_stride, Axis AR, Axis AC)
{
#define SID_RESIZE_CASE(b) case b: hipLaunchKernelGGL((prep_kernel<((b) & 1) != 0, ((b) & 2) != 0, ((b) & 4) != 0, ((b) & 8) != 0, VEC>), \
        grid, dim3(kThreads), 0, st, img, stride, ia, ia_stride, mask, mask_stride, f, K, out, out_rows, out_cols, out_stride, AR, AC); break;
    switch (steps) {                                         // bit 0 dB, bit 1 HH, bit 2 mask, bit 3 detrend
        SID_RESIZE_CASE(0) SID_RESIZE_CASE(1) SID_RESIZE_CASE(2) SID_RESIZE_CASE(3) SID_RESIZE_CASE(4) SID_RESIZE_CASE(5) SID_RESIZE_CASE(6) SID_RESIZE_CASE(7)
        SID_RESIZE_CASE(8) SID_RESIZE_CASE(9) SID_RESIZE_CASE(10) SID_RESIZE_CASE(11) SID_RESIZE_CASE(12) SID_RESIZE_CASE(13) SID_RESIZE_CASE(14) SID_RESIZE_CASE(15)
    }
#undef SID_RESIZE_CASE
}

}  // namespace

SID_EXPORT const char *sid_resize_last_error(void) { return g_err; }

SID_EXPORT int sid_resize_f32(const float *d_src, int64_t rows, int64_t cols, int64_t stride,
                              float *d_dst, int64_t out_rows, int64_t out_cols, int64_t dst_stride, int nan_omit, void *hip_stream)
{
    if (int rc = check_shapes(rows, cols, out_rows, out_cols)) return rc;
    if (int rc = check_plane(d_src, cols, stride, "source")) return rc;
    if (int rc = check_plane(d_dst, out_cols, dst_stride, "destination")) return rc;
    DeviceOf guard(d_src);
    const dim3 grid((unsigned)grid_rows(out_rows)), block(kThreads);
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const int k = whole_ratio(rows, cols, out_rows, out_cols);
    const bool vec = k && !nan_omit && (out_cols & 3) == 0 && aligned(d_src, stride, 4, 16) && aligned(d_dst, dst_stride, 4, 16);
    const Axis AR = axis_of(rows, out_rows), AC = axis_of(cols, out_cols);
    if (vec && k == 2) hipLaunchKernelGGL(resize_f32_vec_kernel<2>, grid, block, 0, st, d_src, stride, d_dst, out_rows, out_cols >> 2, dst_stride);
    else if (vec) hipLaunchKernelGGL(resize_f32_vec_kernel<4>, grid, block, 0, st, d_src, stride, d_dst, out_rows, out_cols >> 2, dst_stride);
    else if (nan_omit) hipLaunchKernelGGL(resize_f32_kernel<true>, grid, block, 0, st, d_src, stride, d_dst, out_rows, out_cols, dst_stride, AR, AC);
    else hipLaunchKernelGGL(resize_f32_kernel<false>, grid, block, 0, st, d_src, stride, d_dst, out_rows, out_cols, dst_stride, AR, AC);
    return launched("resize float32");
}

SID_EXPORT int sid_resize_u8(const uint8_t *d_src, int64_t rows, int64_t cols, int64_t stride,
                             uint8_t *d_dst, int64_t out_rows, int64_t out_cols, int64_t dst_stride, int zero_invalid, void *hip_stream)
{
    if (int rc = check_shapes(rows, cols, out_rows, out_cols)) return rc;
    if (int rc = check_plane(d_src, cols, stride, "source")) return rc;
    if (int rc = check_plane(d_dst, out_cols, dst_stride, "destination")) return rc;
    DeviceOf guard(d_src);
    const dim3 grid((unsigned)grid_rows(out_rows)), block(kThreads);
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const bool vec = whole_ratio(rows, cols, out_rows, out_cols) == 2 && aligned(d_src, stride, 1, 16) && aligned(d_dst, dst_stride, 1, 8);
    if (vec) hipLaunchKernelGGL(resize_u8_vec_kernel, grid, block, 0, st, d_src, stride, d_dst, out_rows, out_cols, dst_stride, zero_invalid != 0);
    else hipLaunchKernelGGL(resize_u8_kernel, grid, block, 0, st, d_src, stride, d_dst, out_rows, out_cols, dst_stride,
                            axis_of(rows, out_rows), axis_of(cols, out_cols), zero_invalid != 0);
    return launched("resize uint8");
}

SID_EXPORT int sid_resize_prep_apply(const float *d_img, int64_t rows, int64_t cols, int64_t stride,
                                     const float *d_ia, int64_t ia_stride, const uint8_t *d_mask, int64_t mask_stride,
                                     int dB, float hh_factor, const double *coeffs,
                                     float *d_out, int64_t out_rows, int64_t out_cols, int64_t out_stride, void *hip_stream)
{
    if (int rc = check_shapes(rows, cols, out_rows, out_cols)) return rc;
    if (int rc = check_plane(d_img, cols, stride, "image")) return rc;
    if (d_ia) { if (int rc = check_plane(d_ia, cols, ia_stride, "incidence angle")) return rc; }
    if (d_mask) { if (int rc = check_plane(d_mask, out_cols, mask_stride, "mask")) return rc; }
    if (int rc = check_plane(d_out, out_cols, out_stride, "output")) return rc;
    DeviceOf guard(d_img);
    Coef K;
    for (int k = 0; k < 6; ++k) K.c[k] = coeffs ? coeffs[k] : 0.0;
    const int steps = (dB ? 1 : 0) | (d_ia ? 2 : 0) | (d_mask ? 4 : 0) | (coeffs ? 8 : 0);
    const bool vec = whole_ratio(rows, cols, out_rows, out_cols) == 2 && (out_cols & 3) == 0 && aligned(d_img, stride, 4, 16) &&
                     aligned(d_out, out_stride, 4, 16) && (!d_ia || aligned(d_ia, ia_stride, 4, 16)) && (!d_mask || aligned(d_mask, mask_stride, 1, 4));
    const dim3 grid((unsigned)grid_rows(out_rows));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const Axis AR = axis_of(rows, out_rows), AC = axis_of(cols, out_cols);
    if (vec) launch_prep<true>(steps, grid, st, d_img, stride, d_ia, ia_stride, d_mask, mask_stride, hh_factor, K, d_out, out_rows, out_cols, out_stride, AR, AC);
    else launch_prep<false>(steps, grid, st, d_img, stride, d_ia, ia_stride, d_mask, mask_stride, hh_factor, K, d_out, out_rows, out_cols, out_stride, AR, AC);
    return launched("resize + apply");
}

SID_EXPORT int sid_resize_prep_subsample(const float *d_img, int64_t rows, int64_t cols, int64_t stride,
                                         const float *d_ia, int64_t ia_stride, const uint8_t *d_mask, int64_t mask_stride,
                                         int dB, float hh_factor, int64_t step, int64_t out_rows, int64_t out_cols,
                                         float *d_sub, void *hip_stream)
{
    if (int rc = check_shapes(rows, cols, out_rows, out_cols)) return rc;
    if (step < 1) return fail(SID_PM_ERR_ARG, "step must be positive");
    if (int rc = check_plane(d_img, cols, stride, "image")) return rc;
    if (d_ia) { if (int rc = check_plane(d_ia, cols, ia_stride, "incidence angle")) return rc; }
    if (d_mask) { if (int rc = check_plane(d_mask, out_cols, mask_stride, "mask")) return rc; }
    if (!d_sub) return fail(SID_PM_ERR_ARG, "null output");
    DeviceOf guard(d_img);
    const int64_t nrs = (out_rows + step - 1) / step, ncs = (out_cols + step - 1) / step;
    const int64_t blocks = std::min<int64_t>((nrs * ncs + kThreads - 1) / kThreads, 2048);
    hipLaunchKernelGGL(prep_subsample_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(hip_stream),
                       d_img, stride, d_ia, ia_stride, d_mask, mask_stride, dB != 0, hh_factor, step, nrs, ncs,
                       axis_of(rows, out_rows), axis_of(cols, out_cols), d_sub);
    return launched("resize + subsample");
}
