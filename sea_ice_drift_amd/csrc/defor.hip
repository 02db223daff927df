// defor.hip - sea-ice deformation on gfx950 (C ABI: include/sid_defor.h; the reference's libdefor.py).
// One thread per triangle: gather the three corners of x, y, u, v, sides, perimeter and Heron's area, the contour integrals,
// and five structure-of-arrays float64 outputs.  The arithmetic is NumPy's, operation for operation;
// the element arithmetic is defor_elem.h (shared with drift_grid.hip); the side lengths use defor_hypot.h, whose host instance
// serves the host check of sid_defor_debug_hypot(-1, ...).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <mutex>

#include "../../include/sid_defor.h"
#include "../../include/sid_pm.h"
#include "defor_elem.h"

#define SID_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

thread_local char g_err[256] = "";
int fail(int code, const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return code;
}

constexpr int kBlock = 256;
constexpr int64_t kMaxElems = (int64_t)0x7fffffff * kBlock;     // grid.x limit

// Corner index k of a triangle as NumPy's fancy indexing reads it: i < 0 wraps once; outside [0, n) is an error
template <typename I>
__device__ __forceinline__ bool wrap(I raw, int64_t n, int64_t &i)
{
    i = (int64_t)raw;
    if (i < 0) i += n;
    return i >= 0 && i < n;
}

// get_deformation_on_triangulation.  An out-of-range index stores `gen` (the call's number) into *flag and NaN into the
// element's outputs; nothing is read through it.
template <typename I>
__global__ __launch_bounds__(kBlock) void k_defor_tri(const double *__restrict__ x, const double *__restrict__ y,
                                                      const double *__restrict__ u, const double *__restrict__ v, int64_t n,
                                                      const I *__restrict__ t, int64_t m,
                                                      double *__restrict__ e1, double *__restrict__ e2, double *__restrict__ e3,
                                                      double *__restrict__ ao, double *__restrict__ po, uint32_t *flag, uint32_t gen)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= m) return;
    int64_t c[3];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) ok = wrap(t[3 * k + j], n, c[j]) && ok;
    if (!ok) {
        *flag = gen;
        e1[k] = NAN; e2[k] = NAN; e3[k] = NAN; ao[k] = NAN; po[k] = NAN;
        return;
    }
    double xs[3], ys[3], us[3], vs[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { xs[j] = x[c[j]]; ys[j] = y[c[j]]; us[j] = u[c[j]]; vs[j] = v[c[j]]; }
    double r1, r2, r3, a, p;
    sid_defor::triangle(xs, ys, us, vs, r1, r2, r3, a, p);
    e1[k] = r1; e2[k] = r2; e3[k] = r3; ao[k] = a; po[k] = p;
}

// get_deformation_elems: x, y, u, v [3][m], a [m]
__global__ __launch_bounds__(kBlock) void k_defor_elems(const double *__restrict__ x, const double *__restrict__ y,
                                                        const double *__restrict__ u, const double *__restrict__ v,
                                                        const double *__restrict__ a, int64_t m,
                                                        double *__restrict__ e1, double *__restrict__ e2, double *__restrict__ e3)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= m) return;
    double xs[3], ys[3], us[3], vs[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { xs[j] = x[j * m + k]; ys[j] = y[j * m + k]; us[j] = u[j * m + k]; vs[j] = v[j * m + k]; }
    double r1, r2, r3;
    sid_defor::elem(xs, ys, us, vs, a[k], r1, r2, r3);
    e1[k] = r1; e2[k] = r2; e3[k] = r3;
}

__global__ __launch_bounds__(kBlock) void k_defor_hypot(const double *__restrict__ x, const double *__restrict__ y, int64_t n,
                                                        double *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < n) out[k] = sid_defor::hypot64(x[k], y[k]);
}

#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { rc = fail(SID_PM_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_)); goto done; } } while (0)

// Per device: a grow-only scratch block for the host-buffer entry points (no hipMalloc / hipFree per call), the index flag
// and its pinned host copy.  The flag is never cleared: each call has its own number and an error is "flag == number".
// Calls are serialised by the mutex.
struct Dev { unsigned char *blk = nullptr; size_t cap = 0; uint32_t *d_flag = nullptr; uint32_t *h_flag = nullptr; uint32_t gen = 0; };
std::mutex g_mu;
Dev g_dev[16];

int current_device(int &dev)
{
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return fail(SID_PM_ERR_NODEVICE, "no current HIP device");
    return SID_PM_OK;
}

int pick_device(int device, int &prev)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n || device >= 16) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    (void)hipGetDevice(&prev); (void)hipSetDevice(device);
    return SID_PM_OK;
}

int flag_ready(Dev &d)
{
    if (d.d_flag) return SID_PM_OK;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d.d_flag), sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(d.d_flag, 0, sizeof(uint32_t));
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&d.h_flag), sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) {
        if (d.d_flag) (void)hipFree(d.d_flag);
        d.d_flag = nullptr; d.h_flag = nullptr;
        return fail(e == hipErrorOutOfMemory ? SID_PM_ERR_NOMEM : SID_PM_ERR_HIP, "index flag: %s", hipGetErrorString(e));
    }
    return SID_PM_OK;
}

int reserve(Dev &d, size_t bytes)
{
    if (d.cap >= bytes) return SID_PM_OK;
    if (d.blk) (void)hipFree(d.blk);
    d.blk = nullptr; d.cap = 0;
    const size_t want = bytes + bytes / 4;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d.blk), want);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SID_PM_ERR_NOMEM : SID_PM_ERR_HIP, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
    d.cap = want;
    return SID_PM_OK;
}

size_t up(size_t b) { return (b + 255) / 256 * 256; }

unsigned blocks(int64_t m) { return (unsigned)((m + kBlock - 1) / kBlock); }

// Launch the triangle kernel and queue the flag's copy; the caller waits for the stream and calls flag_check.
int launch_tri(Dev &d, const double *x, const double *y, const double *u, const double *v, int64_t n, const void *t, int t_int64,
               int64_t m, double *e1, double *e2, double *e3, double *a, double *p, hipStream_t st)
{
    int rc = SID_PM_OK;
    const uint32_t gen = ++d.gen ? d.gen : ++d.gen;                // (0 is the flag's initial value: never a call's number)
    if (t_int64)
        hipLaunchKernelGGL(k_defor_tri<int64_t>, dim3(blocks(m)), dim3(kBlock), 0, st, x, y, u, v, n, (const int64_t *)t, m,
                           e1, e2, e3, a, p, d.d_flag, gen);
    else
        hipLaunchKernelGGL(k_defor_tri<int32_t>, dim3(blocks(m)), dim3(kBlock), 0, st, x, y, u, v, n, (const int32_t *)t, m,
                           e1, e2, e3, a, p, d.d_flag, gen);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d.h_flag, d.d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
done:
    return rc;
}

int flag_check(const Dev &d)
{
    if (*d.h_flag == d.gen) return fail(SID_DEFOR_ERR_INDEX, "an index of t lies outside [-n, n)");
    return SID_PM_OK;
}

int check_tri_args(const void *x, const void *y, const void *u, const void *v, int64_t n, const void *t, int64_t m,
                   const void *e1, const void *e2, const void *e3, const void *a, const void *p)
{
    if (m < 0 || n < 0 || m > kMaxElems) return fail(SID_PM_ERR_ARG, "bad sizes (n = %lld, m = %lld)", (long long)n, (long long)m);
    if (m > 0 && n == 0) return fail(SID_DEFOR_ERR_INDEX, "an index of t lies outside [-n, n) (n = 0)");
    if (m > 0 && (!x || !y || !u || !v || !t || !e1 || !e2 || !e3 || !a || !p)) return fail(SID_PM_ERR_ARG, "null pointer");
    return SID_PM_OK;
}

int check_elem_args(const void *x, const void *y, const void *u, const void *v, const void *a, int64_t m,
                    const void *e1, const void *e2, const void *e3)
{
    if (m < 0 || m > kMaxElems) return fail(SID_PM_ERR_ARG, "bad size (m = %lld)", (long long)m);
    if (m > 0 && (!x || !y || !u || !v || !a || !e1 || !e2 || !e3)) return fail(SID_PM_ERR_ARG, "null pointer");
    return SID_PM_OK;
}

}  // namespace

SID_EXPORT const char *sid_defor_last_error(void) { return g_err; }

SID_EXPORT int sid_defor_release(int device)
{
    std::lock_guard<std::mutex> lock(g_mu);
    int prev = 0;
    (void)hipGetDevice(&prev);
    for (int i = 0; i < 16; ++i) {
        if (device >= 0 && i != device) continue;
        Dev &d = g_dev[i];
        if (!d.blk && !d.d_flag) continue;
        (void)hipSetDevice(i);
        if (d.blk) (void)hipFree(d.blk);
        if (d.d_flag) (void)hipFree(d.d_flag);
        if (d.h_flag) (void)hipHostFree(d.h_flag);
        d = Dev();
    }
    (void)hipSetDevice(prev);
    return SID_PM_OK;
}

SID_EXPORT int sid_defor_triangulation_device(const double *x, const double *y, const double *u, const double *v, int64_t n,
                                              const void *t, int t_int64, int64_t m,
                                              double *e1, double *e2, double *e3, double *a, double *p, void *hip_stream)
{
    if (int rc0 = check_tri_args(x, y, u, v, n, t, m, e1, e2, e3, a, p)) return rc0;
    if (m == 0) return SID_PM_OK;
    int dev = 0;
    if (int rc0 = current_device(dev)) return rc0;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    int rc = SID_PM_OK;
    std::lock_guard<std::mutex> lock(g_mu);
    Dev &d = g_dev[dev];
    if ((rc = flag_ready(d))) return rc;
    if ((rc = launch_tri(d, x, y, u, v, n, t, t_int64, m, e1, e2, e3, a, p, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    rc = flag_check(d);
done:
    return rc;
}

SID_EXPORT int sid_defor_elems_device(const double *x, const double *y, const double *u, const double *v, const double *a, int64_t m,
                                      double *e1, double *e2, double *e3, void *hip_stream)
{
    if (int rc0 = check_elem_args(x, y, u, v, a, m, e1, e2, e3)) return rc0;
    if (m == 0) return SID_PM_OK;
    int rc = SID_PM_OK;
    hipLaunchKernelGGL(k_defor_elems, dim3(blocks(m)), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(hip_stream),
                       x, y, u, v, a, m, e1, e2, e3);
    HIP_TRY(hipGetLastError());
done:
    return rc;
}

SID_EXPORT int sid_defor_triangulation(int device, const double *x, const double *y, const double *u, const double *v, int64_t n,
                                       const void *t, int t_int64, int64_t m,
                                       double *e1, double *e2, double *e3, double *a, double *p)
{
    if (int rc0 = check_tri_args(x, y, u, v, n, t, m, e1, e2, e3, a, p)) return rc0;
    if (m == 0) return SID_PM_OK;
    int prev = 0;
    if (int rc0 = pick_device(device, prev)) return rc0;
    int rc = SID_PM_OK;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        Dev &d = g_dev[device];
        const size_t nb = sizeof(double) * (size_t)n, mb = sizeof(double) * (size_t)m, tb = (t_int64 ? 8 : 4) * 3 * (size_t)m;
        double *dx, *dy, *du, *dv, *out;
        unsigned char *dt;
        if ((rc = flag_ready(d)) || (rc = reserve(d, 4 * up(nb) + up(tb) + 5 * up(mb)))) goto done;
        dx = reinterpret_cast<double *>(d.blk); dy = dx + up(nb) / 8; du = dy + up(nb) / 8; dv = du + up(nb) / 8;
        dt = reinterpret_cast<unsigned char *>(dv + up(nb) / 8);
        out = reinterpret_cast<double *>(dt + up(tb));
        HIP_TRY(hipMemcpyAsync(dx, x, nb, hipMemcpyHostToDevice, 0));
        HIP_TRY(hipMemcpyAsync(dy, y, nb, hipMemcpyHostToDevice, 0));
        HIP_TRY(hipMemcpyAsync(du, u, nb, hipMemcpyHostToDevice, 0));
        HIP_TRY(hipMemcpyAsync(dv, v, nb, hipMemcpyHostToDevice, 0));
        HIP_TRY(hipMemcpyAsync(dt, t, tb, hipMemcpyHostToDevice, 0));
        {
            const size_t o = up(mb) / 8;
            if ((rc = launch_tri(d, dx, dy, du, dv, n, dt, t_int64, m, out, out + o, out + 2 * o, out + 3 * o, out + 4 * o, 0))) goto done;
            double *dst[5] = {e1, e2, e3, a, p};
            for (int j = 0; j < 5; ++j) HIP_TRY(hipMemcpyAsync(dst[j], out + j * o, mb, hipMemcpyDeviceToHost, 0));
        }
        HIP_TRY(hipStreamSynchronize(0));
        rc = flag_check(d);
    }
done:
    (void)hipSetDevice(prev);
    return rc;
}

SID_EXPORT int sid_defor_elems(int device, const double *x, const double *y, const double *u, const double *v, const double *a, int64_t m,
                               double *e1, double *e2, double *e3)
{
    if (int rc0 = check_elem_args(x, y, u, v, a, m, e1, e2, e3)) return rc0;
    if (m == 0) return SID_PM_OK;
    int prev = 0;
    if (int rc0 = pick_device(device, prev)) return rc0;
    int rc = SID_PM_OK;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        Dev &d = g_dev[device];
        const size_t mb = sizeof(double) * (size_t)m, o = up(mb) / 8, o3 = up(3 * mb) / 8;
        double *in, *out;
        if ((rc = reserve(d, 4 * up(3 * mb) + 4 * up(mb)))) goto done;
        in = reinterpret_cast<double *>(d.blk);                          // x, y, u, v [3][m] each, then a, then e1, e2, e3
        out = in + 4 * o3 + o;
        {
            const double *src[4] = {x, y, u, v};
            for (int j = 0; j < 4; ++j) HIP_TRY(hipMemcpyAsync(in + j * o3, src[j], 3 * mb, hipMemcpyHostToDevice, 0));
            HIP_TRY(hipMemcpyAsync(in + 4 * o3, a, mb, hipMemcpyHostToDevice, 0));
        }
        hipLaunchKernelGGL(k_defor_elems, dim3(blocks(m)), dim3(kBlock), 0, 0, in, in + o3, in + 2 * o3, in + 3 * o3, in + 4 * o3, m,
                           out, out + o, out + 2 * o);
        HIP_TRY(hipGetLastError());
        {
            double *dst[3] = {e1, e2, e3};
            for (int j = 0; j < 3; ++j) HIP_TRY(hipMemcpyAsync(dst[j], out + j * o, mb, hipMemcpyDeviceToHost, 0));
        }
        HIP_TRY(hipStreamSynchronize(0));
    }
done:
    (void)hipSetDevice(prev);
    return rc;
}

SID_EXPORT int sid_defor_debug_hypot(int device, const double *x, const double *y, int64_t n, double *out)
{
    if (n < 0 || n > kMaxElems || (n > 0 && (!x || !y || !out))) return fail(SID_PM_ERR_ARG, "bad argument");
    if (n == 0) return SID_PM_OK;
    if (device == -1) {
        for (int64_t i = 0; i < n; ++i) out[i] = sid_defor::hypot64(x[i], y[i]);
        return SID_PM_OK;
    }
    int prev = 0;
    if (int rc0 = pick_device(device, prev)) return rc0;
    int rc = SID_PM_OK;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        Dev &d = g_dev[device];
        const size_t nb = sizeof(double) * (size_t)n, o = up(nb) / 8;
        double *dx;
        if ((rc = reserve(d, 3 * up(nb)))) goto done;
        dx = reinterpret_cast<double *>(d.blk);
        HIP_TRY(hipMemcpyAsync(dx, x, nb, hipMemcpyHostToDevice, 0));
        HIP_TRY(hipMemcpyAsync(dx + o, y, nb, hipMemcpyHostToDevice, 0));
        hipLaunchKernelGGL(k_defor_hypot, dim3(blocks(n)), dim3(kBlock), 0, 0, dx, dx + o, n, dx + 2 * o);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out, dx + 2 * o, nb, hipMemcpyDeviceToHost));
    }
done:
    (void)hipSetDevice(prev);
    return rc;
}
