// defor.hip - sea-ice deformation on gfx950 (C ABI: include/sid_defor.h; the reference's libdefor.py).
// One thread per triangle: gather the three corners of x, y, u, v, sides, perimeter and Heron's area, the contour integrals,
// and five structure-of-arrays float64 outputs.  The arithmetic is NumPy's, operation for operation;
// the element arithmetic is defor_elem.h (shared with drift_grid.hip); the side lengths use defor_hypot.h, whose host instance
// serves the host check of sid_defor_debug_hypot(-1, ...).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/sid_defor.h"
#include "defor_elem.h"
#include "host_util.h"

namespace {

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

// Per device, beside the pool's staging block: the index flag and its pinned host copy.  The flag is never cleared: each call
// has its own number and an error is "flag == number".  Calls are serialised by the pool's mutex.
struct Flag {
    uint32_t *d_flag = nullptr, *h_flag = nullptr, gen = 0;
    bool cached() const { return d_flag != nullptr; }
    void free()
    {
        if (d_flag) (void)hipFree(d_flag);
        if (h_flag) (void)hipHostFree(h_flag);
    }
};
using Dev = DevicePool<Flag>::Slot;
DevicePool<Flag> g_pool;

int current_device(int &dev)
{
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return fail(SID_PM_ERR_NODEVICE, "no current HIP device");
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

unsigned blocks(int64_t m) { return (unsigned)((m + kBlock - 1) / kBlock); }

// Launch the triangle kernel and queue the flag's copy; the caller waits for the stream and calls flag_check.
int launch_tri(Dev &d, const double *x, const double *y, const double *u, const double *v, int64_t n, const void *t, int t_int64,
               int64_t m, double *e1, double *e2, double *e3, double *a, double *p, hipStream_t st)
{
    const uint32_t gen = ++d.gen ? d.gen : ++d.gen;                // (0 is the flag's initial value: never a call's number)
    if (t_int64)
        hipLaunchKernelGGL(k_defor_tri<int64_t>, dim3(blocks(m)), dim3(kBlock), 0, st, x, y, u, v, n, (const int64_t *)t, m,
                           e1, e2, e3, a, p, d.d_flag, gen);
    else
        hipLaunchKernelGGL(k_defor_tri<int32_t>, dim3(blocks(m)), dim3(kBlock), 0, st, x, y, u, v, n, (const int32_t *)t, m,
                           e1, e2, e3, a, p, d.d_flag, gen);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d.h_flag, d.d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return SID_PM_OK;
}

int flag_check(const Dev &d)
{
    if (*d.h_flag == d.gen) return fail(SID_DEFOR_ERR_INDEX, "an index of t lies outside [-n, n)");
    return SID_PM_OK;
}

int launch_elems(const double *x, const double *y, const double *u, const double *v, const double *a, int64_t m,
                 double *e1, double *e2, double *e3, hipStream_t st)
{
    hipLaunchKernelGGL(k_defor_elems, dim3(blocks(m)), dim3(kBlock), 0, st, x, y, u, v, a, m, e1, e2, e3);
    HIP_TRY(hipGetLastError());
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

SID_EXPORT int sid_defor_release(int device) { return g_pool.release(device); }

SID_EXPORT int sid_defor_triangulation_device(const double *x, const double *y, const double *u, const double *v, int64_t n,
                                              const void *t, int t_int64, int64_t m,
                                              double *e1, double *e2, double *e3, double *a, double *p, void *hip_stream)
{
    if (int rc = check_tri_args(x, y, u, v, n, t, m, e1, e2, e3, a, p)) return rc;
    if (m == 0) return SID_PM_OK;
    int dev = 0;
    if (int rc = current_device(dev)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(g_pool.mutex(dev));
    Dev &d = g_pool.slot[dev];
    if (int rc = flag_ready(d)) return rc;
    if (int rc = launch_tri(d, x, y, u, v, n, t, t_int64, m, e1, e2, e3, a, p, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return flag_check(d);
}

SID_EXPORT int sid_defor_elems_device(const double *x, const double *y, const double *u, const double *v, const double *a, int64_t m,
                                      double *e1, double *e2, double *e3, void *hip_stream)
{
    if (int rc = check_elem_args(x, y, u, v, a, m, e1, e2, e3)) return rc;
    if (m == 0) return SID_PM_OK;
    return launch_elems(x, y, u, v, a, m, e1, e2, e3, reinterpret_cast<hipStream_t>(hip_stream));
}

SID_EXPORT int sid_defor_triangulation(int device, const double *x, const double *y, const double *u, const double *v, int64_t n,
                                       const void *t, int t_int64, int64_t m,
                                       double *e1, double *e2, double *e3, double *a, double *p)
{
    if (int rc = check_tri_args(x, y, u, v, n, t, m, e1, e2, e3, a, p)) return rc;
    if (m == 0) return SID_PM_OK;
    Staging s;
    if (!s.enter(g_pool, device)) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    Dev &d = g_pool.slot[device];
    const size_t nb = sizeof(double) * (size_t)n, mb = sizeof(double) * (size_t)m, tb = (t_int64 ? 8 : 4) * 3 * (size_t)m;
    double *in[4], *out[5];
    unsigned char *dt;
    if (int rc = flag_ready(d)) return rc;
    if (int rc = g_pool.carve(device, [&](Carver &c) {
            for (double *&q : in) q = c.take<double>((size_t)n);
            dt = c.take<unsigned char>(tb);
            for (double *&q : out) q = c.take<double>((size_t)m);
        }))
        return rc;
    const double *src[4] = {x, y, u, v};
    for (int j = 0; j < 4; ++j) HIP_TRY(hipMemcpyAsync(in[j], src[j], nb, hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(dt, t, tb, hipMemcpyHostToDevice, 0));
    if (int rc = launch_tri(d, in[0], in[1], in[2], in[3], n, dt, t_int64, m, out[0], out[1], out[2], out[3], out[4], 0)) return rc;
    double *dst[5] = {e1, e2, e3, a, p};
    for (int j = 0; j < 5; ++j) HIP_TRY(hipMemcpyAsync(dst[j], out[j], mb, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipStreamSynchronize(0));
    s.done();
    return flag_check(d);
}

SID_EXPORT int sid_defor_elems(int device, const double *x, const double *y, const double *u, const double *v, const double *a, int64_t m,
                               double *e1, double *e2, double *e3)
{
    if (int rc = check_elem_args(x, y, u, v, a, m, e1, e2, e3)) return rc;
    if (m == 0) return SID_PM_OK;
    Staging s;
    if (!s.enter(g_pool, device)) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    const size_t mb = sizeof(double) * (size_t)m;
    double *in[4], *da, *out[3];                                         // x, y, u, v [3][m] each, then a, then e1, e2, e3
    if (int rc = g_pool.carve(device, [&](Carver &c) {
            for (double *&q : in) q = c.take<double>(3 * (size_t)m);
            da = c.take<double>((size_t)m);
            for (double *&q : out) q = c.take<double>((size_t)m);
        }))
        return rc;
    const double *src[4] = {x, y, u, v};
    for (int j = 0; j < 4; ++j) HIP_TRY(hipMemcpyAsync(in[j], src[j], 3 * mb, hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(da, a, mb, hipMemcpyHostToDevice, 0));
    if (int rc = launch_elems(in[0], in[1], in[2], in[3], da, m, out[0], out[1], out[2], 0)) return rc;
    double *dst[3] = {e1, e2, e3};
    for (int j = 0; j < 3; ++j) HIP_TRY(hipMemcpyAsync(dst[j], out[j], mb, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipStreamSynchronize(0));
    s.done();
    return SID_PM_OK;
}

SID_EXPORT int sid_defor_debug_hypot(int device, const double *x, const double *y, int64_t n, double *out)
{
    if (n < 0 || n > kMaxElems || (n > 0 && (!x || !y || !out))) return fail(SID_PM_ERR_ARG, "bad argument");
    if (n == 0) return SID_PM_OK;
    if (device == -1) {
        for (int64_t i = 0; i < n; ++i) out[i] = sid_defor::hypot64(x[i], y[i]);
        return SID_PM_OK;
    }
    Staging s;
    if (!s.enter(g_pool, device)) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    const size_t nb = sizeof(double) * (size_t)n;
    double *dx, *dy, *dout;
    if (int rc = g_pool.carve(device, [&](Carver &c) { dx = c.take<double>((size_t)n); dy = c.take<double>((size_t)n); dout = c.take<double>((size_t)n); }))
        return rc;
    HIP_TRY(hipMemcpyAsync(dx, x, nb, hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(dy, y, nb, hipMemcpyHostToDevice, 0));
    hipLaunchKernelGGL(k_defor_hypot, dim3(blocks(n)), dim3(kBlock), 0, 0, dx, dy, n, dout);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout, nb, hipMemcpyDeviceToHost));
    s.done();
    return SID_PM_OK;
}
