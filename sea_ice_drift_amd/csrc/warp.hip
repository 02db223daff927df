// warp.hip - piecewise-affine warp of an image along a drift grid on gfx950 (C ABI: include/sid_warp.h).
// The per-cell and per-pixel arithmetic is warp_pixel.h, compiled here for the device and for the host instance (device = -1)
// alike.  One call queues, on one stream:
//   k_warp_fill   a first pass of its own over every wanted output: fill / 0 / NaN, 16 bytes per thread where the row allows
//   k_warp_count  one thread per grid cell: the number of work items (16 x 64 pixel tiles of the cell's clipped pixel box)
//   k_warp_scan   one workgroup: the counts to exclusive offsets in place, the total behind them
//   k_warp_walk   a fixed number of workgroups walk the item list: item -> cell by bisection of the offsets, the cell's
//                 constants once, then each wavefront one row of 64 pixels at a time (stores along columns)
// The host never sees a node coordinate, the work of a workgroup per item is one tile whatever the cell size, and since a
// pixel has one owner the order of the items does not reach the result.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/sid_grid.h"
#include "../../include/sid_warp.h"
#include "host_util.h"
#include "warp_pixel.h"

namespace {

using sid_warp::Cell;
using sid_warp::Images;
using sid_warp::Nodes;
using sid_warp::Tri;

static_assert(sid_warp::kTileRows == SID_WARP_TILE_ROWS && sid_warp::kTileCols == SID_WARP_TILE_COLS, "tile constants of sid_warp.h");
static_assert(sid_warp::kU8 == SID_WARP_U8 && sid_warp::kF32 == SID_WARP_F32 && sid_warp::kKeepZero == SID_WARP_KEEP_ZERO, "codes of sid_warp.h");
static_assert(sid_grid::kShorter == SID_GRID_DIAG_SHORTER && sid_grid::kMain == SID_GRID_DIAG_MAIN && sid_grid::kAnti == SID_GRID_DIAG_ANTI,
              "diagonal codes of sid_grid.h");

constexpr int kBlock = 256, kWaves = kBlock / 64, kScanBlock = 1024, kScanPer = 4;
static_assert(sid_warp::kTileCols == 64 && sid_warp::kTileRows % kWaves == 0, "one wavefront per tile row");

// ---------------------------------------------------------------- fill
// `rows` rows of `row_bytes` bytes, `pitch` bytes apart, set to the 4-byte pattern `pat` (phase: the address modulo 4, so a
// uint8 plane takes a replicated byte and a float plane, 4-byte aligned, its bits).  Piece 0 of a row is the bytes before the
// first 16-byte boundary, piece j > 0 the j-th 16 bytes after it (the last one may be short).
__global__ __launch_bounds__(kBlock) void k_warp_fill(unsigned char *__restrict__ base, int64_t pitch, int64_t row_bytes,
                                                      int64_t rows, uint32_t pat)
{
    const int64_t per_row = row_bytes / 16 + 2, total = rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / per_row, j = i - r * per_row;
        unsigned char *p = base + r * pitch;
        int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15);
        if (head > row_bytes) head = row_bytes;
        const int64_t b0 = j == 0 ? 0 : head + 16 * (j - 1);
        int64_t b1 = j == 0 ? head : b0 + 16;
        if (b1 > row_bytes) b1 = row_bytes;
        if (b0 >= b1) continue;
        if (j > 0 && b1 - b0 == 16) {
            *reinterpret_cast<uint4 *>(p + b0) = make_uint4(pat, pat, pat, pat);
        } else {
            for (int64_t b = b0; b < b1; ++b) p[b] = (unsigned char)(pat >> (8 * (reinterpret_cast<uintptr_t>(p + b) & 3)));
        }
    }
}

void host_fill(unsigned char *base, int64_t pitch, int64_t row_bytes, int64_t rows, uint32_t pat)
{
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t b = 0; b < row_bytes; ++b) base[r * pitch + b] = (unsigned char)(pat >> (8 * (b & 3)));
}

// ---------------------------------------------------------------- items
__global__ __launch_bounds__(kBlock) void k_warp_count(Nodes g, int64_t rows_o, int64_t cols_o, int64_t cells, int64_t *__restrict__ off)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= cells) return;
    double X[4], Y[4], XS[4], YS[4];
    int32_t ids[4];
    const unsigned usable = sid_warp::ring(g, k, X, Y, XS, YS, ids);
    int64_t r_lo, r_hi, c_lo, c_hi;
    off[k] = sid_warp::box(X, Y, usable, rows_o, cols_o, r_lo, r_hi, c_lo, c_hi) ? sid_warp::tiles(r_lo, r_hi, c_lo, c_hi) : 0;
}

// off[0..n) counts -> exclusive offsets in place, off[n] = their sum.  One workgroup: the grids are small beside the images.
__global__ __launch_bounds__(kScanBlock) void k_warp_scan(int64_t *__restrict__ off, int64_t n)
{
    __shared__ int64_t s[kScanBlock];
    const int t = threadIdx.x;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += (int64_t)kScanBlock * kScanPer) {
        const int64_t i0 = base + (int64_t)kScanPer * t;
        int64_t v[kScanPer], sum = 0;
#pragma unroll
        for (int j = 0; j < kScanPer; ++j) {
            v[j] = i0 + j < n ? off[i0 + j] : 0;
            sum += v[j];
        }
        s[t] = sum;
        __syncthreads();
        for (int d = 1; d < kScanBlock; d <<= 1) {
            const int64_t add = t >= d ? s[t - d] : 0;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        int64_t run = carry + s[t] - sum;
#pragma unroll
        for (int j = 0; j < kScanPer; ++j)
            if (i0 + j < n) {
                off[i0 + j] = run;
                run += v[j];
            }
        carry += s[kScanBlock - 1];
        __syncthreads();
    }
    if (t == 0) off[n] = carry;
}

__device__ __forceinline__ int64_t uniform(int64_t v)          // a value every thread of the workgroup holds: keep it scalar
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// A fixed number of workgroups walk the item list, workgroup b the items b, b + G, b + 2 G...: neighbouring workgroups work on
// neighbouring tiles.  Per item: the cell by bisection of the offsets, its ring, then triangle by triangle (a pixel has one
// owner, so only one triangle's constants are live at a time) every wavefront one row of 64 pixels after the other.
template <class T>
__global__ __launch_bounds__(kBlock) void k_warp_walk(Nodes g, Images im, const int64_t *__restrict__ off, int64_t cells)
{
    const int64_t total = off[cells];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {
        int64_t lo = 0, hi = cells;                              // off[lo] <= it < off[hi]: the cell that holds item `it`
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (off[mid] <= it) lo = mid; else hi = mid;
        }
        const int64_t k = uniform(lo), local = uniform(it - off[lo]);
        Cell cs;
        if (!sid_warp::setup(g, k, im.rows_o, im.cols_o, cs)) continue;       // (a cell with items has a box)
        const int64_t across = sid_warp::tiles_across(cs.c_lo, cs.c_hi), tr = local / across, tc = local - tr * across;
        const int64_t c = cs.c_lo + tc * sid_warp::kTileCols + lane;
        if (c > cs.c_hi) continue;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            Tri t;
            if (!sid_warp::setup_tri(cs, s, t)) continue;
            for (int q = wave; q < sid_warp::kTileRows; q += kWaves) {
                const int64_t r = cs.r_lo + tr * sid_warp::kTileRows + q;
                if (r > cs.r_hi) break;
                sid_warp::pixel<T>(t, im, r, c);
            }
        }
    }
}

template <class T>
void host_walk(const Nodes &g, const Images &im)
{
    const int64_t cells = (g.rows - 1) * (g.cols - 1);
    for (int64_t k = 0; k < cells; ++k) {
        Cell cs;
        if (!sid_warp::setup(g, k, im.rows_o, im.cols_o, cs)) continue;
        for (int s = 0; s < 2; ++s) {
            Tri t;
            if (!sid_warp::setup_tri(cs, s, t)) continue;
            for (int64_t r = cs.r_lo; r <= cs.r_hi; ++r)
                for (int64_t c = cs.c_lo; c <= cs.c_hi; ++c) sid_warp::pixel<T>(t, im, r, c);
        }
    }
}

// ---------------------------------------------------------------- arguments
uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

struct Fill { uint32_t out, nan; };

Fill fill_patterns(int dtype, double fill)
{
    Fill f;
    f.out = dtype == SID_WARP_U8 ? 0x01010101u * (uint32_t)(uint8_t)fill : bits_of((float)fill);
    f.nan = 0x7fc00000u;
    return f;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

size_t plane_bytes(int64_t rows, int64_t cols, int64_t stride, size_t es)
{
    return rows > 0 && cols > 0 ? ((size_t)(rows - 1) * (size_t)stride + (size_t)cols) * es : 0;
}

int check_args(const void *x, const void *y, const void *xs, const void *ys, int64_t grid_rows, int64_t grid_cols,
               const void *src, int dtype, int64_t rows_s, int64_t cols_s, int64_t src_stride, int64_t rows_o, int64_t cols_o,
               int order, double fill, int diagonal, uint32_t flags, const void *out, int64_t out_stride, const void *covered,
               const void *map_x, const void *map_y)
{
    if (dtype != SID_WARP_U8 && dtype != SID_WARP_F32) return fail(SID_PM_ERR_ARG, "unknown dtype code %d", dtype);
    if (order != 0 && order != 1) return fail(SID_PM_ERR_ARG, "order must be 0 or 1 (got %d)", order);
    if (diagonal != SID_GRID_DIAG_SHORTER && diagonal != SID_GRID_DIAG_MAIN && diagonal != SID_GRID_DIAG_ANTI)
        return fail(SID_PM_ERR_ARG, "unknown diagonal code %d", diagonal);
    if (flags & ~SID_WARP_KEEP_ZERO) return fail(SID_PM_ERR_ARG, "unknown flags 0x%x", flags);
    if ((flags & SID_WARP_KEEP_ZERO) && dtype == SID_WARP_F32) return fail(SID_PM_ERR_ARG, "SID_WARP_KEEP_ZERO is for uint8 images");
    if (dtype == SID_WARP_U8 && !(fill >= 0.0 && fill <= 255.0 && fill == floor(fill)))
        return fail(SID_PM_ERR_ARG, "fill %g is not a uint8 value", fill);
    if (grid_rows < 0 || grid_cols < 0 || rows_s < 0 || cols_s < 0 || rows_o < 0 || cols_o < 0)
        return fail(SID_PM_ERR_ARG, "negative size (grid %lld x %lld, source %lld x %lld, output %lld x %lld)", (long long)grid_rows,
                    (long long)grid_cols, (long long)rows_s, (long long)cols_s, (long long)rows_o, (long long)cols_o);
    if (grid_rows > 0 && grid_cols > 0x7fffffffLL / grid_rows)
        return fail(SID_PM_ERR_UNSUPPORTED, "grid_rows * grid_cols >= 2^31 (%lld x %lld)", (long long)grid_rows, (long long)grid_cols);
    if (rows_s > 0x7fffffffLL || cols_s > 0x7fffffffLL || rows_o > 0x7fffffffLL || cols_o > 0x7fffffffLL)
        return fail(SID_PM_ERR_UNSUPPORTED, "an image axis >= 2^31 (source %lld x %lld, output %lld x %lld)", (long long)rows_s,
                    (long long)cols_s, (long long)rows_o, (long long)cols_o);
    if (!x || !y || !xs || !ys) return fail(SID_PM_ERR_ARG, "null node grid");
    if (!out && !covered && !map_x && !map_y) return fail(SID_PM_ERR_ARG, "no output");
    if (out && !src) return fail(SID_PM_ERR_ARG, "out without a source image");
    if (src && src_stride < cols_s) return fail(SID_PM_ERR_ARG, "src_stride %lld < cols_s %lld", (long long)src_stride, (long long)cols_s);
    if (out && out_stride < cols_o) return fail(SID_PM_ERR_ARG, "out_stride %lld < cols_o %lld", (long long)out_stride, (long long)cols_o);
    const size_t es = dtype == SID_WARP_U8 ? 1 : 4;
    if (src && out && overlap(src, plane_bytes(rows_s, cols_s, src_stride, es), out, plane_bytes(rows_o, cols_o, out_stride, es)))
        return fail(SID_PM_ERR_ARG, "out overlaps the source image");
    return SID_PM_OK;
}

// ---------------------------------------------------------------- launches
unsigned blocks_for(int64_t threads, int64_t cap)
{
    const int64_t b = (threads + kBlock - 1) / kBlock;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

int launch_fill(void *base, int64_t pitch, int64_t row_bytes, int64_t rows, uint32_t pat, int cus, hipStream_t st)
{
    if (!base || rows == 0 || row_bytes == 0) return SID_PM_OK;
    hipLaunchKernelGGL(k_warp_fill, dim3(blocks_for(rows * (row_bytes / 16 + 2), (int64_t)cus * 32)), dim3(kBlock), 0, st,
                       static_cast<unsigned char *>(base), pitch, row_bytes, rows, pat);
    HIP_TRY(hipGetLastError());
    return SID_PM_OK;
}

size_t cell_count(int64_t grid_rows, int64_t grid_cols)
{
    return grid_rows >= 2 && grid_cols >= 2 ? (size_t)((grid_rows - 1) * (grid_cols - 1)) : 0;
}

// All of one call; `off` holds (cells + 1) int64
int launch_all(const Nodes &g, const Images &im, int dtype, double fill, int64_t *off, int cus, hipStream_t st)
{
    const Fill f = fill_patterns(dtype, fill);
    const int64_t es = dtype == SID_WARP_U8 ? 1 : 4;
    const int64_t cells = (int64_t)cell_count(g.rows, g.cols);
    if (im.rows_o == 0 || im.cols_o == 0) return SID_PM_OK;
    if (int rc = launch_fill(im.out, im.out_stride * es, im.cols_o * es, im.rows_o, f.out, cus, st)) return rc;
    if (int rc = launch_fill(im.covered, im.cols_o, im.cols_o, im.rows_o, 0u, cus, st)) return rc;
    if (int rc = launch_fill(im.map_x, im.cols_o * 4, im.cols_o * 4, im.rows_o, f.nan, cus, st)) return rc;
    if (int rc = launch_fill(im.map_y, im.cols_o * 4, im.cols_o * 4, im.rows_o, f.nan, cus, st)) return rc;
    if (cells == 0) return SID_PM_OK;
    hipLaunchKernelGGL(k_warp_count, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, g, im.rows_o, im.cols_o, cells, off);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_warp_scan, dim3(1), dim3(kScanBlock), 0, st, off, cells);
    HIP_TRY(hipGetLastError());
    if (dtype == SID_WARP_U8) hipLaunchKernelGGL(k_warp_walk<uint8_t>, dim3((unsigned)cus * 8), dim3(kBlock), 0, st, g, im, off, cells);
    else hipLaunchKernelGGL(k_warp_walk<float>, dim3((unsigned)cus * 8), dim3(kBlock), 0, st, g, im, off, cells);
    HIP_TRY(hipGetLastError());
    return SID_PM_OK;
}

void host_all(const Nodes &g, const Images &im, int dtype, double fill)
{
    const Fill f = fill_patterns(dtype, fill);
    const int64_t es = dtype == SID_WARP_U8 ? 1 : 4;
    if (im.out) host_fill(static_cast<unsigned char *>(im.out), im.out_stride * es, im.cols_o * es, im.rows_o, f.out);
    if (im.covered) host_fill(im.covered, im.cols_o, im.cols_o, im.rows_o, 0u);
    if (im.map_x) host_fill(reinterpret_cast<unsigned char *>(im.map_x), im.cols_o * 4, im.cols_o * 4, im.rows_o, f.nan);
    if (im.map_y) host_fill(reinterpret_cast<unsigned char *>(im.map_y), im.cols_o * 4, im.cols_o * 4, im.rows_o, f.nan);
    if (g.rows < 2 || g.cols < 2 || im.rows_o == 0 || im.cols_o == 0) return;
    if (dtype == SID_WARP_U8) host_walk<uint8_t>(g, im);
    else host_walk<float>(g, im);
}

// Per device, beside the pool's staging block of the host-buffer entry point: the offsets of the device entry point (grow-only
// too) and the number of compute units.  Calls are serialised by the pool's mutex.
struct Offsets {
    unsigned char *off = nullptr; size_t off_cap = 0; int cus = 0;
    bool cached() const { return off != nullptr; }
    void free() { if (off) (void)hipFree(off); }
};
using Dev = DevicePool<Offsets>::Slot;
DevicePool<Offsets> g_pool;

int compute_units(Dev &d, int device)
{
    if (d.cus > 0) return SID_PM_OK;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0)
        return fail(SID_PM_ERR_HIP, "hipDeviceGetAttribute(multiprocessor count) failed");
    d.cus = n;
    return SID_PM_OK;
}

}  // namespace

SID_EXPORT const char *sid_warp_last_error(void) { return g_err; }

SID_EXPORT int sid_warp_release(int device) { return g_pool.release(device); }

SID_EXPORT int sid_warp_image_device(const double *x, const double *y, const double *xs, const double *ys, const uint8_t *valid,
                                     int64_t grid_rows, int64_t grid_cols,
                                     const void *src, int dtype, int64_t rows_s, int64_t cols_s, int64_t src_stride,
                                     int64_t rows_o, int64_t cols_o, int order, double fill, int diagonal, uint32_t flags,
                                     void *out, int64_t out_stride, uint8_t *covered, float *map_x, float *map_y, void *hip_stream)
{
    if (int rc = check_args(x, y, xs, ys, grid_rows, grid_cols, src, dtype, rows_s, cols_s, src_stride, rows_o, cols_o, order, fill,
                            diagonal, flags, out, out_stride, covered, map_x, map_y))
        return rc;
    if (rows_o == 0 || cols_o == 0) return SID_PM_OK;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= kMaxDevices) return fail(SID_PM_ERR_NODEVICE, "no current HIP device");
    const Nodes g = {x, y, xs, ys, valid, grid_rows, grid_cols, diagonal};
    const Images im = {src, rows_s, cols_s, src_stride, rows_o, cols_o, order, flags, out, out_stride, covered, map_x, map_y};
    std::lock_guard<std::mutex> lock(g_pool.mutex(device));
    Dev &d = g_pool.slot[device];
    if (int rc = compute_units(d, device)) return rc;
    if (int rc = grow(d.off, d.off_cap, sizeof(int64_t) * (cell_count(grid_rows, grid_cols) + 1))) return rc;
    return launch_all(g, im, dtype, fill, reinterpret_cast<int64_t *>(d.off), d.cus, reinterpret_cast<hipStream_t>(hip_stream));
}

SID_EXPORT int sid_warp_image(int device, const double *x, const double *y, const double *xs, const double *ys, const uint8_t *valid,
                              int64_t grid_rows, int64_t grid_cols,
                              const void *src, int dtype, int64_t rows_s, int64_t cols_s, int64_t src_stride,
                              int64_t rows_o, int64_t cols_o, int order, double fill, int diagonal, uint32_t flags,
                              void *out, int64_t out_stride, uint8_t *covered, float *map_x, float *map_y)
{
    if (int rc = check_args(x, y, xs, ys, grid_rows, grid_cols, src, dtype, rows_s, cols_s, src_stride, rows_o, cols_o, order, fill,
                            diagonal, flags, out, out_stride, covered, map_x, map_y))
        return rc;
    if (rows_o == 0 || cols_o == 0) return SID_PM_OK;
    if (device == -1) {
        const Nodes g = {x, y, xs, ys, valid, grid_rows, grid_cols, diagonal};
        const Images im = {src, rows_s, cols_s, src_stride, rows_o, cols_o, order, flags, out, out_stride, covered, map_x, map_y};
        host_all(g, im, dtype, fill);
        return SID_PM_OK;
    }
    Staging s;
    if (!s.enter(g_pool, device)) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    Dev &d = g_pool.slot[device];
    const size_t es = dtype == SID_WARP_U8 ? 1 : 4;
    const size_t n = (size_t)(grid_rows * grid_cols), nb = sizeof(double) * n;
    const size_t npx = (size_t)rows_o * (size_t)cols_o, nsrc = src ? (size_t)rows_s * (size_t)cols_s : 0;
    int64_t *d_off;
    double *d_nodes[4];
    uint8_t *d_valid, *d_cov;
    unsigned char *d_src, *d_out;
    float *d_mx, *d_my;
    if (int rc = compute_units(d, device)) return rc;
    if (int rc = g_pool.carve(device, [&](Carver &c) {
            d_off = c.take<int64_t>(cell_count(grid_rows, grid_cols) + 1);
            for (double *&q : d_nodes) q = c.take<double>(n);
            d_valid = c.take<uint8_t>(n, valid != nullptr);
            d_src = c.take<unsigned char>(nsrc * es);
            d_out = c.take<unsigned char>(npx * es, out != nullptr);
            d_cov = c.take<uint8_t>(npx, covered != nullptr);
            d_mx = c.take<float>(npx, map_x != nullptr);
            d_my = c.take<float>(npx, map_y != nullptr);
        }))
        return rc;
    const double *nodes[4] = {x, y, xs, ys};
    for (int j = 0; j < 4 && n; ++j) HIP_TRY(hipMemcpyAsync(d_nodes[j], nodes[j], nb, hipMemcpyHostToDevice, 0));
    if (d_valid) HIP_TRY(hipMemcpyAsync(d_valid, valid, n, hipMemcpyHostToDevice, 0));
    if (d_src)
        HIP_TRY(hipMemcpy2DAsync(d_src, (size_t)cols_s * es, src, (size_t)src_stride * es, (size_t)cols_s * es, (size_t)rows_s,
                                 hipMemcpyHostToDevice, 0));
    const Nodes g = {d_nodes[0], d_nodes[1], d_nodes[2], d_nodes[3], d_valid, grid_rows, grid_cols, diagonal};
    const Images im = {d_src, rows_s, cols_s, cols_s, rows_o, cols_o, order, flags, d_out, cols_o, d_cov, d_mx, d_my};
    if (int rc = launch_all(g, im, dtype, fill, d_off, d.cus, 0)) return rc;
    if (out)
        HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_stride * es, d_out, (size_t)cols_o * es, (size_t)cols_o * es, (size_t)rows_o,
                                 hipMemcpyDeviceToHost, 0));
    if (covered) HIP_TRY(hipMemcpyAsync(covered, d_cov, npx, hipMemcpyDeviceToHost, 0));
    if (map_x) HIP_TRY(hipMemcpyAsync(map_x, d_mx, npx * 4, hipMemcpyDeviceToHost, 0));
    if (map_y) HIP_TRY(hipMemcpyAsync(map_y, d_my, npx * 4, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipStreamSynchronize(0));
    s.done();
    return SID_PM_OK;
}
