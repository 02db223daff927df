// track.hip - arbitrary points mapped through a drift grid on gfx950 (C ABI: include/sid_track.h).
// The per-cell and per-point steps are track_point.h, compiled here for the device and for the host instance (device = -1)
// alike.  One call queues, on one stream:
//   k_track_boxes   every cell's box into the scratch, every bucket's rectangle emptied (there are as many buckets as cells),
//                   and per workgroup the bounding box of its cells' boxes
//   k_track_axes    one workgroup: those partial boxes to the two axes of the bucket grid, kept in the scratch
//   k_track_build   one thread per cell: the cell enters the rectangle of every bucket its box touches (integer atomic min / max)
//   k_track_points  one thread per point: its bucket's rectangle in ascending cell number, the boxes first, until a triangle
//                   owns the point
// Grids below SID_TRACK_BRUTE_CELLS cells, and every grid under SID_TRACK_NO_GRID, skip the two middle kernels: every point
// looks at every cell's box.  The host never sees a node coordinate, and the search cannot reach the result: the owner is the
// lowest-numbered owning triangle of the specification's examined cells, and each route visits all of those in ascending order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>

#include "../../include/sid_grid.h"
#include "../../include/sid_track.h"
#include "host_util.h"
#include "track_point.h"

namespace {

using sid_track::Axis;
using sid_track::Box;
using sid_track::Rect;
using sid_warp::Nodes;

static_assert(sid_track::kClosed == SID_TRACK_CLOSED && sid_track::kBruteCells == SID_TRACK_BRUTE_CELLS, "codes of sid_track.h");
static_assert(sid_grid::kShorter == SID_GRID_DIAG_SHORTER && sid_grid::kMain == SID_GRID_DIAG_MAIN && sid_grid::kAnti == SID_GRID_DIAG_ANTI,
              "diagonal codes of sid_grid.h");

constexpr int kBlock = 256, kMaxPartials = 1024;

// The scratch of one call, a function of the number of cells alone (one layout for the device block and the host instance)
struct Scratch {
    Axis *axes;                                        // x, y
    Box *partial;                                      // kMaxPartials
    Box *boxes;                                        // per cell
    Rect *rects;                                       // per bucket = per cell
    void layout(Carver &c, size_t cells)
    {
        axes = c.take<Axis>(2, cells > 0);
        partial = c.take<Box>(kMaxPartials, cells > 0);
        boxes = c.take<Box>(cells);
        rects = c.take<Rect>(cells);
    }
};

// ---------------------------------------------------------------- kernels
// The bounding box of the workgroup's `acc`s, in thread 0
__device__ __forceinline__ Box block_merge(Box acc)
{
    __shared__ Box s[kBlock];
    const int t = threadIdx.x;
    s[t] = acc;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if (t < d) { Box a = s[t]; sid_track::merge(a, s[t + d]); s[t] = a; }
        __syncthreads();
    }
    return s[0];
}

__global__ __launch_bounds__(kBlock) void k_track_boxes(Nodes g, int64_t cells, Box *__restrict__ boxes, Rect *__restrict__ rects,
                                                        Box *__restrict__ partial)
{
    Box acc = sid_track::no_box();
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < cells; k += (int64_t)gridDim.x * kBlock) {
        const Box b = sid_track::cell_box(g, k);
        boxes[k] = b;
        rects[k] = sid_track::no_rect();
        sid_track::merge(acc, b);
    }
    acc = block_merge(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kBlock) void k_track_axes(const Box *__restrict__ partial, int n_partial, int32_t nbx, int32_t nby,
                                                       Axis *__restrict__ axes)
{
    Box acc = sid_track::no_box();
    for (int q = threadIdx.x; q < n_partial; q += kBlock) sid_track::merge(acc, partial[q]);
    acc = block_merge(acc);
    if (threadIdx.x == 0) {
        axes[0] = sid_track::make_axis(acc.xl, acc.xh, nbx);
        axes[1] = sid_track::make_axis(acc.yl, acc.yh, nby);
    }
}

struct AtomicLower { __device__ void operator()(int32_t *p, int32_t v) const { atomicMin(p, v); } };
struct AtomicRaise { __device__ void operator()(int32_t *p, int32_t v) const { atomicMax(p, v); } };
struct HostLower { void operator()(int32_t *p, int32_t v) const { if (v < *p) *p = v; } };
struct HostRaise { void operator()(int32_t *p, int32_t v) const { if (v > *p) *p = v; } };

__global__ __launch_bounds__(kBlock) void k_track_build(const Box *__restrict__ boxes, int64_t cells, int64_t across,
                                                        const Axis *__restrict__ axes, Rect *__restrict__ rects)
{
    const Axis ax = axes[0], ay = axes[1];
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < cells; k += (int64_t)gridDim.x * kBlock)
        sid_track::enter(boxes[k], k, across, ax, ay, rects, AtomicLower(), AtomicRaise());
}

__global__ __launch_bounds__(kBlock) void k_track_points(Nodes g, const Box *__restrict__ boxes, const Axis *__restrict__ axes,
                                                         const Rect *__restrict__ rects, unsigned flags,
                                                         const double *__restrict__ px, const double *__restrict__ py, int64_t n,
                                                         double *__restrict__ sx, double *__restrict__ sy, int32_t *__restrict__ tri)
{
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (int64_t)gridDim.x * kBlock) {
        double ox, oy;
        int32_t ot;
        sid_track::point(g, boxes, axes, rects, flags, px[q], py[q], ox, oy, ot);
        sx[q] = ox;
        sy[q] = oy;
        if (tri) tri[q] = ot;
    }
}

// ---------------------------------------------------------------- arguments
size_t cell_count(int64_t grid_rows, int64_t grid_cols)
{
    return grid_rows >= 2 && grid_cols >= 2 ? (size_t)((grid_rows - 1) * (grid_cols - 1)) : 0;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

int check_args(const double *x, const double *y, const double *xs, const double *ys, const uint8_t *valid, int64_t grid_rows,
               int64_t grid_cols, int diagonal, uint32_t flags, const double *px, const double *py, int64_t n, const double *sx,
               const double *sy, const int32_t *tri)
{
    if (diagonal != SID_GRID_DIAG_SHORTER && diagonal != SID_GRID_DIAG_MAIN && diagonal != SID_GRID_DIAG_ANTI)
        return fail(SID_PM_ERR_ARG, "unknown diagonal code %d", diagonal);
    if (flags & ~SID_TRACK_CLOSED) return fail(SID_PM_ERR_ARG, "unknown flags 0x%x", flags);
    if (grid_rows < 0 || grid_cols < 0 || n < 0)
        return fail(SID_PM_ERR_ARG, "negative size (grid %lld x %lld, %lld points)", (long long)grid_rows, (long long)grid_cols, (long long)n);
    if (grid_rows > 0 && grid_cols > 0x7fffffffLL / grid_rows)
        return fail(SID_PM_ERR_UNSUPPORTED, "grid_rows * grid_cols >= 2^31 (%lld x %lld)", (long long)grid_rows, (long long)grid_cols);
    if (tri && cell_count(grid_rows, grid_cols) >= ((size_t)1 << 30))
        return fail(SID_PM_ERR_UNSUPPORTED, "tri wanted with 2^30 cells or more (%lld x %lld nodes)", (long long)grid_rows, (long long)grid_cols);
    if (!x || !y || !xs || !ys) return fail(SID_PM_ERR_ARG, "null node grid");
    if (n == 0) return SID_PM_OK;
    if (!px || !py) return fail(SID_PM_ERR_ARG, "null point array");
    if (!sx || !sy) return fail(SID_PM_ERR_ARG, "null output");
    const size_t nodes = (size_t)(grid_rows * grid_cols), pts = (size_t)n * sizeof(double);
    const void *in[7] = {x, y, xs, ys, valid, px, py};
    const size_t in_bytes[7] = {nodes * 8, nodes * 8, nodes * 8, nodes * 8, nodes, pts, pts};
    const void *out[3] = {sx, sy, tri};
    const size_t out_bytes[3] = {pts, pts, (size_t)n * sizeof(int32_t)};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 7; ++i)
            if (overlap(out[o], out_bytes[o], in[i], in_bytes[i])) return fail(SID_PM_ERR_ARG, "an output overlaps an input");
        for (int p = 0; p < o; ++p)
            if (overlap(out[o], out_bytes[o], out[p], out_bytes[p])) return fail(SID_PM_ERR_ARG, "two outputs overlap");
    }
    return SID_PM_OK;
}

// every cell for every point?
bool brute(size_t cells) { return cells < SID_TRACK_BRUTE_CELLS || getenv("SID_TRACK_NO_GRID") != nullptr; }

// ---------------------------------------------------------------- launches
unsigned blocks_for(int64_t threads, int64_t cap)
{
    const int64_t b = (threads + kBlock - 1) / kBlock;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

// All of one call (n > 0); `sc` is carved for the grid's cells
int launch_all(const Nodes &g, const Scratch &sc, uint32_t flags, const double *px, const double *py, int64_t n, double *sx, double *sy,
               int32_t *tri, int cus, hipStream_t st)
{
    const int64_t cells = (int64_t)cell_count(g.rows, g.cols);
    const bool every = brute((size_t)cells);
    if (cells > 0) {
        const unsigned parts = blocks_for(cells, kMaxPartials);
        hipLaunchKernelGGL(k_track_boxes, dim3(parts), dim3(kBlock), 0, st, g, cells, sc.boxes, sc.rects, sc.partial);
        HIP_TRY(hipGetLastError());
        if (!every) {
            hipLaunchKernelGGL(k_track_axes, dim3(1), dim3(kBlock), 0, st, sc.partial, (int)parts, (int32_t)(g.cols - 1), (int32_t)(g.rows - 1), sc.axes);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_track_build, dim3(blocks_for(cells, (int64_t)cus * 32)), dim3(kBlock), 0, st, sc.boxes, cells, g.cols - 1,
                               sc.axes, sc.rects);
            HIP_TRY(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_track_points, dim3(blocks_for(n, (int64_t)cus * 32)), dim3(kBlock), 0, st, g, sc.boxes, every ? nullptr : sc.axes,
                       sc.rects, flags, px, py, n, sx, sy, tri);
    HIP_TRY(hipGetLastError());
    return SID_PM_OK;
}

// The same steps in host loops
void host_all(const Nodes &g, uint32_t flags, const double *px, const double *py, int64_t n, double *sx, double *sy, int32_t *tri)
{
    const size_t cells = cell_count(g.rows, g.cols);
    const bool every = brute(cells);
    Carver measure;
    Scratch sc;
    sc.layout(measure, cells);
    std::vector<unsigned char> block(measure.off + 1);
    Carver c(block.data());
    sc.layout(c, cells);
    Box all = sid_track::no_box();
    for (size_t k = 0; k < cells; ++k) {
        sc.boxes[k] = sid_track::cell_box(g, (int64_t)k);
        sc.rects[k] = sid_track::no_rect();
        sid_track::merge(all, sc.boxes[k]);
    }
    if (cells > 0 && !every) {
        sc.axes[0] = sid_track::make_axis(all.xl, all.xh, (int32_t)(g.cols - 1));
        sc.axes[1] = sid_track::make_axis(all.yl, all.yh, (int32_t)(g.rows - 1));
        for (size_t k = 0; k < cells; ++k)
            sid_track::enter(sc.boxes[k], (int64_t)k, g.cols - 1, sc.axes[0], sc.axes[1], sc.rects, HostLower(), HostRaise());
    }
    for (int64_t q = 0; q < n; ++q) {
        int32_t t;
        sid_track::point(g, sc.boxes, every ? nullptr : sc.axes, sc.rects, flags, px[q], py[q], sx[q], sy[q], t);
        if (tri) tri[q] = t;
    }
}

// Per device, beside the pool's staging block of the host-buffer entry point: the scratch of the device entry point (grow-only
// too) and the number of compute units.  Calls are serialised by the pool's mutex.
struct Cached {
    unsigned char *scr = nullptr; size_t scr_cap = 0; int cus = 0;
    bool cached() const { return scr != nullptr; }
    void free() { if (scr) (void)hipFree(scr); }
};
using Dev = DevicePool<Cached>::Slot;
DevicePool<Cached> g_pool;

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

SID_EXPORT const char *sid_track_last_error(void) { return g_err; }

SID_EXPORT int sid_track_release(int device) { return g_pool.release(device); }

SID_EXPORT int sid_track_points_device(const double *x, const double *y, const double *xs, const double *ys, const uint8_t *valid,
                                       int64_t grid_rows, int64_t grid_cols, int diagonal, uint32_t flags,
                                       const double *px, const double *py, int64_t n, double *sx, double *sy, int32_t *tri,
                                       void *hip_stream)
{
    if (int rc = check_args(x, y, xs, ys, valid, grid_rows, grid_cols, diagonal, flags, px, py, n, sx, sy, tri)) return rc;
    if (n == 0) return SID_PM_OK;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= kMaxDevices) return fail(SID_PM_ERR_NODEVICE, "no current HIP device");
    const Nodes g = {x, y, xs, ys, valid, grid_rows, grid_cols, diagonal};
    const size_t cells = cell_count(grid_rows, grid_cols);
    std::lock_guard<std::mutex> lock(g_pool.mutex(device));
    Dev &d = g_pool.slot[device];
    if (int rc = compute_units(d, device)) return rc;
    Carver measure;
    Scratch sc;
    sc.layout(measure, cells);
    if (int rc = grow(d.scr, d.scr_cap, measure.off)) return rc;
    Carver c(d.scr);
    sc.layout(c, cells);
    return launch_all(g, sc, flags, px, py, n, sx, sy, tri, d.cus, reinterpret_cast<hipStream_t>(hip_stream));
}

SID_EXPORT int sid_track_points(int device, const double *x, const double *y, const double *xs, const double *ys, const uint8_t *valid,
                                int64_t grid_rows, int64_t grid_cols, int diagonal, uint32_t flags,
                                const double *px, const double *py, int64_t n, double *sx, double *sy, int32_t *tri)
{
    if (int rc = check_args(x, y, xs, ys, valid, grid_rows, grid_cols, diagonal, flags, px, py, n, sx, sy, tri)) return rc;
    if (n == 0) return SID_PM_OK;
    if (device == -1) {
        const Nodes g = {x, y, xs, ys, valid, grid_rows, grid_cols, diagonal};
        host_all(g, flags, px, py, n, sx, sy, tri);
        return SID_PM_OK;
    }
    Staging s;
    if (!s.enter(g_pool, device)) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    Dev &d = g_pool.slot[device];
    const size_t nodes = (size_t)(grid_rows * grid_cols), nb = sizeof(double) * nodes, pts = (size_t)n;
    const size_t cells = cell_count(grid_rows, grid_cols);
    Scratch sc;
    double *d_nodes[4], *d_px, *d_py, *d_sx, *d_sy;
    uint8_t *d_valid;
    int32_t *d_tri;
    if (int rc = compute_units(d, device)) return rc;
    if (int rc = g_pool.carve(device, [&](Carver &c) {
            sc.layout(c, cells);
            for (double *&q : d_nodes) q = c.take<double>(nodes);
            d_valid = c.take<uint8_t>(nodes, valid != nullptr);
            d_px = c.take<double>(pts);
            d_py = c.take<double>(pts);
            d_sx = c.take<double>(pts);
            d_sy = c.take<double>(pts);
            d_tri = c.take<int32_t>(pts, tri != nullptr);
        }))
        return rc;
    const double *host_nodes[4] = {x, y, xs, ys};
    for (int j = 0; j < 4 && nodes; ++j) HIP_TRY(hipMemcpyAsync(d_nodes[j], host_nodes[j], nb, hipMemcpyHostToDevice, 0));
    if (d_valid) HIP_TRY(hipMemcpyAsync(d_valid, valid, nodes, hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(d_px, px, pts * sizeof(double), hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(d_py, py, pts * sizeof(double), hipMemcpyHostToDevice, 0));
    const Nodes g = {d_nodes[0], d_nodes[1], d_nodes[2], d_nodes[3], d_valid, grid_rows, grid_cols, diagonal};
    if (int rc = launch_all(g, sc, flags, d_px, d_py, n, d_sx, d_sy, d_tri, d.cus, 0)) return rc;
    HIP_TRY(hipMemcpyAsync(sx, d_sx, pts * sizeof(double), hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipMemcpyAsync(sy, d_sy, pts * sizeof(double), hipMemcpyDeviceToHost, 0));
    if (tri) HIP_TRY(hipMemcpyAsync(tri, d_tri, pts * sizeof(int32_t), hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipStreamSynchronize(0));
    s.done();
    return SID_PM_OK;
}
