// ft_guided.hip - guided Hamming k=2 matcher for 256-bit ORB descriptors on gfx950: the two nearest train descriptors among
// those within a radius of the query's predicted position.  C ABI: include/sid_ftg.h; DESIGN.md section 26.
//
// Everything runs on the caller's stream and nothing is read back, so the plan that depends on the data - the grid over the
// bounding box of the finite train positions - is made on the device, by the functions of ft_guided_plan.h:
//   ftg_box, ftg_plan   the box (partial boxes per workgroup, then one workgroup) and the Grid
//   ftg_bin             cell and rank within the cell of every train point and of every query (one atomic add each)
//   ftg_scan            exclusive prefix sums per cell: train points, queries, work items (one workgroup)
//   ftg_fill_train      descriptors, positions and original indices in cell order: a cell is one contiguous run
//   ftg_fill_query      the queries in cell order;  ftg_items: one (cell, run) per up to 256 queries of a cell
//   ftg_match           one workgroup per work item, one thread per query (8 dwords of descriptor and the position in VGPRs, a
//                       running top two by push, as ft_knn2_partial).  The workgroup walks the train runs of the 3 x 3 cells
//                       around its cell; the train index is uniform, so descriptor, position and index come through the
//                       scalar cache.  Each lane applies the float64 inclusion rule to its own query.
// The order within a cell varies from run to run (atomics); the result does not: the top two of the keys
// distance << 22 | original index and the count do not depend on the order they are met in.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "../../include/sid_ftg.h"
#include "ft_guided_plan.h"
#include "host_util.h"

namespace {

using sid_ftg::kThreads; using sid_ftg::kScanThreads; using sid_ftg::kNone; using sid_ftg::kBoxBlocks;
using sid_ftg::Grid; using sid_ftg::Regions; using sid_ftg::cell_of;

static_assert(sid_ftg::kMaxAxis == SID_FTG_MAX_AXIS && sid_ftg::kMargin == 1.0 + 1.0 / (double)(1 << SID_FTG_MARGIN_LOG2),
              "sid_ftg.h documents the plan header's constants");

__device__ __forceinline__ void push(uint32_t &k1, uint32_t &k2, uint32_t key)
{
    const uint32_t t = k1 > key ? k1 : key;                 // the larger of (best, new)
    k1 = k1 < key ? k1 : key;
    k2 = k2 < t ? k2 : t;
}

__device__ __forceinline__ bool finite2(double x, double y) { return isfinite(x) && isfinite(y); }

// The box of the workgroup's values, in thread 0 (b = x_lo, x_hi, y_lo, y_hi)
__device__ __forceinline__ void block_box(double (&b)[4])
{
    __shared__ double s[4][kThreads];
    const int t = threadIdx.x;
    for (int k = 0; k < 4; ++k) s[k][t] = b[k];
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if (t < d) {
            s[0][t] = fmin(s[0][t], s[0][t + d]); s[1][t] = fmax(s[1][t], s[1][t + d]);
            s[2][t] = fmin(s[2][t], s[2][t + d]); s[3][t] = fmax(s[3][t], s[3][t + d]);
        }
        __syncthreads();
    }
    for (int k = 0; k < 4; ++k) b[k] = s[k][0];
}

__global__ __launch_bounds__(kThreads) void ftg_box(const double *__restrict__ tx, const double *__restrict__ ty, int n2, double *__restrict__ part)
{
    double b[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int j = blockIdx.x * kThreads + threadIdx.x; j < n2; j += gridDim.x * kThreads) {
        const double x = tx[j], y = ty[j];
        if (finite2(x, y)) { b[0] = fmin(b[0], x); b[1] = fmax(b[1], x); b[2] = fmin(b[2], y); b[3] = fmax(b[3], y); }
    }
    block_box(b);
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) part[4 * blockIdx.x + k] = b[k];
}

__global__ __launch_bounds__(kThreads) void ftg_plan(const double *__restrict__ part, int nparts, double radius, int cap, Grid *__restrict__ grid)
{
    double b[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int p = threadIdx.x; p < nparts; p += kThreads) {
        b[0] = fmin(b[0], part[4 * p]); b[1] = fmax(b[1], part[4 * p + 1]);
        b[2] = fmin(b[2], part[4 * p + 2]); b[3] = fmax(b[3], part[4 * p + 3]);
    }
    block_box(b);
    if (threadIdx.x == 0) {
        Grid g;
        g.x = sid_ftg::make_axis(b[0], b[1], radius, cap);
        g.y = sid_ftg::make_axis(b[2], b[3], radius, cap);
        *grid = g;
    }
}

// cell[i] and rank[i] = how many points of the cell came before (any order).  A train point that is not finite gets cell -1
// and is in no cell; a query that is not finite is binned like any other (cell_of is total) and finds no candidate.
template <bool TRAIN>
__global__ __launch_bounds__(kThreads) void ftg_bin(const double *__restrict__ px, const double *__restrict__ py, int n, const Grid *__restrict__ grid,
                                                     int32_t *__restrict__ count, int32_t *__restrict__ cell, int32_t *__restrict__ rank)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const Grid g = *grid;
    const double x = px[i], y = py[i];
    if (TRAIN && !finite2(x, y)) { cell[i] = -1; rank[i] = 0; return; }
    const int32_t c = cell_of(g.y, y) * g.x.n + cell_of(g.x, x);
    cell[i] = c;
    rank[i] = atomicAdd(&count[c], 1);
}

// Exclusive prefix sums over the cells (start[cells] = total): train points, queries, work items = ceil(queries / 256)
__global__ __launch_bounds__(kScanThreads) void ftg_scan(const Grid *__restrict__ grid, const int32_t *__restrict__ tcount, const int32_t *__restrict__ qcount,
                                                         int32_t *__restrict__ tstart, int32_t *__restrict__ qstart, int32_t *__restrict__ istart)
{
    __shared__ int32_t part[3][kScanThreads];
    const int cells = grid->x.n * grid->y.n, t = threadIdx.x;
    const int per = (cells + kScanThreads - 1) / kScanThreads;
    const int c0 = min(t * per, cells), c1 = min(c0 + per, cells);
    int32_t st = 0, sq = 0, si = 0;
    for (int c = c0; c < c1; ++c) { st += tcount[c]; const int32_t q = qcount[c]; sq += q; si += (q + kThreads - 1) / kThreads; }
    part[0][t] = st; part[1][t] = sq; part[2][t] = si;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        int32_t v[3] = {0, 0, 0};
        if (t >= d) for (int k = 0; k < 3; ++k) v[k] = part[k][t - d];
        __syncthreads();
        for (int k = 0; k < 3; ++k) part[k][t] += v[k];
        __syncthreads();
    }
    int32_t bt = part[0][t] - st, bq = part[1][t] - sq, bi = part[2][t] - si;
    for (int c = c0; c < c1; ++c) {
        tstart[c] = bt; qstart[c] = bq; istart[c] = bi;
        bt += tcount[c]; const int32_t q = qcount[c]; bq += q; bi += (q + kThreads - 1) / kThreads;
    }
    if (t == kScanThreads - 1) { tstart[cells] = part[0][t]; qstart[cells] = part[1][t]; istart[cells] = part[2][t]; }
}

__global__ __launch_bounds__(kThreads) void ftg_fill_train(const uint4 *__restrict__ d2, const double *__restrict__ tx, const double *__restrict__ ty, int n2,
                                                           const int32_t *__restrict__ tcell, const int32_t *__restrict__ trank, const int32_t *__restrict__ tstart,
                                                           uint4 *__restrict__ sdesc, double *__restrict__ stx, double *__restrict__ sty, int32_t *__restrict__ sidx)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= n2) return;
    const int32_t c = tcell[j];
    if (c < 0) return;
    const int32_t at = tstart[c] + trank[j];                 // < tstart[c + 1] <= n2
    sdesc[2 * at] = d2[2 * j]; sdesc[2 * at + 1] = d2[2 * j + 1];
    stx[at] = tx[j]; sty[at] = ty[j]; sidx[at] = j;
}

__global__ __launch_bounds__(kThreads) void ftg_fill_query(int n1, const int32_t *__restrict__ qcell, const int32_t *__restrict__ qrank,
                                                           const int32_t *__restrict__ qstart, int32_t *__restrict__ qorder)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n1) qorder[qstart[qcell[i]] + qrank[i]] = i;    // (a permutation of 0 .. n1 - 1)
}

__global__ __launch_bounds__(kThreads) void ftg_items(const Grid *__restrict__ grid, const int32_t *__restrict__ qcount, const int32_t *__restrict__ istart,
                                                      int2 *__restrict__ items, int max_items)
{
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= grid->x.n * grid->y.n) return;
    const int runs = (qcount[c] + kThreads - 1) / kThreads;
    for (int k = 0; k < runs; ++k) {
        const int at = istart[c] + k;
        if (at < max_items) items[at] = make_int2(c, k);     // (always: sid_ftg::max_items is the bound of the sum)
    }
}

__global__ __launch_bounds__(kThreads) void ftg_match(const uint4 *__restrict__ d1, const double *__restrict__ qx, const double *__restrict__ qy,
                                                      const Grid *__restrict__ grid, const int32_t *__restrict__ tstart, const int32_t *__restrict__ qstart,
                                                      const int32_t *__restrict__ istart, const int2 *__restrict__ items, const int32_t *__restrict__ qorder,
                                                      const uint4 *__restrict__ sdesc, const double *__restrict__ stx, const double *__restrict__ sty,
                                                      const int32_t *__restrict__ sidx, double r2,
                                                      int32_t *__restrict__ idx, int32_t *__restrict__ dist, int32_t *__restrict__ count)
{
    const int nx = grid->x.n, ny = grid->y.n;
    if ((int)blockIdx.x >= istart[nx * ny]) return;          // the launch is sized by the bound of the work list
    const int2 item = items[blockIdx.x];
    const int cy = item.x / nx, cx = item.x - cy * nx;
    const int s0 = qstart[item.x] + item.y * kThreads, s1 = qstart[item.x + 1];      // s0 < s1: the item exists
    if (s0 + (int)(threadIdx.x & ~63u) >= s1) return;        // a wavefront without a query (no barrier below): most of them where
    const int slot = s0 + (int)threadIdx.x;                  // cells hold a few queries each
    const bool live = slot < s1;
    const int q = qorder[live ? slot : s0];
    const uint4 qa = d1[2 * q], qb = d1[2 * q + 1];
    const double x0 = qx[q], y = qy[q];
    const double x = finite2(x0, y) ? x0 : NAN;              // a query that is not finite: every comparison below is false
    uint32_t k1 = kNone, k2 = kNone;
    int32_t cnt = 0;
    const int ya = cy > 0 ? cy - 1 : 0, yb = cy + 1 < ny ? cy + 1 : ny - 1;
    const int xa = cx > 0 ? cx - 1 : 0, xb = cx + 1 < nx ? cx + 1 : nx - 1;
    for (int yy = ya; yy <= yb; ++yy) {
        const int j0 = tstart[yy * nx + xa], j1 = tstart[yy * nx + xb + 1];          // the cells of a row are consecutive runs
#pragma unroll 2
        for (int j = j0; j < j1; ++j) {                      // j is uniform: scalar loads of the train point
            const uint4 ta = sdesc[2 * j], tb = sdesc[2 * j + 1];
            const double dx = stx[j] - x, dy = sty[j] - y;
            const bool in = dx * dx + dy * dy <= r2;
            uint32_t d = __builtin_popcount(qa.x ^ ta.x);
            d += __builtin_popcount(qa.y ^ ta.y);
            d += __builtin_popcount(qa.z ^ ta.z);
            d += __builtin_popcount(qa.w ^ ta.w);
            d += __builtin_popcount(qb.x ^ tb.x);
            d += __builtin_popcount(qb.y ^ tb.y);
            d += __builtin_popcount(qb.z ^ tb.z);
            d += __builtin_popcount(qb.w ^ tb.w);
            push(k1, k2, (d << 22) | (uint32_t)sidx[j] | (in ? 0u : kNone));      // (no branch: the loads stay ahead of the loop)
            cnt += in ? 1 : 0;
        }
    }
    if (live) {
        idx[2 * q + 0] = k1 == kNone ? -1 : (int32_t)(k1 & 0x3fffffu);
        dist[2 * q + 0] = k1 == kNone ? -1 : (int32_t)(k1 >> 22);
        idx[2 * q + 1] = k2 == kNone ? -1 : (int32_t)(k2 & 0x3fffffu);
        dist[2 * q + 1] = k2 == kNone ? -1 : (int32_t)(k2 >> 22);
        if (count) count[q] = cnt;
    }
}

// an empty train set: nobody has a candidate
__global__ __launch_bounds__(kThreads) void ftg_none(int n1, int32_t *__restrict__ idx, int32_t *__restrict__ dist, int32_t *__restrict__ count)
{
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= n1) return;
    idx[2 * q] = idx[2 * q + 1] = dist[2 * q] = dist[2 * q + 1] = -1;
    if (count) count[q] = 0;
}

// what every entry point checks before any device call
int check_args(int64_t n1, int64_t n2, double radius)
{
    if (n1 < 0 || n2 < 0) return fail(SID_PM_ERR_ARG, "negative descriptor count");
    if (!sid_ftg::sizes_supported(n1, n2))
        return fail(SID_PM_ERR_ARG, "at most %lld queries and %lld train descriptors", (long long)sid_ftg::kMaxQueries, (long long)sid_ftg::kMaxTrain - 1);
    if (!sid_ftg::radius_ok(radius)) return fail(SID_PM_ERR_ARG, "radius must be finite and >= 0 (got %g)", radius);
    return SID_PM_OK;
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

SID_EXPORT const char *sid_ftg_last_error(void) { return g_err; }

SID_EXPORT int64_t sid_ftg_workspace_bytes(int64_t n1, int64_t n2) { return sid_ftg::workspace_bytes(n1, n2); }

// Test support: what ft_guided_plan.h computes.  Host arithmetic only.
SID_EXPORT int sid_ftg_debug_plan(int64_t n1, int64_t n2, double x_lo, double x_hi, double y_lo, double y_hi, double radius,
                                  struct sid_ftg_plan *out)
{
    if (!out) return fail(SID_PM_ERR_ARG, "null plan");
    if (int rc = check_args(n1, n2, radius)) return rc;
    const Regions R = sid_ftg::regions(n1, n2);
    const sid_ftg::Axis ax = sid_ftg::make_axis(x_lo, x_hi, radius, R.cap), ay = sid_ftg::make_axis(y_lo, y_hi, radius, R.cap);
    *out = sid_ftg_plan{ax.x0, ay.x0, ax.cell, ay.cell, ax.n, ay.n, R.cap, R.items, (int64_t)R.total};
    return SID_PM_OK;
}

SID_EXPORT int sid_ftg_knn2_device(const uint8_t *d_desc1, const double *d_qx, const double *d_qy, int64_t n1,
                                   const uint8_t *d_desc2, const double *d_tx, const double *d_ty, int64_t n2, double radius,
                                   int32_t *d_idx, int32_t *d_dist, int32_t *d_count, void *d_workspace, void *hip_stream)
{
    if (int rc = check_args(n1, n2, radius)) return rc;
    if (n1 == 0) return SID_PM_OK;
    if (!d_desc1 || !d_qx || !d_qy || !d_idx || !d_dist || (n2 > 0 && (!d_desc2 || !d_tx || !d_ty || !d_workspace)))
        return fail(SID_PM_ERR_ARG, "null pointer");
    if ((reinterpret_cast<uintptr_t>(d_desc1) | reinterpret_cast<uintptr_t>(d_desc2) | reinterpret_cast<uintptr_t>(d_workspace)) & 15)
        return fail(SID_PM_ERR_ARG, "descriptors and workspace must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (n2 == 0) {
        hipLaunchKernelGGL(ftg_none, dim3(blocks(n1)), dim3(kThreads), 0, st, (int)n1, d_idx, d_dist, d_count);
        return launched("guided matcher launch");
    }
    const Regions R = sid_ftg::regions(n1, n2);
    uint8_t *ws = reinterpret_cast<uint8_t *>(d_workspace);
    auto at = [&](sid_ftg::Region r) { return ws + R.off[r]; };
    auto i32 = [&](sid_ftg::Region r) { return reinterpret_cast<int32_t *>(at(r)); };
    auto f64 = [&](sid_ftg::Region r) { return reinterpret_cast<double *>(at(r)); };
    Grid *grid = reinterpret_cast<Grid *>(at(sid_ftg::kGridR));
    uint4 *sdesc = reinterpret_cast<uint4 *>(at(sid_ftg::kSDesc));
    int2 *items = reinterpret_cast<int2 *>(at(sid_ftg::kItems));
    const uint4 *d1 = reinterpret_cast<const uint4 *>(d_desc1), *d2 = reinterpret_cast<const uint4 *>(d_desc2);
    const int nparts = (int)std::min<int64_t>(kBoxBlocks, blocks(n2));
    // the two count regions lie one behind the other: one fill zeroes both
    HIP_TRY(hipMemsetAsync(at(sid_ftg::kTCount), 0, R.off[sid_ftg::kQCount] - R.off[sid_ftg::kTCount] + R.bytes[sid_ftg::kQCount], st));
    hipLaunchKernelGGL(ftg_box, dim3(nparts), dim3(kThreads), 0, st, d_tx, d_ty, (int)n2, f64(sid_ftg::kBox));
    hipLaunchKernelGGL(ftg_plan, dim3(1), dim3(kThreads), 0, st, f64(sid_ftg::kBox), nparts, radius, (int)R.cap, grid);
    hipLaunchKernelGGL(ftg_bin<true>, dim3(blocks(n2)), dim3(kThreads), 0, st, d_tx, d_ty, (int)n2, grid, i32(sid_ftg::kTCount),
                       i32(sid_ftg::kTCell), i32(sid_ftg::kTRank));
    hipLaunchKernelGGL(ftg_bin<false>, dim3(blocks(n1)), dim3(kThreads), 0, st, d_qx, d_qy, (int)n1, grid, i32(sid_ftg::kQCount),
                       i32(sid_ftg::kQCell), i32(sid_ftg::kQRank));
    hipLaunchKernelGGL(ftg_scan, dim3(1), dim3(kScanThreads), 0, st, grid, i32(sid_ftg::kTCount), i32(sid_ftg::kQCount),
                       i32(sid_ftg::kTStart), i32(sid_ftg::kQStart), i32(sid_ftg::kIStart));
    hipLaunchKernelGGL(ftg_fill_train, dim3(blocks(n2)), dim3(kThreads), 0, st, d2, d_tx, d_ty, (int)n2, i32(sid_ftg::kTCell),
                       i32(sid_ftg::kTRank), i32(sid_ftg::kTStart), sdesc, f64(sid_ftg::kSTx), f64(sid_ftg::kSTy), i32(sid_ftg::kSIdx));
    hipLaunchKernelGGL(ftg_fill_query, dim3(blocks(n1)), dim3(kThreads), 0, st, (int)n1, i32(sid_ftg::kQCell), i32(sid_ftg::kQRank),
                       i32(sid_ftg::kQStart), i32(sid_ftg::kQOrder));
    hipLaunchKernelGGL(ftg_items, dim3(blocks(R.cells_cap)), dim3(kThreads), 0, st, grid, i32(sid_ftg::kQCount), i32(sid_ftg::kIStart),
                       items, (int)R.items);
    hipLaunchKernelGGL(ftg_match, dim3((unsigned)R.items), dim3(kThreads), 0, st, d1, d_qx, d_qy, grid, i32(sid_ftg::kTStart),
                       i32(sid_ftg::kQStart), i32(sid_ftg::kIStart), items, i32(sid_ftg::kQOrder), sdesc, f64(sid_ftg::kSTx),
                       f64(sid_ftg::kSTy), i32(sid_ftg::kSIdx), radius * radius, d_idx, d_dist, d_count);
    return launched("guided matcher launch");
}

// Device scratch of sid_ftg_knn2: one grow-only block per device, kept between calls; one mutex per device, as the matcher's
static DevicePool<NoExtra, true> g_pool;

SID_EXPORT int sid_ftg_release(int device) { return g_pool.release(device); }

SID_EXPORT int sid_ftg_knn2(int device, const uint8_t *desc1, const double *qx, const double *qy, int64_t n1,
                            const uint8_t *desc2, const double *tx, const double *ty, int64_t n2, double radius,
                            int32_t *idx, int32_t *dist, int32_t *count)
{
    if (int rc = check_args(n1, n2, radius)) return rc;
    if (n1 == 0) return SID_PM_OK;
    if (!desc1 || !qx || !qy || !idx || !dist || (n2 > 0 && (!desc2 || !tx || !ty))) return fail(SID_PM_ERR_ARG, "null pointer");
    Staging s;
    if (!s.enter(g_pool, device))
        return s.dev.visible < 1 ? fail(SID_PM_ERR_NODEVICE, "no HIP device visible") : fail(SID_PM_ERR_ARG, "device %d out of range", device);
    const size_t q = (size_t)n1, t = (size_t)std::max<int64_t>(n2, 1);                  // (an empty train set: sized, never read)
    uint8_t *d1, *d2, *ws;
    double *dqx, *dqy, *dtx, *dty;
    int32_t *di, *dd, *dc;
    if (int rc = g_pool.carve(device, [&](Carver &c) {
            d1 = c.take<uint8_t>(q * SID_FTG_DESC_BYTES); dqx = c.take<double>(q); dqy = c.take<double>(q);
            d2 = c.take<uint8_t>(t * SID_FTG_DESC_BYTES); dtx = c.take<double>(t); dty = c.take<double>(t);
            ws = c.take<uint8_t>((size_t)sid_ftg_workspace_bytes(n1, n2));
            di = c.take<int32_t>(2 * q); dd = c.take<int32_t>(2 * q); dc = c.take<int32_t>(q, count != nullptr);
        }))
        return rc;
    HIP_TRY(hipMemcpyAsync(d1, desc1, q * SID_FTG_DESC_BYTES, hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(dqx, qx, q * sizeof(double), hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(dqy, qy, q * sizeof(double), hipMemcpyHostToDevice, nullptr));
    if (n2 > 0) {
        HIP_TRY(hipMemcpyAsync(d2, desc2, (size_t)n2 * SID_FTG_DESC_BYTES, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(dtx, tx, (size_t)n2 * sizeof(double), hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(dty, ty, (size_t)n2 * sizeof(double), hipMemcpyHostToDevice, nullptr));
    }
    if (int rc = sid_ftg_knn2_device(d1, dqx, dqy, n1, d2, dtx, dty, n2, radius, di, dd, dc, ws, nullptr)) return rc;
    HIP_TRY(hipMemcpyAsync(idx, di, sizeof(int32_t) * 2 * q, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpyAsync(dist, dd, sizeof(int32_t) * 2 * q, hipMemcpyDeviceToHost, nullptr));
    if (count) HIP_TRY(hipMemcpyAsync(count, dc, sizeof(int32_t) * q, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    s.done();
    return SID_PM_OK;
}
