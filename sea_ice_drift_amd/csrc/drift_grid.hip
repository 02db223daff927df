// drift_grid.hip - drift grids on gfx950 (C ABI: include/sid_grid.h): the normalised median test and the
// deformation on the grid's own triangles.  The per-node and per-cell arithmetic is grid_cell.h / defor_elem.h, compiled here
// for the device and for the host instance (device = -1) alike.
//   k_grid_filter  one thread per node, 8 x 32 node tiles; the tile and its halo (u, v; NaN in both where a node is unusable or
//                  outside the grid) are staged in LDS once, and the four medians come by rank selection over the <= 24
//                  neighbours read from there: no per-thread array.
//   k_grid_defor   one thread per cell: the four ring nodes of x, y, u, v, the triangle rule, two slots written
//                  structure-of-arrays.
//   k_grid_fill    (section 23) one launch per pass of the gap filling, the filter's tiles; pass 1 from the inputs, later passes
//                  in place on the outputs, told apart by each node's generation.
//   k_grid_smooth  (section 23) normalised convolution on the same tiles, the weight table a kernel argument.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/sid_grid.h"
#include "grid_cell.h"
#include "host_util.h"

namespace {

constexpr int kTR = SID_GRID_TILE_ROWS, kTC = SID_GRID_TILE_COLS, kBlock = kTR * kTC;
static_assert(kBlock == 256, "the filter's tile is one 256-thread workgroup");

// ---------------------------------------------------------------- filter
// Neighbour (di, dj) of the node at (li, lj) of the staged tile
struct LdsGet {
    const double *su, *sv;
    int pitch, li, lj;
    __device__ __forceinline__ void operator()(int di, int dj, double &a, double &b) const
    {
        const int o = (li + di) * pitch + (lj + dj);
        a = su[o]; b = sv[o];
    }
};

// The same from the arrays themselves, for the host instance
struct HostGet {
    const double *u, *v;
    const uint8_t *valid;
    int64_t rows, cols, r, c;
    void operator()(int di, int dj, double &a, double &b) const
    {
        const int64_t rr = r + di, cc = c + dj;
        a = NAN; b = NAN;
        if (rr < 0 || rr >= rows || cc < 0 || cc >= cols) return;
        const int64_t k = rr * cols + cc;
        if (sid_grid::usable_uv(valid, k, u[k], v[k])) { a = u[k]; b = v[k]; }
    }
};

size_t filter_lds_bytes(int radius) { return sizeof(double) * 2 * (size_t)(kTR + 2 * radius) * (size_t)(kTC + 2 * radius); }

__global__ __launch_bounds__(kBlock) void k_grid_filter(const double *__restrict__ u, const double *__restrict__ v,
                                                        const uint8_t *__restrict__ valid, int64_t rows, int64_t cols,
                                                        int64_t tiles_c, double eps, double threshold, int radius,
                                                        int min_neighbours, uint8_t *__restrict__ keep, double *__restrict__ res)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int hh = kTR + 2 * radius, hw = kTC + 2 * radius;
    double *su = reinterpret_cast<double *>(smem), *sv = su + hh * hw;
    const int64_t tile = blockIdx.x, tr = tile / tiles_c, tc = tile - tr * tiles_c;
    const int64_t r0 = tr * kTR - radius, c0 = tc * kTC - radius;
    for (int e = threadIdx.x; e < hh * hw; e += kBlock) {
        const int li = e / hw, lj = e - li * hw;
        const int64_t r = r0 + li, c = c0 + lj;
        double a = NAN, b = NAN;
        if (r >= 0 && r < rows && c >= 0 && c < cols) {
            const int64_t k = r * cols + c;
            const double uu = u[k], vv = v[k];
            if (sid_grid::usable_uv(valid, k, uu, vv)) { a = uu; b = vv; }
        }
        su[e] = a; sv[e] = b;
    }
    __syncthreads();
    const int ti = threadIdx.x / kTC, tj = threadIdx.x - ti * kTC;
    const int64_t r = tr * kTR + ti, c = tc * kTC + tj;
    if (r >= rows || c >= cols) return;
    const LdsGet get = {su, sv, hw, ti + radius, tj + radius};
    const int o = (ti + radius) * hw + (tj + radius);
    uint8_t k8;
    double rs;
    sid_grid::filter_node(get, radius, su[o], sv[o], eps, threshold, min_neighbours, k8, rs);
    keep[r * cols + c] = k8;
    res[r * cols + c] = rs;
}

void host_filter(const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols, double eps, double threshold,
                 int radius, int min_neighbours, uint8_t *keep, double *res)
{
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) {
            const int64_t k = r * cols + c;
            const HostGet get = {u, v, valid, rows, cols, r, c};
            const bool ok = sid_grid::usable_uv(valid, k, u[k], v[k]);
            sid_grid::filter_node(get, radius, ok ? u[k] : NAN, ok ? v[k] : NAN, eps, threshold, min_neighbours, keep[k], res[k]);
        }
}

// ---------------------------------------------------------------- gap filling
// The neighbours of one pass from the arrays themselves, for the host instance: a generation in 0..pass-1 and finite values
struct HostFillGet {
    const double *uo, *vo;
    const int32_t *gen;
    int64_t rows, cols, r, c;
    int pass;
    void operator()(int di, int dj, double &a, double &b) const
    {
        const int64_t rr = r + di, cc = c + dj;
        a = NAN; b = NAN;
        if (rr < 0 || rr >= rows || cc < 0 || cc >= cols) return;
        const int64_t k = rr * cols + cc;
        if (gen[k] >= 0 && gen[k] < pass && isfinite(uo[k]) && isfinite(vo[k])) { a = uo[k]; b = vo[k]; }
    }
};

// One pass.  Pass 1 reads the inputs (its neighbours are generation 0: the usable nodes) and writes every output element.
// Passes 2 and up work in place on the outputs: a node is staged as a neighbour only with a generation in 0..pass-1, so one
// that another workgroup fills during this launch reads as "no generation" or as `pass` and is left out either way - no
// ordering between threads and no second buffer.  A workgroup without a candidate stages nothing.
__global__ __launch_bounds__(kBlock) void k_grid_fill(const double *__restrict__ u, const double *__restrict__ v,
                                                      const uint8_t *__restrict__ valid, const uint8_t *__restrict__ domain,
                                                      int64_t rows, int64_t cols, int64_t tiles_c, int radius, int min_neighbours,
                                                      int pass, double *uo, double *vo, int32_t *gen)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int hh = kTR + 2 * radius, hw = kTC + 2 * radius;
    double *su = reinterpret_cast<double *>(smem), *sv = su + hh * hw;
    const int64_t tile = blockIdx.x, tr = tile / tiles_c, tc = tile - tr * tiles_c;
    const int ti = threadIdx.x / kTC, tj = threadIdx.x - ti * kTC;
    const int64_t r = tr * kTR + ti, c = tc * kTC + tj, k = r * cols + c;
    const bool inside = r < rows && c < cols;
    double fu = NAN, fv = NAN;                                     // what pass 1 writes for a node that stays unfilled
    int32_t g = -1;
    bool candidate = false;
    if (inside) {
        const bool open = !domain || domain[k] != 0;
        if (pass == 1) {
            const double uu = u[k], vv = v[k];
            if (sid_grid::usable_uv(valid, k, uu, vv)) { fu = uu; fv = vv; g = 0; }
            candidate = g < 0 && open;
        } else {
            candidate = gen[k] < 0 && open;
        }
    }
    if (!__syncthreads_or(candidate)) {                            // (the same answer in every thread of the workgroup)
        if (pass == 1 && inside) { uo[k] = fu; vo[k] = fv; gen[k] = g; }
        return;
    }
    const int64_t r0 = tr * kTR - radius, c0 = tc * kTC - radius;
    for (int e = threadIdx.x; e < hh * hw; e += kBlock) {
        const int li = e / hw, lj = e - li * hw;
        const int64_t rr = r0 + li, cc = c0 + lj;
        double a = NAN, b = NAN;
        if (rr >= 0 && rr < rows && cc >= 0 && cc < cols) {
            const int64_t q = rr * cols + cc;
            if (pass == 1) {
                const double uu = u[q], vv = v[q];
                if (sid_grid::usable_uv(valid, q, uu, vv)) { a = uu; b = vv; }
            } else {
                const int32_t gq = gen[q];
                if (gq >= 0 && gq < pass) {
                    const double uu = uo[q], vv = vo[q];
                    if (isfinite(uu) && isfinite(vv)) { a = uu; b = vv; }
                }
            }
        }
        su[e] = a; sv[e] = b;
    }
    __syncthreads();
    if (!inside) return;
    if (candidate) {
        const LdsGet get = {su, sv, hw, ti + radius, tj + radius};
        if (sid_grid::fill_node(get, radius, min_neighbours, fu, fv)) g = pass;
    }
    if (pass == 1 || g == pass) { uo[k] = fu; vo[k] = fv; gen[k] = g; }
}

void host_fill(const double *u, const double *v, const uint8_t *valid, const uint8_t *domain, int64_t rows, int64_t cols,
               int radius, int min_neighbours, int max_passes, double *uo, double *vo, int32_t *gen)
{
    for (int64_t k = 0; k < rows * cols; ++k) {
        const bool ok = sid_grid::usable_uv(valid, k, u[k], v[k]);
        uo[k] = ok ? u[k] : NAN; vo[k] = ok ? v[k] : NAN; gen[k] = ok ? 0 : -1;
    }
    for (int pass = 1; pass <= max_passes; ++pass) {               // a node filled in this pass has gen = pass: not a neighbour
        bool filled = false;
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t c = 0; c < cols; ++c) {
                const int64_t k = r * cols + c;
                if (gen[k] >= 0 || (domain && domain[k] == 0)) continue;
                const HostFillGet get = {uo, vo, gen, rows, cols, r, c, pass};
                double fu, fv;
                if (sid_grid::fill_node(get, radius, min_neighbours, fu, fv)) { uo[k] = fu; vo[k] = fv; gen[k] = pass; filled = true; }
            }
        if (!filled) break;
    }
}

// ---------------------------------------------------------------- smoothing
// (LdsGet and HostGet at (0, 0) give the node itself: the centre takes part)
__global__ __launch_bounds__(kBlock) void k_grid_smooth(const double *__restrict__ u, const double *__restrict__ v,
                                                        const uint8_t *__restrict__ valid, int64_t rows, int64_t cols,
                                                        int64_t tiles_c, sid_grid::Weights wt, int radius,
                                                        double *__restrict__ uo, double *__restrict__ vo)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int hh = kTR + 2 * radius, hw = kTC + 2 * radius;
    double *su = reinterpret_cast<double *>(smem), *sv = su + hh * hw;
    const int64_t tile = blockIdx.x, tr = tile / tiles_c, tc = tile - tr * tiles_c;
    const int64_t r0 = tr * kTR - radius, c0 = tc * kTC - radius;
    for (int e = threadIdx.x; e < hh * hw; e += kBlock) {
        const int li = e / hw, lj = e - li * hw;
        const int64_t r = r0 + li, c = c0 + lj;
        double a = NAN, b = NAN;
        if (r >= 0 && r < rows && c >= 0 && c < cols) {
            const int64_t k = r * cols + c;
            const double uu = u[k], vv = v[k];
            if (sid_grid::usable_uv(valid, k, uu, vv)) { a = uu; b = vv; }
        }
        su[e] = a; sv[e] = b;
    }
    __syncthreads();
    const int ti = threadIdx.x / kTC, tj = threadIdx.x - ti * kTC;
    const int64_t r = tr * kTR + ti, c = tc * kTC + tj;
    if (r >= rows || c >= cols) return;
    const LdsGet get = {su, sv, hw, ti + radius, tj + radius};
    double us, vs;
    sid_grid::smooth_node(get, radius, wt, us, vs);
    uo[r * cols + c] = us;
    vo[r * cols + c] = vs;
}

void host_smooth(const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols, const sid_grid::Weights &wt,
                 int radius, double *uo, double *vo)
{
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) {
            const HostGet get = {u, v, valid, rows, cols, r, c};
            sid_grid::smooth_node(get, radius, wt, uo[r * cols + c], vo[r * cols + c]);
        }
}

// ---------------------------------------------------------------- deformation
// Cell k = i (cols - 1) + j of either instance: gather the ring, apply the rule, write both slots
__host__ __device__ inline void one_cell(const double *x, const double *y, const double *u, const double *v, const uint8_t *valid,
                                         int64_t cols, int diagonal, int64_t k,
                                         double *e1, double *e2, double *e3, double *ao, double *po, int32_t *t)
{
    const int64_t i = k / (cols - 1), j = k - i * (cols - 1), A = i * cols + j;
    const int32_t ids[4] = {(int32_t)A, (int32_t)(A + 1), (int32_t)(A + cols + 1), (int32_t)(A + cols)};
    double xs[4], ys[4], us[4], vs[4];
    unsigned usable = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t n = ids[q];
        xs[q] = x[n]; ys[q] = y[n]; us[q] = u[n]; vs[q] = v[n];
        if (sid_grid::usable_uv(valid, n, us[q], vs[q]) && isfinite(xs[q]) && isfinite(ys[q])) usable |= 1u << q;
    }
    double out[5][2];
    int32_t tt[2][3];
    sid_grid::cell(xs, ys, us, vs, usable, diagonal, ids, out, tt);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int64_t o = 2 * k + s;
        e1[o] = out[0][s]; e2[o] = out[1][s]; e3[o] = out[2][s]; ao[o] = out[3][s]; po[o] = out[4][s];
        t[3 * o] = tt[s][0]; t[3 * o + 1] = tt[s][1]; t[3 * o + 2] = tt[s][2];
    }
}

__global__ __launch_bounds__(kBlock) void k_grid_defor(const double *__restrict__ x, const double *__restrict__ y,
                                                       const double *__restrict__ u, const double *__restrict__ v,
                                                       const uint8_t *__restrict__ valid, int64_t cols, int diagonal, int64_t cells,
                                                       double *__restrict__ e1, double *__restrict__ e2, double *__restrict__ e3,
                                                       double *__restrict__ ao, double *__restrict__ po, int32_t *__restrict__ t)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < cells) one_cell(x, y, u, v, valid, cols, diagonal, k, e1, e2, e3, ao, po, t);
}

// ---------------------------------------------------------------- arguments
int check_size(int64_t rows, int64_t cols)
{
    if (rows < 0 || cols < 0) return fail(SID_PM_ERR_ARG, "bad sizes (rows = %lld, cols = %lld)", (long long)rows, (long long)cols);
    if (rows > 0 && cols > 0x7fffffffLL / rows)
        return fail(SID_PM_ERR_UNSUPPORTED, "rows * cols >= 2^31 (rows = %lld, cols = %lld)", (long long)rows, (long long)cols);
    return SID_PM_OK;
}

int check_filter_args(const void *u, const void *v, int64_t rows, int64_t cols, double eps, double threshold, int radius,
                      int min_neighbours, const void *keep, const void *res)
{
    if (!isfinite(eps) || eps <= 0.0) return fail(SID_PM_ERR_ARG, "eps must be finite and > 0 (got %g)", eps);
    if (!isfinite(threshold) || threshold <= 0.0) return fail(SID_PM_ERR_ARG, "threshold must be finite and > 0 (got %g)", threshold);
    if (radius < 1 || radius > 2) return fail(SID_PM_ERR_ARG, "radius must be 1 or 2 (got %d)", radius);
    if (min_neighbours < 1 || min_neighbours > (2 * radius + 1) * (2 * radius + 1) - 1)
        return fail(SID_PM_ERR_ARG, "min_neighbours must be in 1..%d (got %d)", (2 * radius + 1) * (2 * radius + 1) - 1, min_neighbours);
    if (int rc = check_size(rows, cols)) return rc;
    if (!u || !v || !keep || !res) return fail(SID_PM_ERR_ARG, "null pointer");
    return SID_PM_OK;
}

int check_defor_args(const void *x, const void *y, const void *u, const void *v, int64_t rows, int64_t cols, int diagonal,
                     const void *e1, const void *e2, const void *e3, const void *a, const void *p, const void *t)
{
    if (diagonal != SID_GRID_DIAG_SHORTER && diagonal != SID_GRID_DIAG_MAIN && diagonal != SID_GRID_DIAG_ANTI)
        return fail(SID_PM_ERR_ARG, "unknown diagonal code %d", diagonal);
    if (int rc = check_size(rows, cols)) return rc;
    if (!x || !y || !u || !v || !e1 || !e2 || !e3 || !a || !p || !t) return fail(SID_PM_ERR_ARG, "null pointer");
    return SID_PM_OK;
}

// [a, a + na) and [b, b + nb) bytes share a byte (never for an empty range)
bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return na && nb && pa < pb + nb && pb < pa + na;
}

// two float64 inputs and two float64 outputs of rows * cols elements each: no output on an input or on the other output
int check_no_alias(const double *u, const double *v, int64_t rows, int64_t cols, const double *uo, const double *vo)
{
    const size_t nb = sizeof(double) * (size_t)(rows * cols);
    if (overlap(uo, nb, u, nb) || overlap(uo, nb, v, nb) || overlap(vo, nb, u, nb) || overlap(vo, nb, v, nb) || overlap(uo, nb, vo, nb))
        return fail(SID_PM_ERR_ARG, "u_out and v_out may not overlap u, v or each other");
    return SID_PM_OK;
}

int check_fill_args(const double *u, const double *v, int64_t rows, int64_t cols, int radius, int min_neighbours, int max_passes,
                    const double *uo, const double *vo, const int32_t *gen)
{
    if (radius < 1 || radius > 2) return fail(SID_PM_ERR_ARG, "radius must be 1 or 2 (got %d)", radius);
    if (min_neighbours < 1 || min_neighbours > (2 * radius + 1) * (2 * radius + 1) - 1)
        return fail(SID_PM_ERR_ARG, "min_neighbours must be in 1..%d (got %d)", (2 * radius + 1) * (2 * radius + 1) - 1, min_neighbours);
    if (max_passes < 1 || max_passes > 256) return fail(SID_PM_ERR_ARG, "max_passes must be in 1..256 (got %d)", max_passes);
    if (int rc = check_size(rows, cols)) return rc;
    if (!u || !v || !uo || !vo || !gen) return fail(SID_PM_ERR_ARG, "null pointer");
    const size_t nb = sizeof(double) * (size_t)(rows * cols), ng = sizeof(int32_t) * (size_t)(rows * cols);
    if (overlap(gen, ng, u, nb) || overlap(gen, ng, v, nb) || overlap(gen, ng, uo, nb) || overlap(gen, ng, vo, nb))
        return fail(SID_PM_ERR_ARG, "gen may not overlap u, v, u_out or v_out");
    return check_no_alias(u, v, rows, cols, uo, vo);
}

// The checked copy of the caller's table
int check_smooth_args(const double *u, const double *v, int64_t rows, int64_t cols, const double *weights, int radius,
                      const double *uo, const double *vo, sid_grid::Weights &wt)
{
    if (radius < 1 || radius > 2) return fail(SID_PM_ERR_ARG, "radius must be 1 or 2 (got %d)", radius);
    if (!weights) return fail(SID_PM_ERR_ARG, "null pointer");
    const int side = 2 * radius + 1;
    wt = sid_grid::Weights();
    for (int i = 0; i < side * side; ++i) {
        if (!isfinite(weights[i]) || weights[i] < 0.0)
            return fail(SID_PM_ERR_ARG, "weights[%d][%d] must be finite and >= 0 (got %g)", i / side, i % side, weights[i]);
        wt.w[i] = weights[i];
    }
    if (!(weights[radius * side + radius] > 0.0)) return fail(SID_PM_ERR_ARG, "the centre weight must be > 0");
    if (int rc = check_size(rows, cols)) return rc;
    if (!u || !v || !uo || !vo) return fail(SID_PM_ERR_ARG, "null pointer");
    return check_no_alias(u, v, rows, cols, uo, vo);
}

// ---------------------------------------------------------------- launches
// One launch per pass, all of them: nothing returns to the host that could end the series early, and a pass without a
// candidate costs each workgroup one read of its nodes' generations.
int launch_fill(const double *u, const double *v, const uint8_t *valid, const uint8_t *domain, int64_t rows, int64_t cols,
                int radius, int min_neighbours, int max_passes, double *uo, double *vo, int32_t *gen, hipStream_t st)
{
    const int64_t tiles_r = (rows + kTR - 1) / kTR, tiles_c = (cols + kTC - 1) / kTC;
    for (int pass = 1; pass <= max_passes; ++pass) {
        hipLaunchKernelGGL(k_grid_fill, dim3((unsigned)(tiles_r * tiles_c)), dim3(kBlock), filter_lds_bytes(radius), st,
                           u, v, valid, domain, rows, cols, tiles_c, radius, min_neighbours, pass, uo, vo, gen);
        HIP_TRY(hipGetLastError());
    }
    return SID_PM_OK;
}

int launch_smooth(const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols, const sid_grid::Weights &wt,
                  int radius, double *uo, double *vo, hipStream_t st)
{
    const int64_t tiles_r = (rows + kTR - 1) / kTR, tiles_c = (cols + kTC - 1) / kTC;
    hipLaunchKernelGGL(k_grid_smooth, dim3((unsigned)(tiles_r * tiles_c)), dim3(kBlock), filter_lds_bytes(radius), st,
                       u, v, valid, rows, cols, tiles_c, wt, radius, uo, vo);
    HIP_TRY(hipGetLastError());
    return SID_PM_OK;
}

int launch_filter(const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols, double eps, double threshold,
                  int radius, int min_neighbours, uint8_t *keep, double *res, hipStream_t st)
{
    const int64_t tiles_r = (rows + kTR - 1) / kTR, tiles_c = (cols + kTC - 1) / kTC;     // rows * cols < 2^31: so is the product
    hipLaunchKernelGGL(k_grid_filter, dim3((unsigned)(tiles_r * tiles_c)), dim3(kBlock), filter_lds_bytes(radius), st,
                       u, v, valid, rows, cols, tiles_c, eps, threshold, radius, min_neighbours, keep, res);
    HIP_TRY(hipGetLastError());
    return SID_PM_OK;
}

int launch_defor(const double *x, const double *y, const double *u, const double *v, const uint8_t *valid, int64_t rows,
                 int64_t cols, int diagonal, double *e1, double *e2, double *e3, double *a, double *p, int32_t *t, hipStream_t st)
{
    const int64_t cells = (rows - 1) * (cols - 1);
    hipLaunchKernelGGL(k_grid_defor, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       x, y, u, v, valid, cols, diagonal, cells, e1, e2, e3, a, p, t);
    HIP_TRY(hipGetLastError());
    return SID_PM_OK;
}

// The staging block of the two host-buffer entry points, which carve it differently; calls are serialised by its mutex
DevicePool<> g_pool;

}  // namespace

SID_EXPORT const char *sid_grid_last_error(void) { return g_err; }

SID_EXPORT int sid_grid_release(int device) { return g_pool.release(device); }

SID_EXPORT int sid_grid_filter_device(const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols,
                                      double eps, double threshold, int radius, int min_neighbours, uint8_t *keep, double *res,
                                      void *hip_stream)
{
    if (int rc = check_filter_args(u, v, rows, cols, eps, threshold, radius, min_neighbours, keep, res)) return rc;
    if (rows * cols == 0) return SID_PM_OK;
    return launch_filter(u, v, valid, rows, cols, eps, threshold, radius, min_neighbours, keep, res,
                         reinterpret_cast<hipStream_t>(hip_stream));
}

SID_EXPORT int sid_grid_deformation_device(const double *x, const double *y, const double *u, const double *v, const uint8_t *valid,
                                           int64_t rows, int64_t cols, int diagonal,
                                           double *e1, double *e2, double *e3, double *a, double *p, int32_t *t, void *hip_stream)
{
    if (int rc = check_defor_args(x, y, u, v, rows, cols, diagonal, e1, e2, e3, a, p, t)) return rc;
    if (rows < 2 || cols < 2) return SID_PM_OK;
    return launch_defor(x, y, u, v, valid, rows, cols, diagonal, e1, e2, e3, a, p, t, reinterpret_cast<hipStream_t>(hip_stream));
}

SID_EXPORT int sid_grid_fill_device(const double *u, const double *v, const uint8_t *valid, const uint8_t *domain, int64_t rows,
                                    int64_t cols, int radius, int min_neighbours, int max_passes, double *u_out, double *v_out,
                                    int32_t *gen, void *hip_stream)
{
    if (int rc = check_fill_args(u, v, rows, cols, radius, min_neighbours, max_passes, u_out, v_out, gen)) return rc;
    if (rows * cols == 0) return SID_PM_OK;
    return launch_fill(u, v, valid, domain, rows, cols, radius, min_neighbours, max_passes, u_out, v_out, gen,
                       reinterpret_cast<hipStream_t>(hip_stream));
}

SID_EXPORT int sid_grid_smooth_device(const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols,
                                      const double *weights, int radius, double *u_out, double *v_out, void *hip_stream)
{
    sid_grid::Weights wt;
    if (int rc = check_smooth_args(u, v, rows, cols, weights, radius, u_out, v_out, wt)) return rc;
    if (rows * cols == 0) return SID_PM_OK;
    return launch_smooth(u, v, valid, rows, cols, wt, radius, u_out, v_out, reinterpret_cast<hipStream_t>(hip_stream));
}

SID_EXPORT int sid_grid_fill(int device, const double *u, const double *v, const uint8_t *valid, const uint8_t *domain,
                             int64_t rows, int64_t cols, int radius, int min_neighbours, int max_passes,
                             double *u_out, double *v_out, int32_t *gen)
{
    if (int rc = check_fill_args(u, v, rows, cols, radius, min_neighbours, max_passes, u_out, v_out, gen)) return rc;
    if (rows * cols == 0) return SID_PM_OK;
    if (device == -1) {
        host_fill(u, v, valid, domain, rows, cols, radius, min_neighbours, max_passes, u_out, v_out, gen);
        return SID_PM_OK;
    }
    Staging s;
    if (!s.enter(g_pool, device)) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    const size_t n = (size_t)(rows * cols), nb = sizeof(double) * n;
    double *du, *dv, *duo, *dvo;
    int32_t *dgen;
    uint8_t *dvalid, *ddomain;
    if (int rc = g_pool.carve(device, [&](Carver &c) {
            du = c.take<double>(n); dv = c.take<double>(n); duo = c.take<double>(n); dvo = c.take<double>(n);
            dgen = c.take<int32_t>(n);
            dvalid = c.take<uint8_t>(n, valid != nullptr); ddomain = c.take<uint8_t>(n, domain != nullptr);
        }))
        return rc;
    HIP_TRY(hipMemcpyAsync(du, u, nb, hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(dv, v, nb, hipMemcpyHostToDevice, 0));
    if (valid) HIP_TRY(hipMemcpyAsync(dvalid, valid, n, hipMemcpyHostToDevice, 0));
    if (domain) HIP_TRY(hipMemcpyAsync(ddomain, domain, n, hipMemcpyHostToDevice, 0));
    if (int rc = launch_fill(du, dv, dvalid, ddomain, rows, cols, radius, min_neighbours, max_passes, duo, dvo, dgen, 0)) return rc;
    HIP_TRY(hipMemcpyAsync(u_out, duo, nb, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipMemcpyAsync(v_out, dvo, nb, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipMemcpyAsync(gen, dgen, sizeof(int32_t) * n, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipStreamSynchronize(0));
    s.done();
    return SID_PM_OK;
}

SID_EXPORT int sid_grid_smooth(int device, const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols,
                               const double *weights, int radius, double *u_out, double *v_out)
{
    sid_grid::Weights wt;
    if (int rc = check_smooth_args(u, v, rows, cols, weights, radius, u_out, v_out, wt)) return rc;
    if (rows * cols == 0) return SID_PM_OK;
    if (device == -1) {
        host_smooth(u, v, valid, rows, cols, wt, radius, u_out, v_out);
        return SID_PM_OK;
    }
    Staging s;
    if (!s.enter(g_pool, device)) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    const size_t n = (size_t)(rows * cols), nb = sizeof(double) * n;
    double *du, *dv, *duo, *dvo;
    uint8_t *dvalid;
    if (int rc = g_pool.carve(device, [&](Carver &c) {
            du = c.take<double>(n); dv = c.take<double>(n); duo = c.take<double>(n); dvo = c.take<double>(n);
            dvalid = c.take<uint8_t>(n, valid != nullptr);
        }))
        return rc;
    HIP_TRY(hipMemcpyAsync(du, u, nb, hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(dv, v, nb, hipMemcpyHostToDevice, 0));
    if (valid) HIP_TRY(hipMemcpyAsync(dvalid, valid, n, hipMemcpyHostToDevice, 0));
    if (int rc = launch_smooth(du, dv, dvalid, rows, cols, wt, radius, duo, dvo, 0)) return rc;
    HIP_TRY(hipMemcpyAsync(u_out, duo, nb, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipMemcpyAsync(v_out, dvo, nb, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipStreamSynchronize(0));
    s.done();
    return SID_PM_OK;
}

SID_EXPORT int sid_grid_filter(int device, const double *u, const double *v, const uint8_t *valid, int64_t rows, int64_t cols,
                               double eps, double threshold, int radius, int min_neighbours, uint8_t *keep, double *res)
{
    if (int rc = check_filter_args(u, v, rows, cols, eps, threshold, radius, min_neighbours, keep, res)) return rc;
    if (rows * cols == 0) return SID_PM_OK;
    if (device == -1) {
        host_filter(u, v, valid, rows, cols, eps, threshold, radius, min_neighbours, keep, res);
        return SID_PM_OK;
    }
    Staging s;
    if (!s.enter(g_pool, device)) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    const size_t n = (size_t)(rows * cols), nb = sizeof(double) * n;
    double *du, *dv, *dres;
    uint8_t *dvalid, *dkeep;
    if (int rc = g_pool.carve(device, [&](Carver &c) {
            du = c.take<double>(n); dv = c.take<double>(n); dres = c.take<double>(n);
            dvalid = c.take<uint8_t>(n, valid != nullptr); dkeep = c.take<uint8_t>(n);
        }))
        return rc;
    HIP_TRY(hipMemcpyAsync(du, u, nb, hipMemcpyHostToDevice, 0));
    HIP_TRY(hipMemcpyAsync(dv, v, nb, hipMemcpyHostToDevice, 0));
    if (valid) HIP_TRY(hipMemcpyAsync(dvalid, valid, n, hipMemcpyHostToDevice, 0));
    if (int rc = launch_filter(du, dv, dvalid, rows, cols, eps, threshold, radius, min_neighbours, dkeep, dres, 0)) return rc;
    HIP_TRY(hipMemcpyAsync(keep, dkeep, n, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipMemcpyAsync(res, dres, nb, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipStreamSynchronize(0));
    s.done();
    return SID_PM_OK;
}

SID_EXPORT int sid_grid_deformation(int device, const double *x, const double *y, const double *u, const double *v,
                                    const uint8_t *valid, int64_t rows, int64_t cols, int diagonal,
                                    double *e1, double *e2, double *e3, double *a, double *p, int32_t *t)
{
    if (int rc = check_defor_args(x, y, u, v, rows, cols, diagonal, e1, e2, e3, a, p, t)) return rc;
    if (rows < 2 || cols < 2) return SID_PM_OK;
    if (device == -1) {
        for (int64_t k = 0; k < (rows - 1) * (cols - 1); ++k) one_cell(x, y, u, v, valid, cols, diagonal, k, e1, e2, e3, a, p, t);
        return SID_PM_OK;
    }
    Staging s;
    if (!s.enter(g_pool, device)) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    const size_t n = (size_t)(rows * cols), nb = sizeof(double) * n;
    const size_t m2 = 2 * (size_t)((rows - 1) * (cols - 1)), mb = sizeof(double) * m2, tb = sizeof(int32_t) * 3 * m2;
    double *in[4], *out[5];
    int32_t *dt;
    uint8_t *dvalid;
    if (int rc = g_pool.carve(device, [&](Carver &c) {
            for (double *&q : in) q = c.take<double>(n);
            for (double *&q : out) q = c.take<double>(m2);
            dt = c.take<int32_t>(3 * m2);
            dvalid = c.take<uint8_t>(n, valid != nullptr);
        }))
        return rc;
    const double *src[4] = {x, y, u, v};
    for (int j = 0; j < 4; ++j) HIP_TRY(hipMemcpyAsync(in[j], src[j], nb, hipMemcpyHostToDevice, 0));
    if (valid) HIP_TRY(hipMemcpyAsync(dvalid, valid, n, hipMemcpyHostToDevice, 0));
    if (int rc = launch_defor(in[0], in[1], in[2], in[3], dvalid, rows, cols, diagonal, out[0], out[1], out[2], out[3], out[4], dt, 0)) return rc;
    double *dst[5] = {e1, e2, e3, a, p};
    for (int j = 0; j < 5; ++j) HIP_TRY(hipMemcpyAsync(dst[j], out[j], mb, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipMemcpyAsync(t, dt, tb, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipStreamSynchronize(0));
    s.done();
    return SID_PM_OK;
}
