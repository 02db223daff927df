// local_corr.hip - local zero-mean normalised correlation of two uint8 images on gfx950 (C ABI: include/sid_corr.h; DESIGN.md
// section 24).  The centre / clip / finalisation arithmetic is corr_window.h, compiled here for the device and for the host
// instance (device = -1) alike.
//   k_corr_lattice  nodes on a regular lattice, separable.  A workgroup owns a tile of 8 x 64 nodes and walks the rows of the
//                   tile's pixel footprint four at a time (one wavefront per row): the row's bytes of both images go to LDS
//                   once, each with the bytes zeroed where the other image is 0, so that plain sums are the masked sums; lane
//                   j forms the w-tap horizontal sums of node column j, four bytes per instruction (unsigned 8-bit dot
//                   product; a row sum is at most 255 * 65025 < 2^31); then every node adds the rows of its window, the
//                   squares and the product in 64 bits.  A pixel is read from memory once per tile and multiplied once per
//                   node COLUMN that shares it, not once per node.
//   k_corr_points   nodes anywhere, plain: one wavefront per node over its clipped window, a grid-stride loop over the nodes.
//   k_corr_lattice_plain  the same for a lattice whose steps are both at least the window: no pixel is shared, so there is
//                   nothing for the tiles to save, and a wavefront per node keeps the whole GPU busy on a few thousand nodes.
// Neither kernel needs scratch memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/sid_corr.h"
#include "corr_window.h"
#include "host_util.h"

namespace {

using sid_corr::Sums;

static_assert(sid_corr::kTileRows == SID_CORR_TILE_ROWS && sid_corr::kTileCols == SID_CORR_TILE_COLS, "tile constants of sid_corr.h");

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kTR = sid_corr::kTileRows, kTC = sid_corr::kTileCols;
constexpr int kPerThread = kTR / kWaves;                   // nodes of a thread: rows wave, wave + kWaves, ... of column lane
constexpr int kSegSmall = 512, kSegLarge = 4096;           // dwords of one staged row of one image
constexpr int64_t kPlainBlocks = 1 << 14;                  // most workgroups of a wavefront-per-node launch; the rest by its stride
static_assert(kTC == 64 && kTR % kWaves == 0, "lane = node column; node rows dealt out to the wavefronts");
static_assert((kTC - 1) * 255 + 255 <= 4 * kSegLarge, "the widest footprint row fits the large segment");
static_assert((2 * kWaves * kSegLarge + kWaves * 6 * kTC) * 4 <= 160 * 1024, "LDS of a CU");

struct Img {
    const uint8_t *a, *b;
    int64_t a_stride, b_stride, rows, cols;
};

struct Lattice {
    int64_t r0, c0, sr, sc, nr, nc;
    int w, rp, cp;                                         // rp = min(sr, w), cp = min(sc, w): see slot_* below
};

struct Out {
    double *corr;
    int32_t *count;
    int64_t *sums;
    int64_t min_count;
};

// A tile's footprint in SLOTS.  Along an axis with step s and p = min(s, w), node i of the tile covers the slots
// [i p, i p + w).  With s < w the slots are the contiguous pixels from the first node's window on (neighbours share them); with
// s >= w they are the tile's windows laid side by side (nothing is shared, and the pixels between windows are never read).
// Slot q is the pixel  centre(origin, first + q / p, s) - w / 2 + q % p  either way.
__host__ __device__ inline int64_t slot_pixel(int64_t origin, int64_t first, int64_t step, int p, int w, int q)
{
    return sid_corr::centre(origin, first + q / p, step) - w / 2 + q % p;
}

// 0x01 in every byte of v that is not 0
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t v)
{
    uint32_t t = v | (v >> 4);                              // (bit 0 of a byte collects bits of that byte only)
    t |= t >> 2;
    t |= t >> 1;
    return t & 0x01010101u;
}

__device__ __forceinline__ uint32_t load4(const uint8_t *p)              // four bytes at any alignment
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

template <int kSeg>
__global__ __launch_bounds__(kBlock) void k_corr_lattice(Img im, Lattice g, Out o, int64_t tiles_c)
{
    __shared__ uint32_t sA[kWaves][kSeg], sB[kWaves][kSeg];
    __shared__ uint32_t sH[kWaves][6][kTC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ti = (int64_t)blockIdx.x / tiles_c, tj = (int64_t)blockIdx.x - ti * tiles_c;
    const int64_t i0 = ti * kTR, j0 = tj * kTC;
    const int tra = (int)(g.nr - i0 < kTR ? g.nr - i0 : kTR), tca = (int)(g.nc - j0 < kTC ? g.nc - j0 : kTC);
    const int w = g.w, rp = g.rp, cp = g.cp;
    const int Lr = (tra - 1) * rp + w, Lc = (tca - 1) * cp + w, Ld = (Lc + 3) >> 2;       // slots of the tile; dwords of a row
    const bool contiguous = g.sc == (int64_t)cp;
    const int64_t cbase = sid_corr::centre(g.c0, j0, g.sc) - w / 2;

    uint32_t n[kPerThread], sa[kPerThread], sb[kPerThread];                 // Sa, Sb <= 65025 * 255 < 2^32
    uint64_t saa[kPerThread], sbb[kPerThread], sab[kPerThread];
#pragma unroll
    for (int m = 0; m < kPerThread; ++m) n[m] = sa[m] = sb[m] = 0, saa[m] = sbb[m] = sab[m] = 0;

    for (int q0 = 0; q0 < Lr; q0 += kWaves) {
        // ---- stage: wavefront k the row slot q0 + k, both images masked by each other; zeros outside the image
        {
            const int q = q0 + wave;
            const int64_t rr = slot_pixel(g.r0, i0, g.sr, rp, w, q);
            const bool row_ok = q < Lr && rr >= 0 && rr < im.rows;
            const uint8_t *pa = im.a + (row_ok ? rr : 0) * im.a_stride, *pb = im.b + (row_ok ? rr : 0) * im.b_stride;
            for (int d = lane; d < Ld; d += 64) {
                uint32_t A = 0, B = 0;
                if (row_ok) {
                    const int p = 4 * d;
                    int jj = contiguous ? 0 : p / cp, t = contiguous ? p : p - jj * cp;
                    const int64_t col = contiguous ? cbase + p : sid_corr::centre(g.c0, j0 + jj, g.sc) - w / 2 + t;
                    if ((contiguous || t + 3 < cp) && col >= 0 && col + 3 < im.cols) {
                        A = load4(pa + col);
                        B = load4(pb + col);
                    } else {
                        for (int e = 0; e < 4; ++e) {
                            if (!contiguous && t == cp) { t = 0; ++jj; }
                            const int64_t ce = contiguous ? cbase + p + e : sid_corr::centre(g.c0, j0 + jj, g.sc) - w / 2 + t;
                            if (ce >= 0 && ce < im.cols) {
                                A |= (uint32_t)pa[ce] << (8 * e);
                                B |= (uint32_t)pb[ce] << (8 * e);
                            }
                            ++t;
                        }
                    }
                    const uint32_t ma = nonzero_bytes(A) * 0xffu, mb = nonzero_bytes(B) * 0xffu;
                    A &= mb;
                    B &= ma;
                }
                sA[wave][d] = A;
                sB[wave][d] = B;
            }
        }
        __syncthreads();
        // ---- horizontal: lane j the w taps of node column j in this wavefront's row
        if (lane < tca) {
            const int s = lane * cp, e = s + w, d0 = s >> 2, d1 = (e + 3) >> 2;
            const uint32_t first = 0xffffffffu << (8 * (s & 3)), last = (e & 3) ? 0xffffffffu >> (8 * (4 - (e & 3))) : 0xffffffffu;
            uint32_t hn = 0, ha = 0, hb = 0, haa = 0, hbb = 0, hab = 0;
            for (int d = d0; d < d1; ++d) {
                uint32_t A = sA[wave][d], B = sB[wave][d];
                const uint32_t keep = (d == d0 ? first : 0xffffffffu) & (d == d1 - 1 ? last : 0xffffffffu);
                A &= keep;
                B &= keep;
                hn += (uint32_t)__popc(nonzero_bytes(A));
                ha = __builtin_amdgcn_udot4(A, 0x01010101u, ha, false);
                hb = __builtin_amdgcn_udot4(B, 0x01010101u, hb, false);
                haa = __builtin_amdgcn_udot4(A, A, haa, false);
                hbb = __builtin_amdgcn_udot4(B, B, hbb, false);
                hab = __builtin_amdgcn_udot4(A, B, hab, false);
            }
            sH[wave][0][lane] = hn; sH[wave][1][lane] = ha; sH[wave][2][lane] = hb;
            sH[wave][3][lane] = haa; sH[wave][4][lane] = hbb; sH[wave][5][lane] = hab;
        }
        __syncthreads();
        // ---- vertical: every node the staged rows that lie in its window
        if (lane < tca) {
#pragma unroll
            for (int m = 0; m < kPerThread; ++m) {
                const int lo = (wave + kWaves * m) * rp, hi = lo + w;       // (a node row beyond tra adds to sums nobody stores)
#pragma unroll
                for (int k = 0; k < kWaves; ++k) {
                    const int q = q0 + k;
                    if (q >= lo && q < hi && q < Lr) {
                        n[m] += sH[k][0][lane]; sa[m] += sH[k][1][lane]; sb[m] += sH[k][2][lane];
                        saa[m] += sH[k][3][lane]; sbb[m] += sH[k][4][lane]; sab[m] += sH[k][5][lane];
                    }
                }
            }
        }
        // (the next staging writes sA / sB only, and sH is written again after the next barrier)
    }
    if (lane < tca) {
#pragma unroll
        for (int m = 0; m < kPerThread; ++m) {
            const int i = wave + kWaves * m;
            if (i >= tra) continue;
            const Sums s = {(int64_t)n[m], (int64_t)sa[m], (int64_t)sb[m], (int64_t)saa[m], (int64_t)sbb[m], (int64_t)sab[m]};
            sid_corr::store(s, o.min_count, (i0 + i) * g.nc + j0 + lane, o.corr, o.count, o.sums);
        }
    }
}

__device__ __forceinline__ int64_t wave_sum(int64_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)(uint64_t)v, d, 64);
        const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)((uint64_t)v >> 32), d, 64);
        v += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return v;                                                // (the sum in lane 0)
}

// The sums of one window by the lanes of a wavefront (`lane`, `lanes` = 0, 1 on the host): every lane its share
__host__ __device__ inline Sums window_share(const Img &im, int w, int64_t rc, int64_t cc, int lane, int lanes)
{
    Sums s = {0, 0, 0, 0, 0, 0};
    int64_t r_lo, r_hi, c_lo, c_hi;
    sid_corr::clip(rc, w, im.rows, r_lo, r_hi);
    sid_corr::clip(cc, w, im.cols, c_lo, c_hi);
    const uint32_t wc = (uint32_t)(c_hi - c_lo), total = (uint32_t)(r_hi - r_lo) * wc;
    for (uint32_t idx = (uint32_t)lane; idx < total; idx += (uint32_t)lanes) {
        const uint32_t dr = idx / wc, dc = idx - dr * wc;
        sid_corr::add_pixel(s, im.a[(r_lo + dr) * im.a_stride + c_lo + dc], im.b[(r_lo + dr) * im.b_stride + c_lo + dc]);
    }
    return s;
}

__global__ __launch_bounds__(kBlock) void k_corr_points(Img im, int w, const int32_t *__restrict__ c, const int32_t *__restrict__ r,
                                                        const uint8_t *__restrict__ valid, int64_t npts, Out o)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    for (int64_t k = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); k < npts; k += stride) {      // (uniform in a wavefront)
        Sums s = {0, 0, 0, 0, 0, 0};
        if (!valid || valid[k]) s = window_share(im, w, r[k], c[k], lane, 64);
        s.n = wave_sum(s.n); s.sa = wave_sum(s.sa); s.sb = wave_sum(s.sb);
        s.saa = wave_sum(s.saa); s.sbb = wave_sum(s.sbb); s.sab = wave_sum(s.sab);
        if (lane == 0) sid_corr::store(s, o.min_count, k, o.corr, o.count, o.sums);
    }
}

__global__ __launch_bounds__(kBlock) void k_corr_lattice_plain(Img im, Lattice g, Out o)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kWaves, nodes = g.nr * g.nc;
    for (int64_t k = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); k < nodes; k += stride) {     // (uniform in a wavefront)
        const int64_t i = k / g.nc, j = k - i * g.nc;
        Sums s = window_share(im, g.w, sid_corr::centre(g.r0, i, g.sr), sid_corr::centre(g.c0, j, g.sc), lane, 64);
        s.n = wave_sum(s.n); s.sa = wave_sum(s.sa); s.sb = wave_sum(s.sb);
        s.saa = wave_sum(s.saa); s.sbb = wave_sum(s.sbb); s.sab = wave_sum(s.sab);
        if (lane == 0) sid_corr::store(s, o.min_count, k, o.corr, o.count, o.sums);
    }
}

// ---------------------------------------------------------------- host instance
void host_lattice(const Img &im, const Lattice &g, const Out &o)
{
    for (int64_t i = 0; i < g.nr; ++i)
        for (int64_t j = 0; j < g.nc; ++j)
            sid_corr::store(window_share(im, g.w, sid_corr::centre(g.r0, i, g.sr), sid_corr::centre(g.c0, j, g.sc), 0, 1), o.min_count,
                            i * g.nc + j, o.corr, o.count, o.sums);
}

void host_points(const Img &im, int w, const int32_t *c, const int32_t *r, const uint8_t *valid, int64_t npts, const Out &o)
{
    for (int64_t k = 0; k < npts; ++k) {
        Sums s = {0, 0, 0, 0, 0, 0};
        if (!valid || valid[k]) s = window_share(im, w, r[k], c[k], 0, 1);
        sid_corr::store(s, o.min_count, k, o.corr, o.count, o.sums);
    }
}

// ---------------------------------------------------------------- arguments
bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

size_t plane_bytes(int64_t rows, int64_t cols, int64_t stride)
{
    return rows > 0 && cols > 0 ? (size_t)(rows - 1) * (size_t)stride + (size_t)cols : 0;
}

// What the two entry points share; `nodes` is nr * nc or npts (checked to be in range by the caller)
int check_common(const Img &im, int w, int64_t nodes, const Out &o)
{
    if (!im.a || !im.b) return fail(SID_PM_ERR_ARG, "null image");
    if (!o.corr && !o.count && !o.sums) return fail(SID_PM_ERR_ARG, "no output");
    if (im.rows < 0 || im.cols < 0) return fail(SID_PM_ERR_ARG, "negative image size %lld x %lld", (long long)im.rows, (long long)im.cols);
    if (im.a_stride < im.cols || im.b_stride < im.cols)
        return fail(SID_PM_ERR_ARG, "a row stride (%lld, %lld) below cols %lld", (long long)im.a_stride, (long long)im.b_stride, (long long)im.cols);
    if (o.min_count < 1) return fail(SID_PM_ERR_ARG, "min_count must be >= 1 (got %lld)", (long long)o.min_count);
    if (w < 1 || w > 255) return fail(SID_PM_ERR_UNSUPPORTED, "window side %d outside 1..255", w);
    if (im.rows > 0x7fffffffLL || im.cols > 0x7fffffffLL)
        return fail(SID_PM_ERR_UNSUPPORTED, "an image axis >= 2^31 (%lld x %lld)", (long long)im.rows, (long long)im.cols);
    const size_t na = plane_bytes(im.rows, im.cols, im.a_stride), nb = plane_bytes(im.rows, im.cols, im.b_stride);
    const void *outs[3] = {o.corr, o.count, o.sums};
    const size_t sizes[3] = {8 * (size_t)nodes, 4 * (size_t)nodes, 40 * (size_t)nodes};
    for (int k = 0; k < 3; ++k)
        if (outs[k] && (overlap(outs[k], sizes[k], im.a, na) || overlap(outs[k], sizes[k], im.b, nb)))
            return fail(SID_PM_ERR_ARG, "an output overlaps an image");
    return SID_PM_OK;
}

int check_lattice(const Img &im, int w, int64_t sr, int64_t sc, int64_t nr, int64_t nc, const Out &o)
{
    if (nr < 0 || nc < 0) return fail(SID_PM_ERR_ARG, "negative lattice size %lld x %lld", (long long)nr, (long long)nc);
    if (sr < 1 || sc < 1) return fail(SID_PM_ERR_ARG, "steps must be >= 1 (got %lld, %lld)", (long long)sr, (long long)sc);
    if (nr > 0 && nc > 0x7fffffffLL / nr) return fail(SID_PM_ERR_UNSUPPORTED, "nr * nc >= 2^31 (%lld x %lld)", (long long)nr, (long long)nc);
    return check_common(im, w, nr * nc, o);
}

int check_points(const Img &im, int w, const int32_t *c, const int32_t *r, int64_t npts, const Out &o)
{
    if (npts < 0) return fail(SID_PM_ERR_ARG, "negative npts %lld", (long long)npts);
    if (npts > 0x7fffffffLL) return fail(SID_PM_ERR_UNSUPPORTED, "npts >= 2^31 (%lld)", (long long)npts);
    if (npts > 0 && (!c || !r)) return fail(SID_PM_ERR_ARG, "null centres");
    return check_common(im, w, npts, o);
}

Lattice lattice_of(int w, int64_t r0, int64_t c0, int64_t sr, int64_t sc, int64_t nr, int64_t nc)
{
    return {r0, c0, sr, sc, nr, nc, w, (int)(sr < w ? sr : w), (int)(sc < w ? sc : w)};
}

// ---------------------------------------------------------------- launches
int launch_lattice(const Img &im, const Lattice &g, const Out &o, hipStream_t st)
{
    if (g.nr == 0 || g.nc == 0) return SID_PM_OK;
    if (g.sr >= g.w && g.sc >= g.w) {                                              // nothing shared: a wavefront per node
        const int64_t want = (g.nr * g.nc + kWaves - 1) / kWaves;
        hipLaunchKernelGGL(k_corr_lattice_plain, dim3((unsigned)(want < kPlainBlocks ? want : kPlainBlocks)), dim3(kBlock), 0, st, im, g, o);
        return launched("k_corr_lattice_plain");
    }
    const int64_t tiles_r = (g.nr + kTR - 1) / kTR, tiles_c = (g.nc + kTC - 1) / kTC;
    const int64_t widest = ((g.nc < kTC ? g.nc : kTC) - 1) * g.cp + g.w;          // slots of the widest tile's row
    const dim3 grid((unsigned)(tiles_r * tiles_c));                                  // (nr * nc < 2^31)
    if ((widest + 3) / 4 <= kSegSmall) hipLaunchKernelGGL(k_corr_lattice<kSegSmall>, grid, dim3(kBlock), 0, st, im, g, o, tiles_c);
    else hipLaunchKernelGGL(k_corr_lattice<kSegLarge>, grid, dim3(kBlock), 0, st, im, g, o, tiles_c);
    return launched("k_corr_lattice");
}

int launch_points(const Img &im, int w, const int32_t *c, const int32_t *r, const uint8_t *valid, int64_t npts, const Out &o, hipStream_t st)
{
    if (npts == 0) return SID_PM_OK;
    const int64_t want = (npts + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(k_corr_points, dim3((unsigned)(want < kPlainBlocks ? want : kPlainBlocks)), dim3(kBlock), 0, st, im, w, c, r, valid, npts, o);
    return launched("k_corr_points");
}

DevicePool<> g_pool;

int current_device(int &device)
{
    if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= kMaxDevices) return fail(SID_PM_ERR_NODEVICE, "no current HIP device");
    return SID_PM_OK;
}

// The frame of the two host-buffer entry points: the images up, `run` on the null stream, the wanted outputs down
template <class Extra, class Run>
int staged(int device, const Img &im, int64_t nodes, const Out &o, Extra extra, Run run)
{
    Staging s;
    if (!s.enter(g_pool, device)) return fail(SID_PM_ERR_NODEVICE, "no such HIP device");
    const size_t npx = (size_t)im.rows * (size_t)im.cols, n = (size_t)nodes;
    uint8_t *d_a, *d_b;
    double *d_corr;
    int32_t *d_count;
    int64_t *d_sums;
    if (int rc = g_pool.carve(device, [&](Carver &c) {
            d_a = c.take<uint8_t>(npx);
            d_b = c.take<uint8_t>(npx);
            d_corr = c.take<double>(n, o.corr != nullptr);
            d_count = c.take<int32_t>(n, o.count != nullptr);
            d_sums = c.take<int64_t>(5 * n, o.sums != nullptr);
            extra(c);
        }))
        return rc;
    if (npx) {
        HIP_TRY(hipMemcpy2DAsync(d_a, (size_t)im.cols, im.a, (size_t)im.a_stride, (size_t)im.cols, (size_t)im.rows, hipMemcpyHostToDevice, 0));
        HIP_TRY(hipMemcpy2DAsync(d_b, (size_t)im.cols, im.b, (size_t)im.b_stride, (size_t)im.cols, (size_t)im.rows, hipMemcpyHostToDevice, 0));
    }
    const Img dim = {d_a, d_b, im.cols, im.cols, im.rows, im.cols};
    const Out dout = {d_corr, d_count, d_sums, o.min_count};
    if (int rc = run(dim, dout)) return rc;
    if (o.corr) HIP_TRY(hipMemcpyAsync(o.corr, d_corr, 8 * n, hipMemcpyDeviceToHost, 0));
    if (o.count) HIP_TRY(hipMemcpyAsync(o.count, d_count, 4 * n, hipMemcpyDeviceToHost, 0));
    if (o.sums) HIP_TRY(hipMemcpyAsync(o.sums, d_sums, 40 * n, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipStreamSynchronize(0));
    s.done();
    return SID_PM_OK;
}

}  // namespace

SID_EXPORT const char *sid_corr_last_error(void) { return g_err; }

SID_EXPORT int sid_corr_release(int device) { return g_pool.release(device); }

SID_EXPORT int sid_corr_lattice_device(const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t rows, int64_t cols,
                                       int w, int64_t r0, int64_t c0, int64_t sr, int64_t sc, int64_t nr, int64_t nc, int64_t min_count,
                                       double *corr, int32_t *count, int64_t *sums, void *hip_stream)
{
    const Img im = {a, b, a_stride, b_stride, rows, cols};
    const Out o = {corr, count, sums, min_count};
    if (int rc = check_lattice(im, w, sr, sc, nr, nc, o)) return rc;
    if (nr == 0 || nc == 0) return SID_PM_OK;
    int device = 0;
    if (int rc = current_device(device)) return rc;
    return launch_lattice(im, lattice_of(w, r0, c0, sr, sc, nr, nc), o, reinterpret_cast<hipStream_t>(hip_stream));
}

SID_EXPORT int sid_corr_points_device(const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t rows, int64_t cols,
                                      int w, const int32_t *c, const int32_t *r, const uint8_t *valid, int64_t npts, int64_t min_count,
                                      double *corr, int32_t *count, int64_t *sums, void *hip_stream)
{
    const Img im = {a, b, a_stride, b_stride, rows, cols};
    const Out o = {corr, count, sums, min_count};
    if (int rc = check_points(im, w, c, r, npts, o)) return rc;
    if (npts == 0) return SID_PM_OK;
    int device = 0;
    if (int rc = current_device(device)) return rc;
    return launch_points(im, w, c, r, valid, npts, o, reinterpret_cast<hipStream_t>(hip_stream));
}

SID_EXPORT int sid_corr_lattice(int device, const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t rows, int64_t cols,
                                int w, int64_t r0, int64_t c0, int64_t sr, int64_t sc, int64_t nr, int64_t nc, int64_t min_count,
                                double *corr, int32_t *count, int64_t *sums)
{
    const Img im = {a, b, a_stride, b_stride, rows, cols};
    const Out o = {corr, count, sums, min_count};
    if (int rc = check_lattice(im, w, sr, sc, nr, nc, o)) return rc;
    if (nr == 0 || nc == 0) return SID_PM_OK;
    const Lattice g = lattice_of(w, r0, c0, sr, sc, nr, nc);
    if (device == -1) {
        host_lattice(im, g, o);
        return SID_PM_OK;
    }
    return staged(device, im, nr * nc, o, [](Carver &) {}, [&](const Img &dim, const Out &dout) { return launch_lattice(dim, g, dout, 0); });
}

SID_EXPORT int sid_corr_points(int device, const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int64_t rows, int64_t cols,
                               int w, const int32_t *c, const int32_t *r, const uint8_t *valid, int64_t npts, int64_t min_count,
                               double *corr, int32_t *count, int64_t *sums)
{
    const Img im = {a, b, a_stride, b_stride, rows, cols};
    const Out o = {corr, count, sums, min_count};
    if (int rc = check_points(im, w, c, r, npts, o)) return rc;
    if (npts == 0) return SID_PM_OK;
    if (device == -1) {
        host_points(im, w, c, r, valid, npts, o);
        return SID_PM_OK;
    }
    int32_t *d_c = nullptr, *d_r = nullptr;
    uint8_t *d_valid = nullptr;
    const size_t n = (size_t)npts;
    return staged(device, im, npts, o,
                  [&](Carver &cv) {
                      d_c = cv.take<int32_t>(n);
                      d_r = cv.take<int32_t>(n);
                      d_valid = cv.take<uint8_t>(n, valid != nullptr);
                  },
                  [&](const Img &dim, const Out &dout) {
                      HIP_TRY(hipMemcpyAsync(d_c, c, 4 * n, hipMemcpyHostToDevice, 0));
                      HIP_TRY(hipMemcpyAsync(d_r, r, 4 * n, hipMemcpyHostToDevice, 0));
                      if (d_valid) HIP_TRY(hipMemcpyAsync(d_valid, valid, n, hipMemcpyHostToDevice, 0));
                      return launch_points(dim, w, d_c, d_r, d_valid, npts, dout, 0);
                  });
}
