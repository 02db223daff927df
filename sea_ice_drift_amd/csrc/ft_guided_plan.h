// ft_guided_plan.h - the plan of the guided Hamming matcher of include/sid_ftg.h (csrc/ft_guided.hip):
// the uniform grid laid over the bounding box of the finite train positions, the cell of a point, the bound of the work list
// and the regions of the workspace.  Plain C++ (no HIP), so that tests/cpp/ft_guided_plan_check.cpp compiles it alone.  The
// device entry may not read anything back, so the grid is made ON the device from the box the kernels find - by make_axis
// below, compiled for the device from this very text (IEEE float64 division and floor, no contraction): what the check
// sweeps on the host is what the kernels index with.
//
// Why "inside the radius" means "adjacent cells".  The inclusion rule (sid_ftg.h) is fl(fl(dx dx) + fl(dy dy)) <= fl(r r).  With
// u = 2^-53 it gives |dx| <= r (1 + 2u) + 2^-537 (the second term: squares that underflow), and the true distance along the
// axis is at most |dx| (1 + u).  The cell of p is floor(fl(fl(p - x0) / cell)), clamped to 0 .. n - 1: monotone in p.  Two
// points a <= b whose unclamped quotients differ by at most 1 lie in the same or in neighbouring cells.  Both quotients are
// below 1026 wherever the clamp does not merge them anyway, so their two roundings each add at most 1026 * 2u = 2.3e-13, and
//     t(b) - t(a) <= (r (1 + 4u) + 2^-536) / cell + 4.6e-13 <= (1 + 4u) / (1 + 2^-20) + 2^-36 + 4.6e-13 < 1 - 9e-7
// because cell >= r (1 + 2^-20) (kMargin; its own rounding is another u) and cell >= 2^-500 (kMinCell).
#ifndef SID_FT_GUIDED_PLAN_H
#define SID_FT_GUIDED_PLAN_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef SID_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SID_HD __host__ __device__
#else
#define SID_HD
#endif
#endif
#ifndef SID_HD_INLINE
#define SID_HD_INLINE SID_HD inline __attribute__((always_inline))
#endif

namespace sid_ftg {

constexpr int kThreads = 256;                               // threads of every kernel but the scan; queries of one work item
constexpr int kScanThreads = 1024;
constexpr uint32_t kNone = 0xffffffffu;
constexpr int64_t kMaxTrain = (int64_t)1 << 22;             // index bits of the key, as sid_ft_knn2
constexpr int64_t kMaxQueries = 0x7fffffff / 4;             // (32-bit query numbers index the outputs)
constexpr int kMaxAxis = 1024;                              // cells per axis at the most
constexpr int kBoxBlocks = 256;                             // partial bounding boxes
constexpr double kMargin = 1.0 + 0x1p-20;                   // cell side >= radius * kMargin
constexpr double kMinCell = 0x1p-500;                       // and >= this: far above the 2^-537 of underflowing squares

// One axis of the grid: cell = floor((p - x0) / cell), clamped to 0 .. n - 1
struct Axis {
    double x0, cell;
    int32_t n, pad_;
};
struct Grid {
    Axis x, y;                                              // cell number = cy * x.n + cx
};

// Cells per axis the grid may have for n2 train points: more cells than points buy nothing.  ceil(sqrt(n2)) in 1 .. kMaxAxis.
inline int32_t axis_cap(int64_t n2)
{
    int64_t a = 1;
    while (a < kMaxAxis && a * a < n2) ++a;
    return (int32_t)a;
}

// The axis over [lo, hi] (the finite train positions; lo > hi: there are none) for `radius` (finite, >= 0) with at most `cap`
// cells.  The side is at least radius * kMargin, at least extent / cap and at least kMinCell; an extent of zero, one that
// overflows or a side that overflows gives ONE cell (every quotient is then 0 or not a number, and cell_of sends both to 0).
SID_HD_INLINE Axis make_axis(double lo, double hi, double radius, int32_t cap)
{
    Axis a;
    a.x0 = 0.0;
    a.cell = fmax(radius * kMargin, kMinCell);
    a.n = 1;
    a.pad_ = 0;
    if (cap < 1) cap = 1;
    if (!(lo <= hi)) return a;
    a.x0 = lo;
    const double extent = hi - lo;
    a.cell = fmax(a.cell, extent / (double)cap);
    const double t = floor(extent / a.cell);               // (inf / inf is not a number: one cell)
    if (t > 0.0) a.n = t >= (double)(cap - 1) ? cap : (int32_t)t + 1;
    return a;
}

// Total and monotone in p: what is not above 0 (not a number included) is cell 0
SID_HD_INLINE int32_t cell_of(const Axis &a, double p)
{
    const double t = floor((p - a.x0) / a.cell);
    if (!(t > 0.0)) return 0;
    if (t >= (double)(a.n - 1)) return a.n - 1;
    return (int32_t)t;
}

// Work items: one per (query cell, run of up to kThreads of its queries).  sum ceil(q_c / kThreads) over the cells that hold
// queries is at most n1 / kThreads + the number of such cells.
inline int64_t max_items(int64_t n1, int64_t cells_cap)
{
    return n1 / kThreads + (n1 < cells_cap ? n1 : cells_cap) + 1;
}

// The regions of the workspace, in order.  Every region starts on a multiple of 256 bytes.
enum Region {
    kGridR, kBox, kTCount, kQCount, kTStart, kQStart, kIStart, kTCell, kTRank, kQCell, kQRank, kSDesc, kSTx, kSTy, kSIdx, kQOrder,
    kItems, kRegions
};
struct Regions {
    size_t off[kRegions], bytes[kRegions], total;
    int32_t cap;                                            // cells per axis at the most
    int64_t cells_cap, items;                               // cap * cap; max_items
};
inline Regions regions(int64_t n1, int64_t n2)
{
    Regions R;
    R.cap = axis_cap(n2);
    R.cells_cap = (int64_t)R.cap * R.cap;
    R.items = max_items(n1, R.cells_cap);
    const size_t q = (size_t)(n1 > 0 ? n1 : 1), t = (size_t)(n2 > 0 ? n2 : 1), c = (size_t)R.cells_cap;
    const size_t want[kRegions] = {
        sizeof(Grid), sizeof(double) * 4 * kBoxBlocks,
        4 * c, 4 * c,                                       // points per cell: train, queries (zeroed together: kept adjacent)
        4 * (c + 1), 4 * (c + 1), 4 * (c + 1),              // exclusive prefix sums: train, queries, work items
        4 * t, 4 * t, 4 * q, 4 * q,                         // cell and rank within the cell: train, queries
        32 * t, 8 * t, 8 * t, 4 * t,                        // the train set in cell order: descriptors, x, y, original index
        4 * q,                                              // the queries in cell order
        8 * (size_t)R.items,                                // (cell, run) of every work item
    };
    size_t off = 0;
    for (int r = 0; r < kRegions; ++r) {
        R.off[r] = off;
        R.bytes[r] = want[r];
        off += (want[r] + 255) / 256 * 256;
    }
    R.total = off;
    return R;
}

inline bool sizes_supported(int64_t n1, int64_t n2) { return n1 >= 0 && n2 >= 0 && n1 <= kMaxQueries && n2 < kMaxTrain; }
inline bool radius_ok(double radius) { return radius >= 0.0 && isfinite(radius); }

inline int64_t workspace_bytes(int64_t n1, int64_t n2)
{
    if (!sizes_supported(n1, n2)) return 0;
    return (int64_t)regions(n1, n2).total;
}

}  // namespace sid_ftg

#endif
