// Host check of csrc/ft_guided_plan.h: the grid and the workspace of the guided matcher (include/sid_ftg.h), g++ only.  Over
//   radii   0, 2^-1000, 1e-300, 1e-12, 0.5, 1, 5, 7.25, 60, 135, 540, 1e4, 1e9, 1e300, the largest double  (+ seeded random ones),
//   extents 0, 2^-1060, 1e-9, 1, 299, 400, 5000, 1e6, 1e7, 1e300, overflowing                              (+ seeded random ones),
//   offsets 0, +-0.5, +-1e7, +-1e15, +-1e300, and caps 1, 2, 3, 37, 317, 1024:
//   cells      1 <= n <= cap along the axis, the side is >= radius * (1 + 2^-20), >= 2^-500 and >= extent / cap
//   total      cell_of is within 0 .. n - 1 for points inside the box, outside it, at +-inf and not a number, and monotone
//   adjacent   pairs (a, b) that satisfy the inclusion rule fl(dx dx) + fl(dy dy) <= fl(r r) - b exactly one radius from a, a few
//              ulps either side of that, a on and a few ulps either side of every kind of cell boundary, Pythagorean (3, 4, 5)
//              offsets on both axes - lie in the same or in neighbouring cells
//   empty box  lo > hi (no finite train position): one cell
//   regions    every region of the workspace starts on a multiple of 256 bytes, they follow one another without overlap and end
//              within workspace_bytes; the two count regions are adjacent in the order the one fill relies on; the item bound
//              holds for every way of spreading n1 queries over the cells that was tried
//   limits     n2 = 2^22 - 1 is accepted, 2^22 is not; radius_ok
// Prints "<n> checks" and "<v> violations"; exit status 1 on a violation.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <limits>
#include <random>
#include <vector>

#include "../../sea_ice_drift_amd/csrc/ft_guided_plan.h"

namespace {

using sid_ftg::Axis;

long g_checks = 0, g_bad = 0;

void expect(bool ok, const char *what, double lo, double extent, double radius, int cap, double a = 0.0, double b = 0.0)
{
    ++g_checks;
    if (ok) return;
    if (++g_bad <= 20) printf("%s: lo = %.17g, extent = %.17g, radius = %.17g, cap = %d, a = %.17g, b = %.17g\n", what, lo, extent, radius, cap, a, b);
}

double step(double v, int ulps)
{
    for (int k = 0; k < abs(ulps); ++k) v = nextafter(v, ulps > 0 ? INFINITY : -INFINITY);
    return v;
}

// the rule of include/sid_ftg.h, for one axis (dy = 0) or two
bool inside(double dx, double dy, double r) { return dx * dx + dy * dy <= r * r; }

void check_pair(const Axis &ax, double lo, double extent, double radius, int cap, double a, double b)
{
    if (!isfinite(a) || !isfinite(b)) return;
    if (!inside(b - a, 0.0, radius)) return;
    const int ca = sid_ftg::cell_of(ax, a), cb = sid_ftg::cell_of(ax, b);
    expect(abs(ca - cb) <= 1, "adjacent", lo, extent, radius, cap, a, b);
}

void check_axis(double lo, double extent, double radius, int cap, std::mt19937_64 &rng)
{
    const double hi = lo + extent;
    const Axis ax = sid_ftg::make_axis(lo, hi, radius, cap);
    const double span = hi - lo;                                       // (what make_axis sees: lo + extent is rounded)
    expect(ax.n >= 1 && ax.n <= cap && ax.n <= sid_ftg::kMaxAxis, "cells within the cap", lo, extent, radius, cap);
    expect(ax.cell >= radius * sid_ftg::kMargin && ax.cell >= sid_ftg::kMinCell && ax.cell >= span / cap, "cell side", lo, extent, radius, cap);
    if (span == 0.0 || !isfinite(span)) expect(ax.n == 1, "degenerate box: one cell", lo, extent, radius, cap);
    // points: the ends, the cell boundaries, outside, not finite
    std::vector<double> pts = {lo, hi, step(lo, 1), step(lo, -1), step(hi, 1), step(hi, -1), lo - radius, hi + radius, lo - 3 * ax.cell, hi + 3 * ax.cell,
                               0.0, -1e300, 1e300, std::numeric_limits<double>::max(), -std::numeric_limits<double>::max()};
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    std::uniform_int_distribution<int> anyk(0, ax.n);
    for (int s = 0; s < 12; ++s) {
        const int k = s < 4 ? s : s < 8 ? ax.n - (s - 4) : anyk(rng);
        const double edge = lo + k * ax.cell;
        for (int u = -3; u <= 3; ++u) pts.push_back(step(edge, u));
        pts.push_back(lo + (k + unit(rng)) * ax.cell);
    }
    int prev = -1;
    double prev_p = 0.0;
    std::vector<double> finite;
    for (double p : pts) if (isfinite(p)) finite.push_back(p);
    std::sort(finite.begin(), finite.end());
    for (double p : finite) {
        const int c = sid_ftg::cell_of(ax, p);
        expect(c >= 0 && c < ax.n, "cell inside the grid", lo, extent, radius, cap, p);
        expect(c >= prev, "monotone", lo, extent, radius, cap, prev_p, p);
        if (p >= lo && p <= hi && isfinite(span)) expect((double)c <= floor((p - lo) / ax.cell) && c >= 0, "cell of a point of the box", lo, extent, radius, cap, p);
        prev = c; prev_p = p;
    }
    for (double p : {(double)INFINITY, (double)-INFINITY, (double)NAN}) {
        const int c = sid_ftg::cell_of(ax, p);
        expect(c >= 0 && c < ax.n, "cell of a position that is not finite", lo, extent, radius, cap, p);
    }
    // pairs within the radius
    for (double a : finite) {
        for (int u = -4; u <= 4; ++u) {
            check_pair(ax, lo, extent, radius, cap, a, step(a + radius, u));
            check_pair(ax, lo, extent, radius, cap, a, step(a - radius, u));
            check_pair(ax, lo, extent, radius, cap, step(a - radius, u), a);
        }
        check_pair(ax, lo, extent, radius, cap, a, a + radius * unit(rng));
        check_pair(ax, lo, extent, radius, cap, a, a);
        check_pair(ax, lo, extent, radius, cap, a, a + 0x1p-538);                       // squares that underflow: inside any radius
        // Pythagorean offsets: (3, 4) scaled so that the hypotenuse is the radius exactly where that is representable
        const double k = radius / 5.0;
        if (inside(3 * k, 4 * k, radius)) {
            expect(abs(sid_ftg::cell_of(ax, a) - sid_ftg::cell_of(ax, a + 3 * k)) <= 1 || !inside((a + 3 * k) - a, 4 * k, radius), "adjacent (3 of 3, 4, 5)", lo, extent, radius, cap, a);
            expect(abs(sid_ftg::cell_of(ax, a) - sid_ftg::cell_of(ax, a + 4 * k)) <= 1 || !inside(3 * k, (a + 4 * k) - a, radius), "adjacent (4 of 3, 4, 5)", lo, extent, radius, cap, a);
        }
    }
}

void check_regions(int64_t n1, int64_t n2, std::mt19937_64 &rng)
{
    const sid_ftg::Regions R = sid_ftg::regions(n1, n2);
    auto bad = [&](const char *what) { expect(false, what, (double)n1, (double)n2, 0.0, R.cap); };
    ++g_checks;
    if (R.cap < 1 || R.cap > sid_ftg::kMaxAxis || ((int64_t)(R.cap - 1) * (R.cap - 1) >= n2 && R.cap > 1) || ((int64_t)R.cap * R.cap < n2 && R.cap < sid_ftg::kMaxAxis))
        bad("axis cap = ceil(sqrt(n2)) in 1 .. 1024");
    size_t end = 0;
    for (int r = 0; r < sid_ftg::kRegions; ++r) {
        ++g_checks;
        if (R.off[r] % 256 != 0) bad("regions: alignment");
        if (R.off[r] < end) bad("regions: overlap");
        if (R.bytes[r] == 0) bad("regions: empty");
        end = R.off[r] + R.bytes[r];
    }
    ++g_checks;
    if ((int64_t)end > sid_ftg::workspace_bytes(n1, n2) || (int64_t)R.total != sid_ftg::workspace_bytes(n1, n2)) bad("regions: within the workspace");
    ++g_checks;
    if (R.off[sid_ftg::kQCount] <= R.off[sid_ftg::kTCount] || sid_ftg::kQCount != sid_ftg::kTCount + 1) bad("regions: the counts are adjacent");
    const size_t q = n1 > 0 ? n1 : 1, t = n2 > 0 ? n2 : 1, c = (size_t)R.cells_cap;
    ++g_checks;
    if (R.bytes[sid_ftg::kGridR] < sizeof(sid_ftg::Grid) || R.bytes[sid_ftg::kBox] < 32 * (size_t)sid_ftg::kBoxBlocks || R.bytes[sid_ftg::kTCount] < 4 * c ||
        R.bytes[sid_ftg::kQCount] < 4 * c || R.bytes[sid_ftg::kTStart] < 4 * (c + 1) || R.bytes[sid_ftg::kQStart] < 4 * (c + 1) ||
        R.bytes[sid_ftg::kIStart] < 4 * (c + 1) || R.bytes[sid_ftg::kTCell] < 4 * t || R.bytes[sid_ftg::kTRank] < 4 * t || R.bytes[sid_ftg::kQCell] < 4 * q ||
        R.bytes[sid_ftg::kQRank] < 4 * q || R.bytes[sid_ftg::kSDesc] < 32 * t || R.bytes[sid_ftg::kSTx] < 8 * t || R.bytes[sid_ftg::kSTy] < 8 * t ||
        R.bytes[sid_ftg::kSIdx] < 4 * t || R.bytes[sid_ftg::kQOrder] < 4 * q || R.bytes[sid_ftg::kItems] < 8 * (size_t)R.items)
        bad("regions: sizes");
    // the item bound: all queries in one cell, one query per cell, and random spreads
    ++g_checks;
    const int64_t cells = R.cells_cap;
    if ((n1 + 255) / 256 > R.items) bad("items: one cell");
    if ((n1 < cells ? n1 : cells) + (n1 > cells ? (n1 - cells + 255) / 256 : 0) > R.items) bad("items: one query per cell first");
    if (n1 <= 100000) {
        std::uniform_int_distribution<int64_t> cut(0, n1);
        const int64_t used = 1 + cut(rng) % cells;
        int64_t left = n1, items = 0;
        for (int64_t k = 0; k < used && k < 4096; ++k) {
            const int64_t take = k + 1 == used || k == 4095 ? left : cut(rng) % (left + 1);
            items += (take + 255) / 256;
            left -= take;
        }
        if (items > R.items) bad("items: a random spread");
    }
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261021);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    const double big = std::numeric_limits<double>::max();
    std::vector<double> radii = {0.0, 0x1p-1000, 1e-300, 1e-12, 0.5, 1.0, 5.0, 7.25, 60.0, 135.0, 540.0, 1e4, 1e9, 1e300, big};
    std::vector<double> extents = {0.0, 0x1p-1060, 1e-9, 1.0, 299.0, 400.0, 5000.0, 1e6, 1e7, 1e300, big};
    for (int k = 0; k < 12; ++k) { radii.push_back(exp10(-3.0 + 12.0 * unit(rng))); extents.push_back(exp10(-2.0 + 9.0 * unit(rng))); }
    const double offsets[] = {0.0, 0.5, -0.5, 1e7, -1e7, 1e15, -1e15, 1e300, -1e300, -big};
    const int caps[] = {1, 2, 3, 37, 317, 1024};
    for (double r : radii)
        for (double e : extents)
            for (double lo : offsets)
                for (int cap : caps) check_axis(lo, e, r, cap, rng);
    // cell sides exactly one radius apart on integer lattices (the quotient lands on or a hair beside an integer)
    for (double r : {1.0, 3.0, 5.0, 7.0, 0.1, 1.0 / 3.0})
        for (double lo : {0.0, -1e7, 1e7, 0.1})
            for (int cap : {317, 1024}) {
                const Axis ax = sid_ftg::make_axis(lo, lo + 1000 * r, r, cap);
                for (int k = -2; k < 1003; ++k)
                    for (int u = -2; u <= 2; ++u) {
                        const double a = step(lo + k * r, u);
                        check_pair(ax, lo, 1000 * r, r, cap, a, a + r);
                        check_pair(ax, lo, 1000 * r, r, cap, a, step(a + r, 1));
                        check_pair(ax, lo, 1000 * r, r, cap, a - r, a);
                    }
            }
    {   // no finite train position
        const Axis ax = sid_ftg::make_axis(INFINITY, -INFINITY, 5.0, 1024);
        expect(ax.n == 1 && sid_ftg::cell_of(ax, 1e300) == 0 && sid_ftg::cell_of(ax, NAN) == 0 && sid_ftg::cell_of(ax, -INFINITY) == 0, "empty box", INFINITY, 0, 5.0, 1024);
    }
    const int64_t a1[] = {0, 1, 255, 256, 257, 700, 1000, 100000, (int64_t)1 << 20, 0x7fffffff / 4};
    const int64_t a2[] = {0, 1, 2, 3, 4, 5, 255, 1300, 100000, (int64_t)1 << 20, ((int64_t)1 << 20) + 1, ((int64_t)1 << 22) - 1};
    for (int64_t n1 : a1)
        for (int64_t n2 : a2) check_regions(n1, n2, rng);
    for (int k = 0; k < 5000; ++k) check_regions((int64_t)exp2(21.0 * unit(rng)) - 1, (int64_t)exp2(22.0 * unit(rng)) - 1, rng);
    const int64_t t = (int64_t)1 << 22, q = 0x7fffffff / 4;
    expect(sid_ftg::sizes_supported(1, t - 1) && !sid_ftg::sizes_supported(1, t), "limit: n2", 0, 0, 0, 0);
    expect(sid_ftg::sizes_supported(q, 1) && !sid_ftg::sizes_supported(q + 1, 1), "limit: n1", 0, 0, 0, 0);
    expect(sid_ftg::workspace_bytes(-1, 5) == 0 && sid_ftg::workspace_bytes(5, -1) == 0 && sid_ftg::workspace_bytes(1, t) == 0, "sizes the entry does not accept", 0, 0, 0, 0);
    expect(sid_ftg::radius_ok(0.0) && sid_ftg::radius_ok(big) && !sid_ftg::radius_ok(-1.0) && !sid_ftg::radius_ok(-0x1p-1074) && !sid_ftg::radius_ok(NAN) &&
           !sid_ftg::radius_ok(INFINITY), "radius_ok", 0, 0, 0, 0);
    printf("%ld checks\n%ld violations\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
