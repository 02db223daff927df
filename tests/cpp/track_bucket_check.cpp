// Host check of csrc/track_bucket.h: the bucket index of the point search of include/sid_track.h is one monotone function of a
// coordinate, so a point inside a cell's box never falls outside the cell's bucket range.  Over seeded axes - ordinary spans,
// spans of a few denormals, min == max, spans that overflow, boxes of 1e300, an empty box, non-finite ends - and seeded
// coordinates around and far from them (the ends themselves, +-inf and NaN among them):
//   range         0 <= bucket < n
//   monotone      p <= q  gives  bucket(p) <= bucket(q)              (sorted coordinates, neighbours compared)
//   containment   lo <= p <= hi  gives  bucket(lo) <= bucket(p) <= bucket(hi)
// Built with -fsanitize=address,undefined: a cast of a value that an int cannot hold would stop it.
// Prints "<n> checks, <v> violations"; exit status 1 on a violation.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <random>
#include <vector>

#include "../../sea_ice_drift_amd/csrc/track_bucket.h"

namespace {

using sid_track::Axis;

long g_checks = 0, g_bad = 0;

void expect(bool ok, const char *what, const Axis &a, double p, double q)
{
    ++g_checks;
    if (ok) return;
    if (++g_bad <= 20) printf("%s: x0 = %a, inv = %a, n = %d, p = %a, q = %a\n", what, a.x0, a.inv, a.n, p, q);
}

void check_axis(const Axis &a, std::vector<double> pts)
{
    std::sort(pts.begin(), pts.end());
    int32_t prev = 0;
    for (size_t k = 0; k < pts.size(); ++k) {
        const int32_t b = sid_track::bucket(a, pts[k]);
        expect(b >= 0 && b < a.n, "range", a, pts[k], 0.0);
        if (k) expect(prev <= b, "monotone", a, pts[k - 1], pts[k]);
        prev = b;
    }
    // every pair (lo, hi) of a thinned list as a box, every point between them inside it
    const size_t step = pts.size() / 40 + 1;
    for (size_t i = 0; i < pts.size(); i += step)
        for (size_t j = i; j < pts.size(); j += step) {
            const int32_t b0 = sid_track::bucket(a, pts[i]), b1 = sid_track::bucket(a, pts[j]);
            for (size_t k = i; k <= j; k += step / 3 + 1) {
                const int32_t b = sid_track::bucket(a, pts[k]);
                expect(b0 <= b && b <= b1, "containment", a, pts[i], pts[k]);
            }
        }
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261021);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    const double den = 4.9406564584124654e-324, big = 1e300, inf = INFINITY;
    struct Span { double lo, hi; };
    std::vector<Span> spans = {{0.0, 100.0}, {-37.25, 9012.5}, {5.0, 5.0}, {0.0, 0.0}, {0.0, den}, {-3 * den, 5 * den}, {1.0, 1.0 + 2.220446049250313e-16},
                               {-big, big}, {-1.7e308, 1.7e308}, {big, 1.0001 * big}, {-1e-310, 1e-310}, {1e15, 1e15 + 2.0},
                               {inf, -inf}, {-inf, inf}, {0.0, inf}, {NAN, 1.0}, {1.0, NAN}, {3.0, 2.0}};
    for (int k = 0; k < 40; ++k) {
        const double c = (unit(rng) - 0.5) * pow(10.0, 12.0 * unit(rng)), w = pow(10.0, 16.0 * unit(rng) - 8.0);
        spans.push_back({c, c + w});
    }
    const int32_t counts[] = {1, 2, 3, 39, 199, 4096, 0x7fffffff, 0, -5};
    for (const Span &s : spans)
        for (int32_t n : counts) {
            const Axis a = sid_track::make_axis(s.lo, s.hi, n);
            expect(a.n >= 1 && a.inv >= 0.0 && isfinite(a.inv) && isfinite(a.x0), "axis", a, s.lo, s.hi);
            std::vector<double> pts = {s.lo, s.hi, 0.0, -0.0, den, -den, big, -big, 1.7e308, -1.7e308, inf, -inf};
            const double lo = isfinite(s.lo) ? s.lo : 0.0, hi = isfinite(s.hi) ? s.hi : 1.0, w = hi - lo;
            for (int k = 0; k < 400; ++k) {
                const double u = unit(rng);
                pts.push_back(lo + u * w);                               // inside
                pts.push_back(lo + (3.0 * u - 1.0) * w);                 // around
                pts.push_back(nextafter(lo, k & 1 ? inf : -inf) + k * den);
                pts.push_back((u - 0.5) * pow(10.0, 600.0 * unit(rng) - 300.0));
                pts.push_back(lo + (isfinite(w) ? w : 1.0) * (double)k / 400.0 * (a.n > 1 ? 1.0 : 0.5));   // on bucket borders, nearly
            }
            pts.erase(std::remove_if(pts.begin(), pts.end(), [](double v) { return v != v; }), pts.end());
            check_axis(a, pts);
            expect(sid_track::bucket(a, NAN) == 0, "not a number", a, NAN, 0.0);
        }
    printf("%ld checks, %ld violations\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
