// Host check of csrc/ncc_norm.h (the shortened normalisation of the winner's NCC matrix) against the specification written
// out here: IEEE double, 1 / sqrt with two roundings, no fused operation.  Build with -ffp-contract=off.
// Seeds of three qualities stand in for v_rsq_f64: correctly rounded, rounded to float32, perturbed by +-2^-20 relative.
//   (a) >= 10^7 random physical inputs per seed (|q| <= 0.999, dI > N; sides 2, 34, 35, 64, 255): unflagged values bit-equal to
//       the specification, at most 20 flagged in 10^7
//   (b) constructed inputs: the final value is the specification's, every inf / NaN is flagged
//   (c) the fma forms of dI and numer equal the mul / sub forms on extreme integers at side 255
// Prints counts and ends with "<n> violations".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../sea_ice_drift_amd/csrc/ncc_norm.h"

typedef uint32_t u32;
typedef unsigned long long u64;

// ---- the specification, written out ----
static float spec(int p, int swp, u32 siiv, double nd, double sT, double rTd, bool cT)
{
    const double swd = (double)swp, siid = (double)siiv;
    const double dI = nd * siid - swd * swd;
    const double s2 = siid + 256.0 * swd + 16384.0 * nd;
    const bool lowvar = (2.0 * dI <= nd) && (dI * 8388608.0 <= 10.0 * nd * s2);
    const double numer = nd * (double)p - swd * sT;
    if (cT) return 1.0f;
    if (lowvar) return 0.0f;
    const double rI = 1.0 / std::sqrt(dI);
    double q = numer * rI;
    q = q * rTd;
    const double aq = std::fabs(q);
    return aq < 1.0 ? (float)q : (aq < 1.125 ? (q > 0.0 ? 1.0f : -1.0f) : 0.0f);
}

// ---- seeds ----
struct SeedExact { double operator()(double x) const { return (double)(1.0L / sqrtl((long double)x)); } };
struct SeedF32 { double operator()(double x) const { return (double)(float)(1.0 / std::sqrt(x)); } };
struct SeedPert {
    mutable u32 n = 0;
    double operator()(double x) const { const double y = 1.0 / std::sqrt(x); return (n++ & 1u) ? y * (1.0 + 0x1p-20) : y * (1.0 - 0x1p-20); }
};

static u64 g_viol = 0;
static void viol(const char *what, int p, int sw, u32 sii, double nd, double sT, double rT, float got, float want)
{
    if (++g_viol <= 20) std::printf("VIOLATION %s: p=%d sw=%d sii=%u nd=%.0f sT=%.0f rT=%a got=%a want=%a\n", what, p, sw, sii, nd, sT, rT, got, want);
}
static bool same(float a, float b) { u32 x, y; std::memcpy(&x, &a, 4); std::memcpy(&y, &b, 4); return x == y; }

static u64 g_st = 0x243f6a8885a308d3ull;
static u64 rnd() { g_st ^= g_st << 13; g_st ^= g_st >> 7; g_st ^= g_st << 17; return g_st; }

struct In { int p, sw; u32 sii; double nd, sT, rT; };

// one physical input for side s: window and template sums of plausible ranges, |q| <= 0.999 by the specification, dI > N
static In physical(int s)
{
    const int n = s * s;
    const double nd = (double)n;
    for (;;) {
        In v; v.nd = nd;
        v.sT = (double)((long long)(rnd() % (u64)(2 * 128 * n + 1)) - 128ll * n);
        const double dT = 1.0 + (double)(rnd() % (1ull << (20 + (int)(rnd() % 26))));
        v.rT = 1.0 / std::sqrt(dT);
        v.sw = (int)((long long)(rnd() % (u64)(2 * 128 * n + 1)) - 128ll * n);
        const u64 sw2 = (u64)((long long)v.sw * v.sw);
        const u64 sii_min = (sw2 + (u64)n - 1) / (u64)n, sii_max = (u64)n * 16384ull;
        if (sii_min > sii_max) continue;
        const u64 room = sii_max - sii_min;
        v.sii = (u32)(sii_min + (rnd() % (room + 1)) % (1ull << (1 + (int)(rnd() % 30))));
        if ((u64)v.sii > sii_max) continue;
        const double dI = nd * (double)v.sii - (double)v.sw * (double)v.sw;
        if (!(dI > nd)) continue;
        const double f = ((double)(long long)(rnd() % 1998001ull) - 999000.0) / 1000000.0;
        const double target = f * std::sqrt(dI) * std::sqrt(dT);
        const double pd = std::nearbyint((target + (double)v.sw * v.sT) / nd);
        if (!(std::fabs(pd) <= nd * 16384.0)) continue;
        v.p = (int)pd;
        const double q = ((nd * (double)v.p - (double)v.sw * v.sT) * (1.0 / std::sqrt(dI))) * v.rT;
        if (!(std::fabs(q) <= 0.999)) continue;
        return v;
    }
}

template <class Rsq>
static void part_a(const char *name, Rsq rsq, u64 per_side)
{
    const int sides[5] = {2, 34, 35, 64, 255};
    u64 n = 0, flagged = 0;
    for (int si = 0; si < 5; ++si)
        for (u64 i = 0; i < per_side; ++i) {
            const In v = physical(sides[si]);
            const ncc_norm::Hoisted c = ncc_norm::Hoisted::make(v.nd, v.sT, v.rT);
            bool fl; double q;
            const float a = ncc_norm::lean(v.p, v.sw, v.sii, c, rsq, fl, q);
            const float want = spec(v.p, v.sw, v.sii, v.nd, v.sT, v.rT, false);
            ++n;
            if (fl) {
                ++flagged;
                bool sr;
                const float b = ncc_norm::flagged_value(v.p, v.sw, v.sii, c, v.rT, q, sr);
                if (!same(b, want)) viol("a/flagged", v.p, v.sw, v.sii, v.nd, v.sT, v.rT, b, want);
            } else if (!same(a, want)) viol("a/unflagged", v.p, v.sw, v.sii, v.nd, v.sT, v.rT, a, want);
        }
    std::printf("(a) seed %-8s: %llu inputs, %llu flagged (cap %llu)\n", name, n, flagged, 20 * n / 10000000ull);
    if (flagged * 10000000ull > 20 * n) { ++g_viol; std::printf("VIOLATION a/cap: seed %s\n", name); }
}

// (b): final value by the shortened route (all three seeds) against the specification; inf / NaN must be flagged
static u64 g_b = 0, g_b_spec = 0, g_b_nan = 0, g_b_nan_q = 0;   // (g_b_nan_q: q' NaN although dI > N / 2)
static void check_b(const char *what, const In &v, bool cT)
{
    const float want = spec(v.p, v.sw, v.sii, v.nd, v.sT, v.rT, cT);
    const SeedExact s0; const SeedF32 s1; const SeedPert s2;
    bool sr[3];
    const float got[3] = {ncc_norm::from_sums_fast(v.p, v.sw, v.sii, v.nd, v.sT, v.rT, cT, s0, sr[0]),
                          ncc_norm::from_sums_fast(v.p, v.sw, v.sii, v.nd, v.sT, v.rT, cT, s1, sr[1]),
                          ncc_norm::from_sums_fast(v.p, v.sw, v.sii, v.nd, v.sT, v.rT, cT, s2, sr[2])};
    for (int i = 0; i < 3; ++i) {
        if (!same(got[i], want)) viol(what, v.p, v.sw, v.sii, v.nd, v.sT, v.rT, got[i], want);
        if (std::isnan(got[i])) viol("b/nan out", v.p, v.sw, v.sii, v.nd, v.sT, v.rT, got[i], want);
    }
    g_b_spec += sr[0] ? 1 : 0;
    if (!cT) {
        const ncc_norm::Hoisted c = ncc_norm::Hoisted::make(v.nd, v.sT, v.rT);
        bool fl; double q;
        (void)ncc_norm::lean(v.p, v.sw, v.sii, c, s0, fl, q);
        if (std::isnan(q) && v.nd * (double)v.sii - (double)v.sw * (double)v.sw > 0.5 * v.nd) ++g_b_nan_q;
        if (!std::isfinite(q)) { ++g_b_nan; if (!fl) viol("b/nan unflagged", v.p, v.sw, v.sii, v.nd, v.sT, v.rT, (float)q, want); }
    }
    ++g_b;
}

// a base input with dI > N and numer != 0 whose rT is then chosen to put q at `target`
static In with_q(const In &base, double target)
{
    In v = base;
    const double dI = v.nd * (double)v.sii - (double)v.sw * (double)v.sw;
    const double numer = v.nd * (double)v.p - (double)v.sw * v.sT;
    v.rT = target / (numer * (1.0 / std::sqrt(dI)));
    return v;
}

static void part_b()
{
    const int sides[5] = {2, 34, 35, 64, 255};
    for (int si = 0; si < 5; ++si) {
        const int s = sides[si];
        for (int rep = 0; rep < 40; ++rep) {
            In base = physical(s);
            if (base.nd * (double)base.p - (double)base.sw * base.sT == 0.0) continue;
            // float32 rounding midpoints: a float in (2^-20, 1), the midpoint to its successor, +-100 double ulps
            for (int m = 0; m < 8; ++m) {
                u32 fb = 0x35800000u + (u32)(rnd() % (0x3f800000u - 0x35800000u));
                float f0, f1; std::memcpy(&f0, &fb, 4); ++fb; std::memcpy(&f1, &fb, 4);
                const double mid = 0.5 * ((double)f0 + (double)f1);
                u64 mb; std::memcpy(&mb, &mid, 8);
                for (int k = -100; k <= 100; ++k) {
                    const u64 tb = mb + (u64)(long long)k; double t; std::memcpy(&t, &tb, 8);
                    check_b("b/midpoint", with_q(base, t), false);
                    check_b("b/midpoint-", with_q(base, -t), false);
                }
            }
            // the clamp thresholds and their neighbourhoods, and values beyond them
            const double thr[2] = {1.0, 1.125};
            const double eps[] = {0.0, 1e-16, 3e-16, 1e-15, 5e-14, 0.99e-13, 0.999e-13, 1e-13, 1.001e-13, 1.01e-13, 2e-13, 1e-12, 1e-9};
            for (int t = 0; t < 2; ++t)
                for (unsigned e = 0; e < sizeof(eps) / sizeof(eps[0]); ++e)
                    for (int sg = -1; sg <= 1; sg += 2)
                        for (int qs = -1; qs <= 1; qs += 2)
                            check_b("b/threshold", with_q(base, qs * (thr[t] + sg * eps[e])), false);
            u64 one; { const double o = 1.0; std::memcpy(&one, &o, 8); }
            for (int k = -100; k <= 100; ++k) {
                const u64 tb = one + (u64)(long long)k; double t; std::memcpy(&t, &tb, 8);
                check_b("b/one", with_q(base, t), false); check_b("b/one-", with_q(base, -t), false);
                check_b("b/1.125", with_q(base, t * 1.125), false); check_b("b/1.125-", with_q(base, -t * 1.125), false);
            }
            const double beyond[] = {1.0000001, 1.01, 1.06, 1.12, 1.124999, 1.125001, 1.2, 2.0, 17.0, 1e6, 1e300};
            for (unsigned e = 0; e < sizeof(beyond) / sizeof(beyond[0]); ++e) {
                check_b("b/beyond", with_q(base, beyond[e]), false); check_b("b/beyond-", with_q(base, -beyond[e]), false);
            }
            // 1 / sqrt(dT) of a constant template: inf, with and without the flag that goes with it
            In c = base; c.rT = INFINITY;
            check_b("b/constT", c, true); check_b("b/rT inf", c, false);
            c = base; check_b("b/constT finite", c, true);
            // q = NaN with dI > N / 2: numer = 0 (p = 0, sw = 0) times 1 / sqrt(dT) = inf.  Only the compare on |q| can flag it, and
            // only if it is written so that a NaN sets it; the specification answers 0
            In z = base; z.p = 0; z.sw = 0; z.sT = base.sT; z.sii = (u32)(2 * s * s + 1 + rep); z.rT = INFINITY;
            check_b("b/q NaN", z, false);
            z.sT = 0.0; z.sw = (int)(rep % (s + 1)); z.p = 0;              // numer = -sw sT = 0 again, dI = N sii - sw^2 > N
            check_b("b/q NaN 2", z, false);
        }
        // q = +-1 exactly: window = +-template (p = +-S_TT, sw = +-sT, dI = dT a perfect square 2^2k N^2 ... by sw = 0)
        for (int k = 0; k <= 12; k += 2) {
            In v; v.nd = (double)(s * s); v.sw = 0; v.sT = 0.0; v.sii = (u32)(1u << k); v.p = (int)v.sii;
            const double dI = v.nd * (double)v.sii;
            v.rT = 1.0 / std::sqrt(dI);
            if (dI > v.nd) { check_b("b/exact one", v, false); v.p = -v.p; check_b("b/exact minus one", v, false); }
        }
        // perfect matches with texture: p = sii, sw = sT, rT = 1 / sqrt(dI)
        for (int rep = 0; rep < 2000; ++rep) {
            In v = physical(s);
            const double dI = v.nd * (double)v.sii - (double)v.sw * (double)v.sw;
            v.p = (int)v.sii; v.sT = (double)v.sw; v.rT = 1.0 / std::sqrt(dI);
            check_b("b/perfect", v, false);
            v.p = -v.p; v.sT = -v.sT;                                   // (template = -window: q = -1)
            check_b("b/inverted", v, false);
        }
        // dI = 0 and dI <= N / 2: sw^2 = N sii - d.  Dark windows (sw near -128 N) make the low-variance rule false, others true.
        const long long n = (long long)s * s;
        int found_true = 0, found_false = 0, zeros = 0;
        for (long long e = 0; e < 200000 && (found_true < 50 || found_false < 50 || zeros < 50); ++e) {
            for (int dark = 0; dark < 2; ++dark) {
                const long long sw = dark ? -128 * n + e : e;
                if (sw < -128 * n || sw > 128 * n) continue;
                const u64 sw2 = (u64)(sw * sw);
                const u64 sii = (sw2 + (u64)n - 1) / (u64)n;
                if (sii > (u64)n * 16384ull) continue;
                const long long d = (long long)((u64)n * sii - sw2);
                if (2 * d > n) continue;
                In v; v.nd = (double)n; v.sw = (int)sw; v.sii = (u32)sii; v.sT = (double)(rnd() % 1000) - 500.0; v.p = (int)(rnd() % 2001) - 1000;
                v.rT = 1.0 / std::sqrt(1.0 + (double)(rnd() % 100000000ull));
                const double s2 = (double)sii + 256.0 * (double)sw + 16384.0 * (double)n;
                const bool lowvar = (double)d * 8388608.0 <= 10.0 * (double)n * s2;
                if (d == 0) { if (zeros++ < 50) check_b("b/dI zero", v, false); }
                else if (lowvar) { if (found_true++ < 50) check_b("b/lowvar true", v, false); }
                else { if (found_false++ < 50) check_b("b/lowvar false", v, false); }
            }
        }
        std::printf("(b) side %3d: dI = 0: %d, dI <= N/2 with the rule true: %d, false: %d\n", s, zeros, found_true, found_false);
        // (side 2: N sii - sw^2 is 0 or 3 mod 4, never 1 or 2 - only dI = 0 exists there)
        if (zeros == 0 || (s > 2 && (found_true == 0 || found_false == 0))) { ++g_viol; std::printf("VIOLATION b/coverage at side %d\n", s); }
    }
    std::printf("(b) %llu constructed inputs, %llu by the specification's route, %llu with inf / NaN in the short route\n", g_b, g_b_spec, g_b_nan);
    std::printf("(b) %llu of them with q' = NaN and dI > N / 2\n", g_b_nan_q);
    if (g_b_nan == 0 || g_b_nan_q == 0 || g_b_spec == 0 || g_b_spec == g_b) { ++g_viol; std::printf("VIOLATION b/coverage\n"); }
}

static void part_c()
{
    const double nd = 255.0 * 255.0;
    const long long N = 255 * 255;
    u64 n = 0;
    auto one = [&](long long sw, long long sii, long long p, long long sT) {
        const double swd = (double)sw, siid = (double)sii, pd = (double)p, sTd = (double)sT;
        const double a = nd * siid - swd * swd, b = __builtin_fma(-swd, swd, nd * siid);
        const double c = nd * pd - swd * sTd, d = __builtin_fma(-swd, sTd, nd * pd);
        ++n;
        if (a != b || c != d || a != (double)(N * sii - sw * sw) || c != (double)(N * p - sw * sT)) {
            if (++g_viol <= 20) std::printf("VIOLATION c: sw=%lld sii=%lld p=%lld sT=%lld\n", sw, sii, p, sT);
        }
    };
    const long long swx[] = {128 * N, 128 * N - 1, 128 * N - 255, -128 * N, -128 * N + 1, 127 * N, -127 * N - 3, 1, 0, -1};
    const long long six[] = {16384 * N, 16384 * N - 1, 16384 * N - 65025, 16129 * N, 1, 0};
    const long long px[] = {16384 * N, -16384 * N, 16384 * N - 1, -16384 * N + 1, 16256 * N, -16256 * N + 7, 1, 0};
    for (long long sw : swx) for (long long si : six) for (long long p : px) for (long long sT : swx) one(sw, si, p, sT);
    for (int i = 0; i < 1000000; ++i)
        one((long long)(rnd() % (u64)(256 * N + 1)) - 128 * N, 16384 * N - (long long)(rnd() % 100000), (rnd() & 1 ? 1 : -1) * (16384 * N - (long long)(rnd() % 100000)),
            (long long)(rnd() % (u64)(256 * N + 1)) - 128 * N);
    std::printf("(c) %llu fma / mul-sub comparisons at side 255\n", n);
}

int main(int argc, char **argv)
{
    const u64 per_side = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 2000000ull;   // x 5 sides = 10^7 per seed
    part_a("exact", SeedExact(), per_side);
    part_a("float32", SeedF32(), per_side);
    part_a("2^-20", SeedPert(), per_side);
    part_b();
    part_c();
    std::printf("%llu violations\n", g_viol);
    return g_viol ? 1 : 0;
}
