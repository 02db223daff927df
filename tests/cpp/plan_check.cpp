// Host-side invariants of the PM launch planner (sea_ice_drift_amd/csrc/pm_plan.h plan_points): compiled and run by
// tests/test_plan_host.py with g++ alone.  No argument: the matrix of template sides x angle counts x flags x switch sets on a
// 400 x 400 image 2, one line per violated invariant, then "<n> violations".  `grid FILE s K`: the launch table (count lds band
// pitch occ) of the points in FILE (n, then c1 r1 c2fg r2fg border per point) on a 10000 x 10000 pair, default switches.
// `instances`: the table of kernel instantiations (pm_instances.h) against the written-out predicate, over the whole domain.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <map>
#define __host__
#define __device__
#include "../../sea_ice_drift_amd/csrc/pm_plan.h"

// What the planner asks about the kernels' instantiations it reads from the table the library ships (pm_instances.h).  The
// predicate that used to stand in for that table here is its SPECIFICATION now: written out, and compared with the table over
// the whole domain (`instances`; the pitches the kernels carry and four they do not).
static bool rp_pitch_spec(int band, int paired, int pitch, int occ)
{
    if (occ == 4) return band == 4 && (pitch == 104 || pitch == 112) && (paired == 1 || paired == 2);
    const bool common = pitch == 136 || pitch == 168 || pitch == 0;
    if (paired == 0 && band == 8) return common;
    return common || pitch == 104 || pitch == 112 || pitch == 1104;
}

using namespace sid;
using namespace sid::plan;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++bad; if (bad < 60) { printf(__VA_ARGS__); printf("  [%s]\n", #cond); } } } while (0)

struct Points { std::vector<double> c1, r1, c2, r2, b; };
static void add(Points &P, double c2, double r2, double b) { P.c1.push_back(c2); P.r1.push_back(r2); P.c2.push_back(c2); P.r2.push_back(r2); P.b.push_back(b); }

static PlanInput input_of(const Points &P, int s, int K, uint32_t flags, const Switches &sw, int64_t rows, int64_t cols)
{
    PlanInput in;
    in.n = (int64_t)P.b.size();
    in.c1 = P.c1.data(); in.r1 = P.r1.data(); in.c2fg = P.c2.data(); in.r2fg = P.r2.data(); in.border = P.b.data();
    in.s = s; in.K = K; in.flags = flags;
    in.rows1 = rows; in.cols1 = cols; in.rows2 = rows; in.cols2 = cols;
    in.rp = use_rp(sw, s); in.rpp = in.rp ? rp_paired(sw, K) : 0;
    return in;
}

static void check_plan(const char *tag, const PlanInput &in, const Switches &sw)
{
    Plan pl;
    std::string err;
    const int rc = plan_points(in, sw, pl, err);
    CHECK(rc == 0, "%s: plan_points failed: %s", tag, err.c_str());
    if (rc) return;
    const int64_t n = in.n;
    const int s = in.s, K = in.K;
    const bool rp = in.rp, small_ok = mfma_img_size_supported(s), b8 = band8_ok(sw, rp, in.rpp, s, K);
    const bool keep_si = rp && !sw.no_gsi, policy = keep_acc_policy(sw, rp, in.rpp, K);
    // ---- coverage: order, large_idx and nan_idx are disjoint and together 0 .. n-1
    std::vector<int> where((size_t)n, 0), pos_of((size_t)n, -1);      // 1 order, 2 large, 3 nan
    auto put = [&](const std::vector<int32_t> &v, int w) {
        for (size_t p = 0; p < v.size(); ++p) {
            const int32_t i = v[p];
            CHECK(i >= 0 && i < n, "%s: index %d out of range", tag, (int)i);
            if (i < 0 || i >= n) continue;
            CHECK(where[(size_t)i] == 0, "%s: point %d listed twice", tag, (int)i);
            where[(size_t)i] = w;
            if (w == 1) pos_of[(size_t)i] = (int)p;
        }
    };
    put(pl.order, 1); put(pl.large_idx, 2); put(pl.nan_idx, 3);
    std::vector<int32_t> est((size_t)n, 0);
    estimate_points(sw, in.border, n, s, K, in.flags, nullptr, est.data());
    CHECK(pl.info[0] == (double)pl.buckets.size(), "%s: info[0]", tag);
    // ---- buckets tile `order`
    std::vector<int> bucket_of(pl.order.size(), -1);
    size_t at = 0;
    for (size_t k = 0; k < pl.buckets.size(); ++k) {
        const Bucket &b = pl.buckets[k];
        CHECK((size_t)b.offset == at && b.count > 0, "%s: bucket %zu offset %d count %d, expected offset %zu", tag, k, b.offset, b.count, at);
        for (int p = 0; p < b.count && at + p < bucket_of.size(); ++p) bucket_of[at + (size_t)p] = (int)k;
        at += (size_t)std::max(b.count, 0);
    }
    CHECK(at == pl.order.size(), "%s: the buckets hold %zu positions, order %zu", tag, at, pl.order.size());
    if (at != pl.order.size()) return;
    if (rp) CHECK(pl.goff.size() == pl.order.size() && pl.recs.size() == pl.order.size(), "%s: goff / recs sizes", tag);
    else CHECK(pl.goff.empty() && pl.gsii_granules == 0 && pl.pool_stride == 0, "%s: blocks without the row-pair kernel", tag);
    // ---- per point
    struct Key { int cls; double work; bool operator<(const Key &o) const { return cls != o.cls ? cls < o.cls : work > o.work; } };
    std::vector<std::map<Key, std::vector<int32_t>>> runs(pl.buckets.size());
    uint64_t gsum = 0;
    std::vector<uint32_t> gran((size_t)n, 0u);
    for (int64_t i = 0; i < n; ++i) {
        int wh = 0, ww = 0;
        bool clipped = false;
        const bool valid = window_dims(in.c2fg[i], in.r2fg[i], in.border[i], s, in.rows2, in.cols2, wh, ww, &clipped);
        const int w = where[(size_t)i];
        CHECK(w != 0, "%s: point %d in no list", tag, (int)i);
        if (!valid) { CHECK(w == (small_ok ? 1 : 3), "%s: point %d without a window is in list %d", tag, (int)i, w); }
        else CHECK(w != 3, "%s: valid point %d among the NaN points", tag, (int)i);
        if (valid && (clipped || !small_ok || sw.all_large)) CHECK(w == 2, "%s: point %d (clipped %d) not in large_idx", tag, (int)i, (int)clipped);
        ShapeClass sc{false, 4, 1, 0, 0};
        if (valid && !clipped && small_ok) {
            sc = shape_class(sw, rp, in.rpp, wh, ww, s, K, in.flags, b8, sw.no_fixed_pitch);
            CHECK((w == 2) == (sc.lds > max_lds_bytes() || sw.all_large), "%s: point %d border %g needs %d B of LDS, list %d", tag, (int)i, in.border[i], sc.lds, w);
            // agreement with the cost model (unclipped windows inside image 2)
            const int e = est[(size_t)i];
            CHECK(((e & SID_PM_CLASS_LARGE) != 0) == (w == 2 && !sw.all_large) || sw.all_large, "%s: border %g estimate %d, LARGE bit against list %d", tag, in.border[i], e, w);
        }
        if (w != 1) continue;
        const int p = pos_of[(size_t)i];
        const Bucket &b = pl.buckets[(size_t)bucket_of[(size_t)p]];
        const bool gs = rp && (b.big || rp_pitch_is_gs(b.pitch));
        if (rp) CHECK(pl.recs[(size_t)p].pt == (int32_t)i && pl.recs[(size_t)p].gsii_off == pl.goff[(size_t)p] && (pl.recs[(size_t)p].border == in.border[i] || !valid), "%s: record of position %d", tag, p);
        if (!valid) { runs[(size_t)bucket_of[(size_t)p]][Key{99, 0.0}].push_back((int32_t)i); continue; }
        runs[(size_t)bucket_of[(size_t)p]][Key{sc.cls, (double)(wh - s + 1) * (double)(ww - s + 1)}].push_back((int32_t)i);
        // footprint and instantiation
        const int need = b.big ? big_layout(wh, ww, s, K, in.flags).total : lds_need(sw, rp, in.rpp, wh, ww, s, K, in.flags, b.band, b.pitch, gs);
        CHECK(need <= b.lds && b.lds <= max_lds_bytes(), "%s: border %g needs %d B, its launch has %d", tag, in.border[i], need, b.lds);
        CHECK(sc.big == b.big && sc.band == b.band, "%s: border %g big %d band %d in a launch of big %d band %d", tag, in.border[i], (int)sc.big, sc.band, (int)b.big, b.band);
        const LaunchShape ls = launch_shape(b, rp);
        CHECK(ls.per_cu >= std::max(1, sc.cls) || (b.occ == 3 && sc.cls == 4), "%s: border %g class %d in a launch of %d per CU", tag, in.border[i], sc.cls, ls.per_cu);
        if (sc.cls == 4) CHECK(blocks_per_cu(b.lds) >= 4 && (b.occ == 4 || rp_pitch_is_w3(b.pitch)), "%s: border %g class 4, launch lds %d occ %d pitch %d", tag, in.border[i], b.lds, b.occ, b.pitch);
        if (rp && in.rpp == 0) CHECK(rp_pitch_is_w3(b.pitch) == (sc.cls == 4), "%s: border %g class %d pitch %d", tag, in.border[i], sc.cls, b.pitch);
        // blocks
        const uint32_t blk = !gs ? 0u : b.big ? (uint32_t)(big_layout(wh, ww, s, K, in.flags).big_bytes / 4) : block_entries(in.rpp, s, keep_si, wh, ww, b.band, b.keep);
        if (gs) CHECK(b.gs_stride >= blk, "%s: border %g block %u, gs_stride %u", tag, in.border[i], blk, b.gs_stride);
        if (b.pooled) CHECK(pl.pool_stride >= blk, "%s: border %g block %u, pool_stride %u", tag, in.border[i], blk, pl.pool_stride);
        gran[(size_t)i] = (b.pooled || !gs) ? 0u : blk / 64u;
        // cost model: the low four bits and the GS / BIG bits
        const int e = est[(size_t)i];
        CHECK((e & SID_PM_CLASS_PER_CU) == ls.per_cu, "%s: border %g estimate %d per CU, launch %d", tag, in.border[i], e & SID_PM_CLASS_PER_CU, ls.per_cu);
        CHECK(((e & SID_PM_CLASS_GS) != 0) == gs && ((e & SID_PM_CLASS_BIG) != 0) == b.big, "%s: border %g estimate %d, launch gs %d big %d", tag, in.border[i], e, (int)gs, (int)b.big);
    }
    // ---- per bucket
    for (size_t k = 0; k < pl.buckets.size(); ++k) {
        const Bucket &b = pl.buckets[k];
        const bool gs = rp && (b.big || rp_pitch_is_gs(b.pitch));
        if (b.pitch) CHECK(rp && rp_pitch_instantiated(b.band, in.rpp, b.pitch, b.occ == 4 ? 4 : 3), "%s: bucket %zu pitch %d band %d occ %d not instantiated", tag, k, b.pitch, b.band, b.occ);
        CHECK(b.occ == 3 || (b.occ == 4 && rp && rp_pitch_instantiated(b.band, in.rpp, b.pitch, 4)), "%s: bucket %zu occ %d", tag, k, b.occ);
        CHECK(b.band == 4 || (b.band == 8 && b8), "%s: bucket %zu band %d", tag, k, b.band);
        if (b.big) CHECK(rp && b.pitch == 0 && b.band == 4 && b.occ == 3 && !b.keep && !b.pooled, "%s: bucket %zu big", tag, k);
        if (b.keep) CHECK(policy && gs && !b.big, "%s: bucket %zu keeps accumulators", tag, k);
        const bool only_nan = runs[k].size() == 1 && runs[k].begin()->first.cls == 99;
        if (!only_nan) CHECK(b.pooled == (gs && !b.big && !sw.no_recycle && (b.keep || sw.recycle_all)), "%s: bucket %zu pooled %d", tag, k, (int)b.pooled);
        if (!gs) CHECK(b.gs_stride == 0, "%s: bucket %zu gs_stride without gs", tag, k);
        // XCD order: the runs of equal class and work in their place (long work first), each interleaved from 32 points on
        size_t p = (size_t)b.offset;
        for (const auto &kv : runs[k]) {
            const std::vector<int32_t> &src = kv.second;              // (ascending: filled in the caller's order)
            const int64_t L = (int64_t)src.size(), m = (L + 7) / 8;
            std::vector<int32_t> want;
            if (!sw.no_xcd_order && L >= 32) { for (int64_t q = 0; q < m; ++q) for (int64_t c = 0; c < 8; ++c) if (c * m + q < L) want.push_back(src[(size_t)(c * m + q)]); }
            else want = src;
            bool same = true;
            for (size_t q = 0; q < want.size(); ++q) same = same && pl.order[p + q] == want[q];
            CHECK(same, "%s: bucket %zu run of %lld points (class %d work %g) not in the expected order", tag, k, (long long)L, kv.first.cls, kv.first.work);
            p += want.size();
        }
    }
    // ---- block offsets
    for (size_t p = 0; p < pl.goff.size(); ++p) {
        CHECK(pl.goff[p] == (uint32_t)gsum, "%s: goff[%zu] = %u, expected %llu", tag, p, pl.goff[p], (unsigned long long)gsum);
        gsum += gran[(size_t)pl.order[p]];
    }
    CHECK(gsum == pl.gsii_granules, "%s: gsii_granules %llu, expected %llu", tag, (unsigned long long)pl.gsii_granules, (unsigned long long)gsum);
}

struct Set { const char *name; Switches sw; };
static std::vector<Set> switch_sets()
{
    std::vector<Set> v;
    auto add_set = [&](const char *name, void (*f)(Switches &)) { Set s{name, Switches()}; f(s.sw); v.push_back(s); };
    add_set("default", [](Switches &) {});
    add_set("NO_W3", [](Switches &w) { w.no_w3 = true; });
    add_set("NO_OCC4", [](Switches &w) { w.no_occ4 = true; });
    add_set("ALWAYS_GS", [](Switches &w) { w.always_gs = true; });
    add_set("NO_GS", [](Switches &w) { w.no_gs = true; });
    add_set("NO_GSI", [](Switches &w) { w.no_gsi = true; });
    add_set("NO_RP", [](Switches &w) { w.no_rp = true; });
    add_set("ALL_LARGE", [](Switches &w) { w.all_large = true; });
    add_set("NO_RECYCLE", [](Switches &w) { w.no_recycle = true; });
    add_set("RECYCLE_ALL=0", [](Switches &w) { w.recycle_all = false; });
    add_set("KEEP_ACC=0", [](Switches &w) { w.keep_acc = 0; });
    add_set("KEEP_ACC=1", [](Switches &w) { w.keep_acc = 1; });
    add_set("NO_BAND8", [](Switches &w) { w.no_band8 = true; });
    add_set("NO_FIXED_PITCH", [](Switches &w) { w.no_fixed_pitch = true; });
    add_set("NO_XCD_ORDER", [](Switches &w) { w.no_xcd_order = true; });
    add_set("NO_PAIRED", [](Switches &w) { w.no_paired = true; });
    add_set("NO_QUAD", [](Switches &w) { w.no_quad = true; });
    add_set("NO_BIG", [](Switches &w) { w.no_big = true; });
    return v;
}

// the table against the written-out predicate; prints "<n> instance checks, <m> violations"
static int check_instances()
{
    int checks = 0;
    for (int band : {4, 8})
        for (int paired : {0, 1, 2})
            for (int occ : {3, 4})
                for (int pitch : {0, 104, 112, 136, 168, 1104, 96, 120, 1112, 2104}) {
                    CHECK(sid::rp_pitch_instantiated(band, paired, pitch, occ) == rp_pitch_spec(band, paired, pitch, occ),
                          "band %d paired %d pitch %d occ %d: the table says %d", band, paired, pitch, occ, (int)sid::rp_pitch_instantiated(band, paired, pitch, occ));
                    ++checks;
                }
    // both sides carry the same rows (rp_pitch_instantiated asks side 34), and the default register budget is three per SIMD
    for (int band : {4, 8})
        for (int paired : {0, 1, 2})
            for (int occ : {3, 4})
                for (int pitch : {0, 104, 112, 136, 168, 1104, 96, 120, 1112, 2104})
                    for (bool big : {false, true}) {
                        CHECK(sid::rp_instantiated(34, band, paired, pitch, occ, big) == sid::rp_instantiated(35, band, paired, pitch, occ, big),
                              "band %d paired %d pitch %d occ %d big %d: sides 34 and 35 differ", band, paired, pitch, occ, (int)big);
                        ++checks;
                    }
    CHECK(sid::rp_pitch_instantiated(4, 1, 104) == sid::rp_pitch_instantiated(4, 1, 104, 3) && sid::rp_pitch_instantiated(8, 0, 104) == sid::rp_pitch_instantiated(8, 0, 104, 3), "default occ");
    // the other three answers, written out
    for (int s = -1; s <= 70; ++s) {
        CHECK(sid::mfma_img_size_supported(s) == (s >= 2 && s <= 64), "mfma_img_size_supported(%d)", s);
        CHECK(sid::mfma_band8_supported(s) == (s == 34 || s == 35), "mfma_band8_supported(%d)", s);
        CHECK(sid::mfma_side_arg(s) == ((s == 34 || s == 35) ? s : 0), "mfma_side_arg(%d)", s);
        checks += 3;
    }
    CHECK(sid::max_lds_bytes() == 160 * 1024, "max_lds_bytes");
    checks += 2;
    printf("%d instance checks, %d violations\n", checks, bad);
    return bad > 125 ? 125 : bad;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "instances")) return check_instances();
    if (argc == 5 && !strcmp(argv[1], "grid")) {
        FILE *f = fopen(argv[2], "r");
        if (!f) return 2;
        long long n = 0;
        if (fscanf(f, "%lld", &n) != 1) return 2;
        Points P;
        for (long long i = 0; i < n; ++i) {
            double v[5];
            if (fscanf(f, "%lf %lf %lf %lf %lf", v, v + 1, v + 2, v + 3, v + 4) != 5) return 2;
            P.c1.push_back(v[0]); P.r1.push_back(v[1]); P.c2.push_back(v[2]); P.r2.push_back(v[3]); P.b.push_back(v[4]);
        }
        fclose(f);
        const Switches sw;
        Plan pl;
        std::string err;
        if (plan_points(input_of(P, atoi(argv[3]), atoi(argv[4]), SID_PM_HES_NORM, sw, 10000, 10000), sw, pl, err)) { printf("%s\n", err.c_str()); return 2; }
        for (const Bucket &b : pl.buckets) printf("%d %d %d %d %d\n", b.count, b.lds, b.band, b.pitch, b.occ);
        return 0;
    }
    Points P;
    for (int b = 2; b <= 112; ++b) add(P, 200, 200, b);
    add(P, 200, 200, 120);
    for (int k = 0; k < 33; ++k) add(P, 200, 200, 20);               // runs of 33 + 1, 32 + 1 and 31 + 1 - 1 points of equal border:
    for (int k = 0; k < 31; ++k) add(P, 200, 200, 21);               // border 20: 34 points, border 21: 32, border 22: 31
    for (int k = 0; k < 30; ++k) add(P, 200, 200, 22);
    for (int k = 0; k < 32; ++k) add(P, 200, 200, 30);               // ... and 33 of border 30
    add(P, 200, 200, NAN); add(P, 200, 200, -3.0);
    add(P, 380, 200, 25); add(P, 200, 385, 30); add(P, 392, 392, 20);   // clipped by the right / bottom edge / both
    add(P, 10, 200, 25); add(P, 200, 5, 20); add(P, -50, -50, 20); add(P, 500, 200, 20);   // starting outside the image
    const int sides[4] = {34, 35, 20, 70}, angle_counts[4] = {kQuadMaxAngles, kPairedMaxAngles, kRpGroup, kRpGroup + 1};
    int plans = 0;
    for (const Set &set : switch_sets())
        for (int s : sides)
            for (int K : angle_counts)
                for (uint32_t flags : {SID_PM_HES_NORM, SID_PM_HES_NORM | SID_PM_HES_SMTH}) {
                    char tag[96];
                    snprintf(tag, sizeof tag, "%s s=%d K=%d flags=%u", set.name, s, K, flags);
                    check_plan(tag, input_of(P, s, K, flags, set.sw, 400, 400), set.sw);
                    for (int n : {0, 1}) {                               // point counts 0 and 1
                        Points Q;
                        if (n) add(Q, 200, 200, 20);
                        char t2[112];
                        snprintf(t2, sizeof t2, "%s n=%d", tag, n);
                        check_plan(t2, input_of(Q, s, K, flags, set.sw, 400, 400), set.sw);
                    }
                    plans += 3;
                }
    printf("%d plans, %d violations\n", plans, bad);
    return bad > 125 ? 125 : bad;
}
