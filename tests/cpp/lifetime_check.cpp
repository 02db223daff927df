// Lifetimes of the PM core's host pieces (sea_ice_drift_amd/csrc/pm_host.h), a program of its own: compiled by
// tests/test_schedule_host.py with g++ -fsanitize=address,undefined and run on the CPU.  ScopedBuf against a stub allocator that
// counts what lives (the sanitizer sees a double free, a leak or a use after free; the counts see a block freed by the wrong
// owner), and the arena layout of sid_pm_set_points: measured size = last pointer + its region, every region 256-byte aligned.
// One line per violation, then "<n> violations".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../sea_ice_drift_amd/csrc/pm_host.h"

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++bad; if (bad < 40) { printf(__VA_ARGS__); printf("  [%s]\n", #cond); } } } while (0)

static std::set<void *> live;
static int refuse_next = 0;
struct Stub {
    static int alloc(void **p, size_t bytes)
    {
        if (refuse_next) { --refuse_next; return -3; }
        *p = malloc(bytes);
        memset(*p, 0xa5, bytes);
        live.insert(*p);
        return 0;
    }
    static void free(void *p)
    {
        CHECK(live.erase(p) == 1, "free of a block that is not live");
        ::free(p);
    }
};
typedef ScopedBuf<double, Stub> Buf;

static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "one owner per allocation");
static_assert(std::is_nothrow_move_constructible<Buf>::value && std::is_nothrow_move_assignable<Buf>::value, "move-only");

static int early_return(int fail_at)
{
    Buf a, b, c;                                                      // (an entry point: every way out frees what it got)
    refuse_next = 0;
    if (int rc = a.reserve(10)) return rc;
    if (fail_at == 1) refuse_next = 1;
    if (int rc = b.reserve(20)) return rc;
    if (fail_at == 2) refuse_next = 1;
    if (int rc = c.reserve(30)) return rc;
    a.p[9] = b.p[19] = c.p[29] = 1.0;
    return 0;
}

struct Handle { Buf own[2][2], out; };                               // (members, arrays of them: freed by `delete`)

int main()
{
    {
        Buf a;
        CHECK(a.p == nullptr && a.cap == 0, "a fresh buffer holds something");
        CHECK(a.reserve(0) == 0 && live.empty(), "reserve(0) of an empty buffer allocates");
        CHECK(a.reserve(100) == 0 && a.p && a.cap == 100 && live.size() == 1, "reserve(100)");
        a.p[99] = 1.0;
        double *const first = a.p;
        CHECK(a.reserve(50) == 0 && a.p == first && a.cap == 100, "a smaller request moved the block");
        CHECK(a.reserve(200) == 0 && a.cap == 200 && live.size() == 1, "growing kept the old block");
        a.p[199] = 2.0;
        Buf b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.cap == 200 && live.size() == 1, "move construction");
        b.p[199] = 3.0;
        Buf c;
        CHECK(c.reserve(7) == 0 && live.size() == 2, "second buffer");
        c = std::move(b);
        CHECK(b.p == nullptr && c.cap == 200 && live.size() == 1, "move assignment frees what the target held");
        Buf &self = c;
        c = std::move(self);
        CHECK(c.p && c.cap == 200 && live.size() == 1, "self move");
        refuse_next = 1;
        CHECK(c.reserve(400) == -3 && c.p == nullptr && c.cap == 0 && live.empty(), "a refused growth: error code, nothing held");
        CHECK(c.reserve(4) == 0 && live.size() == 1, "reserve after a refusal");
        c.release();
        CHECK(c.p == nullptr && c.cap == 0 && live.empty(), "release");
        c.release();
        CHECK(a.reserve(3) == 0 && live.size() == 1, "a moved-from buffer is an empty one");
    }
    CHECK(live.empty(), "%zu blocks outlive their scope", live.size());
    for (int fail_at = 0; fail_at < 3; ++fail_at) {
        CHECK(early_return(fail_at) == (fail_at ? -3 : 0), "early return %d", fail_at);
        CHECK(live.empty(), "early return %d leaves %zu blocks", fail_at, live.size());
    }
    {
        Handle *h = new Handle();
        CHECK(h->own[1][0].reserve(5) == 0 && h->own[0][1].reserve(6) == 0 && h->out.reserve(7) == 0 && live.size() == 3, "members");
        std::vector<Buf> v(3);
        CHECK(v[1].reserve(9) == 0, "vector element");
        v.resize(40);                                                 // (reallocation moves the elements)
        CHECK(v[1].cap == 9 && live.size() == 4, "elements moved by the vector");
        delete h;
        CHECK(live.size() == 1, "delete of the handle leaves %zu blocks", live.size());
    }
    CHECK(live.empty(), "%zu blocks outlive the vector", live.size());

    // the arena of sid_pm_set_points: point counts, angle counts, with and without the two sampling tables
    const size_t ns[] = {0, 1, 6, 31, 32, 33, 1000, 40000}, Ks[] = {1, 3, 7, 15, 16, 64}, samps[] = {0, 34 * 36, 15 * 34 * 36, 64 * 64 * 64};
    for (size_t n : ns) for (size_t K : Ks) for (size_t n_samp : samps) for (size_t n_samp2 : {(size_t)0, K * 1500}) {
        Carver measure;
        point_arena(measure, n, K, n_samp, n_samp2);
        std::vector<unsigned char> block(measure.off + 256);
        unsigned char *base = block.data() + (256 - (size_t)block.data() % 256) % 256;     // (as hipMalloc hands out: 256-aligned)
        Carver c(base);
        const PointArena a = point_arena(c, n, K, n_samp, n_samp2);
        CHECK(c.off == measure.off, "n %zu K %zu: measured %zu, carved %zu", n, K, measure.off, c.off);
        struct Region { const char *name; const void *p; size_t bytes; bool present; };
        const Region R[6] = {{"vec", a.vec, 5 * n * sizeof(double), n > 0}, {"angles", a.angles, K * sizeof(double), true}, {"rot", a.rot, 4 * K * sizeof(double), true},
                             {"order", a.order, n * sizeof(int32_t), n > 0}, {"samp", a.samp, (n_samp + 4) * sizeof(uint16_t), true}, {"samp2", a.samp2, n_samp2 * sizeof(uint32_t), n_samp2 > 0}};
        const unsigned char *expect = base;
        for (const Region &r : R) {
            CHECK((r.p != nullptr) == r.present, "n %zu K %zu samp %zu samp2 %zu: region %s present %d", n, K, n_samp, n_samp2, r.name, (int)(r.p != nullptr));
            if (!r.p) continue;
            const unsigned char *p = static_cast<const unsigned char *>(r.p);
            CHECK((size_t)p % 256 == 0, "n %zu K %zu: region %s is not 256-byte aligned", n, K, r.name);
            CHECK(p == expect, "n %zu K %zu: region %s at %td, expected %td (in order, 256 bytes apart at the least, no gap of more)", n, K, r.name, p - base, expect - base);
            expect = p + (r.bytes + 255) / 256 * 256;
            memset(const_cast<unsigned char *>(p), 0x5a, r.bytes);     // (inside the block: the sanitizer watches)
        }
        CHECK(expect == base + measure.off, "n %zu K %zu: the last region ends at %td, measured %zu", n, K, expect - base, measure.off);
        // the offsets the entry point computed by hand before it used carve.h
        auto up256 = [](size_t v) { return (v + 255) / 256 * 256; };
        const size_t o_ang = up256(8 * 5 * n), o_rot = up256(o_ang + 8 * K), o_ord = up256(o_rot + 8 * 4 * K), o_smp = up256(o_ord + 4 * n),
                     o_smp2 = up256(o_smp + 2 * (n_samp + 4)), total = up256(o_smp2 + 4 * n_samp2);
        CHECK(total == measure.off, "n %zu K %zu: %zu bytes, the offset chain gave %zu", n, K, measure.off, total);
        CHECK((const unsigned char *)a.angles == base + o_ang && (const unsigned char *)a.rot == base + o_rot && (const unsigned char *)a.samp == base + o_smp, "n %zu K %zu: offsets moved", n, K);
        if (n) CHECK((const unsigned char *)a.order == base + o_ord, "n %zu K %zu: order moved", n, K);
        if (n_samp2) CHECK((const unsigned char *)a.samp2 == base + o_smp2, "n %zu K %zu: samp2 moved", n, K);
    }
    printf("%d violations\n", bad);
    return bad ? 1 : 0;
}
