// Host check of csrc/carve.h: a staging layout is one function of a Carver&, run once to measure and once to carve; the two runs
// must agree.  Layouts of 0..12 regions; element counts 0, 1, 255, 256, 257 and one that makes the region about 2^33 bytes;
// elements of 1, 4, 8 and 48 bytes; every subset of the regions absent.  No memory is touched: the block is an address only.
// Prints "<n> layouts, <v> violations"; exit status 1 on a violation.
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../sea_ice_drift_amd/csrc/carve.h"

namespace {

struct E48 { unsigned char b[48]; };
constexpr size_t kElem[4] = {1, 4, 8, 48};
constexpr int kMaxRegions = 12, kCounts = 6;

struct Region { int type; size_t n; bool present; };

size_t count_of(int which, size_t elem)
{
    const size_t c[kCounts] = {0, 1, 255, 256, 257, ((size_t)1 << 33) / elem + 1};
    return c[which];
}

// The layout under test: the regions in order, each through take<T>
void layout(Carver &c, const std::vector<Region> &rs, std::vector<unsigned char *> &out)
{
    out.clear();
    for (const Region &r : rs) {
        unsigned char *p = nullptr;
        switch (r.type) {
        case 0: p = reinterpret_cast<unsigned char *>(c.take<uint8_t>(r.n, r.present)); break;
        case 1: p = reinterpret_cast<unsigned char *>(c.take<uint32_t>(r.n, r.present)); break;
        case 2: p = reinterpret_cast<unsigned char *>(c.take<double>(r.n, r.present)); break;
        default: p = reinterpret_cast<unsigned char *>(c.take<E48>(r.n, r.present)); break;
        }
        out.push_back(p);
    }
}

long long violations = 0;
void violation(const char *what, int regions, unsigned absent, int shift)
{
    if (++violations <= 20) printf("violation: %s (regions = %d, absent mask = 0x%x, shift = %d)\n", what, regions, absent, shift);
}

}  // namespace

int main()
{
    static_assert(sizeof(E48) == 48, "48-byte element");
    unsigned char *const base = reinterpret_cast<unsigned char *>((uintptr_t)1 << 20);
    long long layouts = 0;
    std::vector<Region> rs;
    std::vector<unsigned char *> none, first, second;
    for (int regions = 0; regions <= kMaxRegions; ++regions)
        for (int shift = 0; shift < kCounts * 4; ++shift)                  // which count and element size region 0 starts with
            for (unsigned absent = 0; absent < (1u << regions); ++absent) {
                rs.clear();
                size_t want = 0;                                           // the sum written out by hand: what the block must hold
                for (int i = 0; i < regions; ++i) {
                    Region r;
                    r.type = (i + shift / kCounts) % 4;
                    r.n = count_of((i + shift) % kCounts, kElem[r.type]);
                    r.present = !((absent >> i) & 1u);
                    if (r.present && r.n) want += (r.n * kElem[r.type] + 255) / 256 * 256;
                    rs.push_back(r);
                }
                ++layouts;
                Carver measure;
                layout(measure, rs, none);
                Carver c1(base), c2(base);
                layout(c1, rs, first);
                layout(c2, rs, second);
                if (measure.off != want) violation("measured size is not the sum of the present regions", regions, absent, shift);
                if (c1.off != measure.off) violation("carving ends elsewhere than measuring", regions, absent, shift);
                if (first != second) violation("a second run gives other pointers", regions, absent, shift);
                size_t end = 0;                                            // end of the last present region
                for (int i = 0; i < regions; ++i) {
                    const Region &r = rs[(size_t)i];
                    if (none[(size_t)i]) violation("measuring hands out a pointer", regions, absent, shift);
                    if (!r.present || r.n == 0) {
                        if (first[(size_t)i]) violation("an absent region has a pointer", regions, absent, shift);
                        continue;
                    }
                    if (!first[(size_t)i]) { violation("a present region has none", regions, absent, shift); continue; }
                    const size_t at = (size_t)(first[(size_t)i] - base);
                    if (at % 256) violation("a region is not 256-byte aligned", regions, absent, shift);
                    if (at < end) violation("regions overlap or are out of order", regions, absent, shift);
                    end = at + r.n * kElem[r.type];
                }
                if (end > c1.off) violation("the last region ends behind the block", regions, absent, shift);
            }
    printf("%lld layouts, %lld violations\n", layouts, violations);
    return violations ? 1 : 0;
}
