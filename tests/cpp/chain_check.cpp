// Host-side checks of the chained launches (sea_ice_drift_amd/csrc/pm_kernel.h chain_shard_count, pm_plan.h chain_rule):
// compiled and run by tests/test_chain_host.py with g++ alone.  One line per violation, then "<n> violations".
#include <cstdio>
#include <cstdint>
#define __host__
#define __device__
#include "../../sea_ice_drift_amd/csrc/pm_plan.h"


using namespace sid;
using namespace sid::plan;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++bad; if (bad < 40) { printf(__VA_ARGS__); printf("  [%s]\n", #cond); } } } while (0)

int main()
{
    // the shards of a launch of n workgroups: shard j = the workgroups with (blockIdx.x & 7) == j
    for (int n = 1; n <= 4100; ++n) {
        int sum = 0, nonempty = 0;
        for (int j = 0; j < kChainShards; ++j) {
            const int c = chain_shard_count(n, j);
            int brute = 0;
            for (int i = j; i < n; i += kChainShards) ++brute;
            CHECK(c == brute, "n %d shard %d: %d, counted %d", n, j, c, brute);
            CHECK((c == 0) == (n < kChainShards && j >= n), "n %d shard %d: %d", n, j, c);
            sum += c; nonempty += c > 0 ? 1 : 0;
        }
        CHECK(sum == n, "n %d: shards sum to %d", n, sum);
        CHECK(nonempty == chain_nonempty_shards(n), "n %d: %d non-empty shards, chain_nonempty_shards says %d", n, nonempty, chain_nonempty_shards(n));
    }
    CHECK(chain_shard_count(0, 0) == 0 && chain_nonempty_shards(0) == 0, "n 0");
    static_assert(kChainShards == 8 && kChainLineWords * 4 == 128 && kChainWords == 9 * kChainLineWords, "eight shards and the shard count, a 128-byte line each");

    // the rule: more than one launch, not a short run, the switch unset, the device's support, the handle's signal memory
    const size_t launches[3] = {1, 2, 5};
    for (size_t nl : launches)
        for (int is_short = 0; is_short < 2; ++is_short)
            for (int supported = 0; supported < 2; ++supported)
                for (int memory = 0; memory < 2; ++memory)
                    for (int off = 0; off < 2; ++off) {
                        Switches sw;
                        sw.no_chain = off != 0;
                        const double rounds = is_short ? kSideRounds : kSideRounds + 0.5;
                        const bool want = nl > 1 && !is_short && supported && memory && !off;
                        const bool got = chain_rule(sw, nl, rounds, supported != 0, memory != 0);
                        CHECK(got == want, "launches %zu short %d supported %d memory %d switch %d: %d", nl, is_short, supported, memory, off, (int)got);
                        CHECK(!(got && side_by_side_rule(sw, nl, rounds)), "chained and side by side at once");
                        const ChainReason why = chain_reason(sw, nl, rounds, supported != 0, memory != 0);
                        CHECK((why == kChainYes) == got, "reason %d", (int)why);
                        if (nl > 1 && !is_short && !off && !supported) CHECK(why == kChainNoWaitValue, "reason %d", (int)why);
                        if (nl > 1 && !is_short && !off && supported && !memory) CHECK(why == kChainNoSignalMemory, "reason %d", (int)why);
                    }
    {   // the A/B switches of the side-by-side order: forced on, a long run stays side by side; forced off, a short run is chained
        Switches sw;
        sw.side_by_side = 1;
        CHECK(!chain_rule(sw, 5, 100.0, true, true), "SID_PM_SIDE_BY_SIDE=1");
        sw.side_by_side = 0;
        CHECK(chain_rule(sw, 5, 1.0, true, true), "SID_PM_SIDE_BY_SIDE=0");
        sw.no_chain = true;
        CHECK(!chain_rule(sw, 5, 1.0, true, true), "SID_PM_SIDE_BY_SIDE=0 SID_PM_NO_CHAIN=1");
        Switches first;
        first.side_first = 2;
        CHECK(!chain_rule(first, 5, 100.0, true, true), "SID_PM_SIDE_FIRST=2");
    }
    printf("%d violations\n", bad);
    return bad ? 1 : 0;
}
