// Host-side checks of the launch order of a run (sea_ice_drift_amd/csrc/pm_plan.h launch_schedule, release_upto): compiled and
// run by tests/test_schedule_host.py with g++ alone.  Every vector of 1..6 bucket counts over {0, 1, 24, 5000} x row-pair / classic
// kernel x SID_PM_SIDE_BY_SIDE unset / 0 / 1 x SID_PM_SIDE_FIRST unset / 0 / 1 / 2 / 3 / 9 x SID_PM_NO_CHAIN x stream wait-value
// support x signal memory.  One line per violation, then "<n> violations".
#include <cstdio>
#include <cstdint>
#include <cstring>
#define __host__
#define __device__
#include "../../sea_ice_drift_amd/csrc/pm_plan.h"


using namespace sid;
using namespace sid::plan;

static int bad = 0;
static char tag[200];
#define CHECK(cond, ...) do { if (!(cond)) { ++bad; if (bad < 40) { printf("%s: ", tag); printf(__VA_ARGS__); printf("  [%s]\n", #cond); } } } while (0)

// The streams as the device sees them.  Steps [0, cut) are waits + launch; step `cut` (a failure there, cut < n) has its waits
// enqueued and no launch, and the host has stored the release words 0 .. release_upto(S, cut).  A stream runs its steps in order;
// a step starts once its release word is stored; a launch that counts arrivals stores its word when it starts (its last workgroup
// has started by then at the latest - the earliest moment is the adversarial one); the side streams wait for nothing else (the
// fork event is recorded before any of them).  As many steps as possible start before any completes.  Returns false when
// something enqueued never runs; *peak = most chained launches in flight at once.
static bool simulate(const Schedule &S, const std::vector<Bucket> &B, size_t cut, int *peak)
{
    const size_t n = S.steps.size(), end = cut < n ? cut + 1 : n;
    std::vector<int> state(end, 0);                                   // 0 enqueued, 1 running, 2 done
    std::vector<bool> released(n, false);
    if (cut < n) for (int j = 0; j <= release_upto(S, cut); ++j) released[(size_t)j] = true;
    *peak = 0;
    for (;;) {
        bool started = false;
        for (size_t k = 0; k < end; ++k) {
            if (state[k] != 0) continue;
            const LaunchStep &st = S.steps[k];
            bool head = true;                                         // every earlier step of its stream is done
            for (size_t j = 0; j < k; ++j) if (S.steps[j].stream == st.stream && state[j] != 2) head = false;
            if (!head || (st.wait_release >= 0 && !released[(size_t)st.wait_release])) continue;
            if (k == cut) { state[k] = 2; started = true; continue; }   // (the waits alone: through at once)
            state[k] = 1; started = true;
            if (st.counts_arrival) released[k] = true;
            int flying = 0;
            for (size_t j = 0; j < end; ++j) flying += (state[j] == 1 && S.steps[j].stream >= 0 && B[j].count > 0) ? 1 : 0;
            *peak = std::max(*peak, flying);
        }
        if (started) continue;
        size_t oldest = end;
        for (size_t k = 0; k < end && oldest == end; ++k) if (state[k] == 1) oldest = k;
        if (oldest == end) break;
        state[oldest] = 2;
    }
    for (size_t k = 0; k < end; ++k) if (state[k] != 2) return false;
    return true;
}

static long n_short = 0, n_long = 0, n_order[3] = {0, 0, 0};

static void check(const Switches &sw, const std::vector<Bucket> &B, bool rp, bool can_wait, bool have_mem)
{
    const size_t n = B.size();
    const Schedule S = launch_schedule(sw, B, rp, can_wait, have_mem);
    // ---- structure
    CHECK(S.steps.size() == n, "%zu steps", S.steps.size());
    if (S.steps.size() != n) return;
    double rounds = 0;
    for (const Bucket &b : B) rounds += (double)b.count / (256.0 * launch_shape(b, rp).round_slots);
    CHECK(S.rounds == rounds, "rounds %.17g, counted %.17g", S.rounds, rounds);
    if (n > 1) ++(rounds <= kSideRounds ? n_short : n_long);
    const bool side = side_by_side_rule(sw, n, rounds);
    const ChainReason why = chain_reason(sw, n, rounds, can_wait, have_mem);
    const bool chained = why == kChainYes;
    CHECK(S.why == why, "why %d, chain_reason %d", (int)S.why, (int)why);
    CHECK(S.order == (chained ? Schedule::kChained : side ? Schedule::kSideBySide : Schedule::kSequence), "order %d", (int)S.order);
    CHECK(!(chained && side), "chained and side by side at once");
    ++n_order[S.order];
    bool any_fork = false;
    int forks[3] = {0, 0, 0}, joins = 0;
    for (size_t k = 0; k < n; ++k) {
        const LaunchStep &st = S.steps[k];
        CHECK(st.stream >= -1 && st.stream <= 2, "step %zu: stream %d", k, st.stream);
        if (st.stream < -1 || st.stream > 2) return;
        CHECK(!st.wait_fork || st.stream >= 0, "step %zu: the handle's stream waits for its own fork", k);
        if (st.wait_fork && st.stream >= 0) ++forks[st.stream];
        any_fork = any_fork || st.wait_fork;
        joins += st.join_before ? 1 : 0;
        bool first_use = st.stream >= 0;
        for (size_t j = 0; j < k; ++j) if (S.steps[j].stream == st.stream) first_use = false;
        CHECK(st.wait_fork == first_use, "step %zu: wait_fork %d at %s use of side[%d]", k, (int)st.wait_fork, first_use ? "the first" : "a later", st.stream);
    }
    CHECK(S.record_fork == any_fork, "record_fork %d, a step waits for the fork: %d", (int)S.record_fork, (int)any_fork);
    for (int f : forks) CHECK(f <= 1, "a side stream waits for the fork %d times", f);

    if (chained) {
        int last = -1, counting = -1;
        for (size_t k = 0; k < n; ++k) if (B[k].count > 0) last = (int)k;
        std::vector<int> waited(n, 0);
        CHECK(joins == 0 && S.record_fork == (last >= 0), "chained: %d joins before a launch, record_fork %d", joins, (int)S.record_fork);
        for (size_t k = 0; k < n; ++k) {
            const LaunchStep &st = S.steps[k];
            if (B[k].count == 0) {
                CHECK(st.stream == -1 && st.wait_release == -1 && !st.counts_arrival && !st.wait_fork, "step %zu without points: stream %d waits for %d counts %d", k, st.stream, st.wait_release, (int)st.counts_arrival);
                continue;
            }
            CHECK(st.stream == (int)(k & 1), "step %zu on side[%d]", k, st.stream);
            CHECK(st.wait_release == counting, "step %zu waits for %d, the latest counting launch before it is %d", k, st.wait_release, counting);
            if (st.wait_release >= 0) {
                CHECK((size_t)st.wait_release < k && S.steps[(size_t)st.wait_release].counts_arrival, "step %zu waits for %d, which is not an earlier counting launch", k, st.wait_release);
                if ((size_t)st.wait_release < n) ++waited[(size_t)st.wait_release];
            }
            CHECK(st.counts_arrival == ((int)k != last), "step %zu (last with points: %d) counts %d", k, last, (int)st.counts_arrival);
            if (st.counts_arrival) counting = (int)k;
        }
        for (size_t k = 0; k < n; ++k) CHECK(waited[k] == (S.steps[k].counts_arrival ? 1 : 0), "step %zu counts %d and %d launches wait for it", k, (int)S.steps[k].counts_arrival, waited[k]);
        int peak = 0;
        CHECK(simulate(S, B, n, &peak), "the run does not drain");
        CHECK(peak <= 2, "%d chained launches in flight", peak);
        for (size_t cut = 0; cut < n; ++cut) {
            // every wait enqueued up to and including the failing step is on a word the host stores ...
            for (size_t j = 0; j <= cut; ++j) CHECK(S.steps[j].wait_release <= release_upto(S, cut), "failure at %zu: step %zu waits for %d, the host stores 0..%d", cut, j, S.steps[j].wait_release, release_upto(S, cut));
            CHECK(release_upto(S, cut) < (int)cut, "failure at %zu: the host stores words up to %d", cut, release_upto(S, cut));
            // ... and with those stored, what was enqueued drains
            CHECK(simulate(S, B, cut, &peak), "failure at %zu: a stream is left waiting", cut);
        }
        return;
    }

    // ---- side by side (all launches, or the SID_PM_SIDE_FIRST prefix of a run that is reported as a sequence) and sequence
    const size_t n_side = side ? n : sw.side_first >= 0 ? std::min(n, (size_t)sw.side_first) : 0;
    CHECK(S.record_fork == (n_side > 1), "record_fork %d with %zu launches side by side", (int)S.record_fork, n_side);
    CHECK(joins == ((n_side > 1 && n_side < n) ? 1 : 0), "%d joins before a launch (%zu of %zu side by side)", joins, n_side, n);
    bool joined = false;
    for (size_t k = 0; k < n; ++k) {
        const LaunchStep &st = S.steps[k];
        const int want = (k > 0 && k < n_side) ? (int)((k - 1) % 3) : -1;
        CHECK(st.stream == want, "step %zu on stream %d, not %d (%zu side by side)", k, st.stream, want, n_side);
        CHECK(st.join_before == (k == n_side && n_side > 1), "step %zu: join_before %d (%zu side by side)", k, (int)st.join_before, n_side);
        CHECK(st.wait_release == -1 && !st.counts_arrival, "step %zu of an unchained run waits for %d / counts %d", k, st.wait_release, (int)st.counts_arrival);
        joined = joined || st.join_before;
        CHECK(!(joined && st.stream >= 0), "step %zu uses side[%d] after the join", k, st.stream);
    }
    if (n_side <= 1) for (size_t k = 0; k < n; ++k) CHECK(S.steps[k].stream == -1 && !S.steps[k].wait_fork && !S.steps[k].join_before, "sequence: step %zu on stream %d", k, S.steps[k].stream);
    CHECK(release_upto(S, n) == -1, "an unchained run stores release words");
}

int main()
{
    static const int kCounts[4] = {0, 1, 24, 5000};
    static const int kSideFirst[6] = {-1, 0, 1, 2, 3, 9};
    // footprints: one workgroup per CU at even launch indices (5000 points = 19.5 rounds: a long run), four at odd ones (4.9 rounds)
    static const int kLds[2] = {150000, 30000};
    for (size_t len = 1; len <= 6; ++len) {
        size_t combos = 1;
        for (size_t i = 0; i < len; ++i) combos *= 4;
        for (size_t c = 0; c < combos; ++c) {
            std::vector<Bucket> B;
            int offset = 0;
            char counts[80] = "";
            for (size_t i = 0, d = c; i < len; ++i, d /= 4) {
                Bucket b{offset, kCounts[d % 4], kLds[i & 1], 4, 0, 3};
                offset += b.count;
                B.push_back(b);
                snprintf(counts + strlen(counts), sizeof counts - strlen(counts), "%s%d", i ? "," : "", b.count);
            }
            for (int rp = 0; rp < 2; ++rp)
                for (int sbs = -1; sbs <= 1; ++sbs)
                    for (int sf : kSideFirst)
                        for (int mask = 0; mask < 8; ++mask) {
                            Switches sw;
                            sw.side_by_side = sbs; sw.side_first = sf; sw.no_chain = (mask & 1) != 0;
                            snprintf(tag, sizeof tag, "[%s] rp %d side_by_side %d side_first %d no_chain %d wait_value %d memory %d", counts, rp, sbs, sf, mask & 1, (mask >> 1) & 1, (mask >> 2) & 1);
                            check(sw, B, rp != 0, (mask & 2) != 0, (mask & 4) != 0);
                        }
        }
    }
    tag[0] = 0;
    CHECK(n_short > 0 && n_long > 0, "short runs %ld, long runs %ld: the footprints must give both", n_short, n_long);
    CHECK(n_order[0] > 0 && n_order[1] > 0 && n_order[2] > 0, "orders seen: %ld sequence, %ld side by side, %ld chained", n_order[0], n_order[1], n_order[2]);
    printf("%ld sequence, %ld side by side, %ld chained schedules\n%d violations\n", n_order[0], n_order[1], n_order[2], bad);
    return bad ? 1 : 0;
}
