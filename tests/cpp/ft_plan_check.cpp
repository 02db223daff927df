// Host check of csrc/ft_plan.h: the launch plan of the Hamming matcher (include/sid_ft.h), g++ only.  Over
//   n1 in {0, 1, 255, 256, 257, 4096, 16383, 16384, 16385, 32768, 2^20},
//   n2 in {0, 1, 2, 255, 256, 257, 513, 1023, 1024, 1025, 8200, 2^22 - 1}  and seeded random pairs:
//   valu tiling    the chunks of the one-thread-per-query form tile [0, n2) exactly and none is empty (n2 = 0: one chunk, which
//                  the kernel walks zero times); the second grid dimension stays within 65535
//   mfma tiling    n1pad, n2pad are the sizes rounded up to 256, the chunk is a multiple of 256, the chunks tile [0, n2pad) and
//                  none is empty; every train index fits the 22 index bits of the key
//   regions        part, e1, e2, c2 are 16-byte aligned, lie in this order without overlap and end within
//                  workspace_bytes (= sid_ft_workspace_bytes); so does the part of the one-thread-per-query form
//   switch         use_mfma at 2^24 - 1 / 2^24 pairs and n2 = 1023 / 1024, with and without SID_FT_NO_MFMA
//   limits         n2 = 2^22 - 1 is accepted, 2^22 is not; n1 = (2^31 - 1) / 4 is accepted, one more is not
// Prints "<n> checks" and "<v> violations"; exit status 1 on a violation.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>

#include "../../sea_ice_drift_amd/csrc/ft_plan.h"

namespace {

long g_checks = 0, g_bad = 0;

void expect(bool ok, const char *what, int64_t n1, int64_t n2)
{
    ++g_checks;
    if (ok) return;
    if (++g_bad <= 20) printf("%s: n1 = %lld, n2 = %lld\n", what, (long long)n1, (long long)n2);
}

void check_pair(int64_t n1, int64_t n2)
{
    const int64_t ws = sid_ft::workspace_bytes(n1, n2), rows = n1 > 1 ? n1 : 1;
    {   // one thread per query
        int chunk = -1, nchunks = -1;
        sid_ft::plan(n1, n2, chunk, nchunks);
        expect(chunk >= 1 && nchunks >= 1 && nchunks <= 65535, "valu: sizes", n1, n2);
        if (n2 == 0) expect(nchunks == 1, "valu: empty train set", n1, n2);
        else expect((int64_t)(nchunks - 1) * chunk < n2 && n2 <= (int64_t)nchunks * chunk, "valu: tiling", n1, n2);
        expect(n2 == 0 || n2 - 1 < sid_ft::kMaxTrain, "valu: index bits", n1, n2);
        expect(8 * rows * nchunks <= ws, "valu: part within the workspace", n1, n2);
    }
    {   // MFMA form
        const sid_ft::MfmaPlan P = sid_ft::plan_mfma(n1, n2);
        const int64_t m2 = n2 > 1 ? n2 : 1;
        expect(P.n1pad % 256 == 0 && P.n1pad >= rows && P.n1pad - rows < 256, "mfma: n1pad", n1, n2);
        expect(P.n2pad % 256 == 0 && P.n2pad >= m2 && P.n2pad - m2 < 256, "mfma: n2pad", n1, n2);
        expect(P.n2pad <= sid_ft::kMaxTrain, "mfma: index bits", n1, n2);
        expect(P.chunk >= 256 && P.chunk % 256 == 0, "mfma: chunk of whole batches", n1, n2);
        expect(P.nchunks >= 1 && P.nchunks <= 65535, "mfma: chunks", n1, n2);
        expect((int64_t)(P.nchunks - 1) * P.chunk < P.n2pad && P.n2pad <= (int64_t)P.nchunks * P.chunk, "mfma: tiling", n1, n2);
        const int64_t part_end = 8 * rows * P.nchunks, e1 = (int64_t)P.off_e1, e2 = (int64_t)P.off_e2, c = (int64_t)P.off_c;
        expect(e1 % 16 == 0 && e2 % 16 == 0 && c % 16 == 0, "regions: alignment", n1, n2);
        expect(part_end <= e1, "regions: part / e1", n1, n2);
        expect(e1 + P.n1pad * 256 <= e2, "regions: e1 / e2", n1, n2);
        expect(e2 + P.n2pad * 256 <= c, "regions: e2 / c2", n1, n2);
        expect(c + 4 * P.n2pad <= (int64_t)P.total, "regions: c2 / total", n1, n2);
        expect((int64_t)P.total <= ws, "regions: within the workspace", n1, n2);
    }
}

void check_switch(bool env)
{
    struct Row { int64_t n1, n2; bool mfma; };
    const Row rows[] = {
        {16384, 1024, true},  {16383, 1024, false},           // 2^24 pairs and one row of pairs short of it
        {15184, 1105, true},  {15183, 1105, false},           // 15183 x 1105 = 2^24 - 1 pairs exactly
        {16401, 1023, false}, {16400, 1023, false},           // n2 < 1024 on either side of 2^24 pairs
        {1 << 20, 1023, false}, {1 << 20, 1024, true}, {0, 1024, false}, {1, 1 << 21, false}, {8, 1 << 21, true},
    };
    for (const Row &r : rows) expect(sid_ft::use_mfma(r.n1, r.n2) == (r.mfma && !env), env ? "switch (SID_FT_NO_MFMA)" : "switch", r.n1, r.n2);
}

}  // namespace

int main()
{
    unsetenv("SID_FT_NO_MFMA");
    const int64_t a1[] = {0, 1, 255, 256, 257, 4096, 16383, 16384, 16385, 32768, (int64_t)1 << 20};
    const int64_t a2[] = {0, 1, 2, 255, 256, 257, 513, 1023, 1024, 1025, 8200, ((int64_t)1 << 22) - 1};
    for (int64_t n1 : a1)
        for (int64_t n2 : a2) check_pair(n1, n2);
    std::mt19937_64 rng(20261021);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    for (int k = 0; k < 20000; ++k) {
        const int64_t n1 = (int64_t)exp2(21.0 * unit(rng)) - (k & 1), n2 = (int64_t)exp2(22.0 * unit(rng)) - 1;
        check_pair(n1 < 0 ? 0 : n1, n2);
    }
    check_switch(false);
    setenv("SID_FT_NO_MFMA", "1", 1);
    check_switch(true);
    unsetenv("SID_FT_NO_MFMA");
    check_switch(false);
    const int64_t t = (int64_t)1 << 22, q = 0x7fffffff / 4;
    expect(sid_ft::sizes_supported(1, t - 1), "limit: n2 = 2^22 - 1", 1, t - 1);
    expect(!sid_ft::sizes_supported(1, t), "limit: n2 = 2^22", 1, t);
    expect(sid_ft::sizes_supported(q, 1), "limit: n1 = (2^31 - 1) / 4", q, 1);
    expect(!sid_ft::sizes_supported(q + 1, 1), "limit: n1 one more", q + 1, 1);
    expect(sid_ft::workspace_bytes(-1, 5) == 0 && sid_ft::workspace_bytes(5, -1) == 0, "negative sizes", -1, -1);
    printf("%ld checks\n%ld violations\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
