// Host-side invariants of the classic kernel's LDS layout (sea_ice_drift_amd/csrc/pm_kernel.h mfma_lds_layout) at every
// run-time template side: compiled and run by tests/test_side_cases_cpu.py.  Prints one line per violated invariant; exit
// code = number of violations (capped).
#include <cstdio>
#include <cstdint>
#define __host__
#define __device__
#include "../../sea_ice_drift_amd/csrc/pm_kernel.h"

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++bad; if (bad < 40) { printf(__VA_ARGS__); printf("  [%s]\n", #cond); } } } while (0)

int main()
{
    using namespace sid;
    long checked = 0;
    for (int s = 2; s <= 64; ++s)
        for (int paired = 0; paired <= 1; ++paired)
            for (int b = 0; b <= 70; ++b)
                for (int dw = 0; dw <= 3; dw += 3) {
                    const int hws = s / 2, wh = 2 * hws + 2 * b + 1, ww = wh - dw;
                    if (ww < s + 1 || wh < s + 1) continue;
                    const MfmaLdsLayout L = mfma_lds_layout(wh, ww, s, 4, paired != 0);
                    const int rh = wh - s + 1, rw = ww - s + 1, ntx = (rw + 15) / 16;
                    const int groups = (s + 15) / 16;                       // k-groups of 16 template columns that hold a pixel
                    ++checked;
                    // operand table: 8 (paired) or 16 slots of 16 bytes per k-group, and room for every k-group that holds a pixel
                    CHECK(L.gpitch == (paired ? 8 : 16) * 16, "s=%d paired=%d: gpitch %d", s, paired, L.gpitch);
                    CHECK(L.arow >= groups * L.gpitch, "s=%d paired=%d: a table row of %d B does not hold %d k-groups", s, paired, L.arow, groups);
                    CHECK(L.tab_rows == (paired ? s + 9 : s + 1) && L.arow0 == (paired ? 4 * L.arow : 0), "s=%d paired=%d: tab_rows %d arow0 %d", s, paired, L.tab_rows, L.arow0);
                    // window: every pixel of a row, and the 20 bytes a fragment reads from (x0 + 15 + 16 g) & ~3 for the last tile
                    // and the last k-group that reads addresses of its own
                    const int gmax = s <= 48 ? 2 : 3, last = ((16 * (ntx - 1) + 15 + 16 * gmax) & ~3) + 20;
                    CHECK(L.wpitch >= ww && L.wpitch % 4 == 0, "s=%d b=%d: wpitch %d, window %d wide", s, b, L.wpitch, ww);
                    CHECK(L.wpitch >= last, "s=%d b=%d: wpitch %d, last fragment byte %d", s, b, L.wpitch, last);
                    // regions in order, none overlapping, every one 16-byte aligned
                    CHECK(L.win_off == kMiscMfmaBytes && L.sii_off >= L.win_off + (wh + (paired ? 8 : 4) - 1) * L.wpitch, "s=%d b=%d: window region", s, b);
                    CHECK(L.u_off >= L.sii_off + rh * rw * 4, "s=%d b=%d: sums region", s, b);
                    CHECK(L.patch_off >= L.u_off + L.tab_rows * L.arow + 16, "s=%d b=%d: operand table", s, b);
                    // the winner's operand blocks are zeroed and filled while the templates are still sampled from the patch
                    CHECK(L.patch_off >= L.u_off + 2 * L.trow_bytes, "s=%d paired=%d: the winner's operands (%d B) reach the patch at %d", s, paired, 2 * L.trow_bytes, L.patch_off - L.u_off);
                    CHECK(L.queue_off >= L.patch_off + L.pdim * L.ppitch + 1, "s=%d b=%d: patch", s, b);
                    CHECK(L.total >= L.queue_off + kQueueCap * 16, "s=%d b=%d: queue", s, b);
                    CHECK(L.total >= L.u_off + 2 * L.trow_bytes + rh * rw * 4, "s=%d b=%d: winner operands + NCC matrix", s, b);
                    CHECK(L.total >= L.u_off + rh * ww * 4, "s=%d b=%d: column sums", s, b);
                    CHECK(2 * L.trow_bytes >= 5 * 1024, "s=%d: the Hessian's histograms need 5 KB of the dead winner operands", s);
                    CHECK(L.sii_off % 16 == 0 && L.u_off % 16 == 0 && L.patch_off % 16 == 0 && L.queue_off % 16 == 0 && L.total % 16 == 0, "s=%d b=%d: alignment", s, b);
                    // the patch holds every sample of a rotated template: radius hypot(tc, tc) + 1 around the centre
                    const int tc = s / 2 + 1;
                    CHECK((L.pradius - 1) * (L.pradius - 1) >= 2 * tc * tc && L.pdim == 2 * L.pradius + 2 && L.ppitch >= L.pdim, "s=%d: patch radius %d", s, L.pradius);
                    // the winner's operand block: 16 + s - 1 steps taken in fours stay inside s + kTrowPad rows
                    CHECK(L.trow_bytes >= 4 * (s + kTrowPad) * 16 && ((16 + s - 1 + 3) / 4) * 4 <= s + kTrowPad - 16, "s=%d: trow_bytes %d", s, L.trow_bytes);
                }
    printf("%ld layouts, %d violations\n", checked, bad);
    return bad > 100 ? 100 : bad;
}
