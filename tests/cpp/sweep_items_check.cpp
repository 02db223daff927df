// Host-side invariants of the sweep's work items (sea_ice_drift_amd/csrc/pm_kernel.h rp_sweep_items / rp_sweep_single_lane):
// compiled and run by tests/test_sweep_items.py.  Prints one line per violated invariant; exit code = number of violations
// (capped).  With the argument "units" it prints, per border and band height, the item units of today's and of the chosen
// tiling, those of the busiest of 3 / 4 / 12 wavefronts and the pair / single item counts of both instead (the table DESIGN.md
// section 5.2 quotes).
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include <initializer_list>
#define __host__
#define __device__
#include "../../sea_ice_drift_amd/csrc/pm_kernel.h"

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++bad; if (bad < 40) { printf(__VA_ARGS__); printf("  [%s]\n", #cond); } } } while (0)

using namespace sid;

// units of every wavefront when the items are dealt as rp_sweep deals them: wavefront w takes the pair items w, w + W, ... and
// the single items W-1-w, W-1-w + W, ...; `seen` counts how often an item was taken
static int busiest(const RpSweepItems &I, int W, std::vector<int> *seen_pair = nullptr, std::vector<int> *seen_single = nullptr)
{
    int mx = 0;
    for (int wv = 0; wv < W; ++wv) {
        const int my_pairs = wv < I.n_pair_items ? (I.n_pair_items - wv + W - 1) / W : 0;
        const int wr = W - 1 - wv;
        const int my_singles = wr < I.n_single_items ? (I.n_single_items - wr + W - 1) / W : 0;
        if (seen_pair) for (int i = 0; i < my_pairs; ++i) ++(*seen_pair)[wv + i * W];
        if (seen_single) for (int i = 0; i < my_singles; ++i) ++(*seen_single)[wr + i * W];
        const int u = 2 * my_pairs + my_singles;
        if (u > mx) mx = u;
    }
    return mx;
}

static void check_shape(int s, int wh, int ww, int band, const char *tag)
{
    const int rh = wh - s + 1, rw = ww - s + 1, rem = rw % 32;
    const RpSweepItems T = rp_sweep_items(rh, rw, band, false), I = rp_sweep_items(rh, rw, band, true);
    const RpLdsLayout N = rp_lds_layout(wh, ww, s, true, band);
    // today's tiling is the layout's, and what the paths without ragged items get
    CHECK(T.npair == N.npair && T.nsingle == N.nsingle && T.rem == 0 && T.nbands == (rh + band - 1) / band, "%s: today's tiling", tag);
    CHECK(T.n_pair_items == T.nbands * N.npair && T.n_single_items == T.nbands * N.nsingle && T.units == T.nbands * (2 * N.npair + N.nsingle), "%s: today's counts", tag);
    CHECK(I.units <= T.units && I.units == 2 * I.n_pair_items + I.n_single_items, "%s: %d units, today %d", tag, I.units, T.units);
    if (rem == 0 || rem == 16) CHECK(I.rem == 0, "%s: rem %d is today's tiling by construction", tag, rem);
    if (I.rem == 0) CHECK(I.npair == T.npair && I.nsingle == T.nsingle && I.n_single_items == T.n_single_items && I.units == T.units, "%s: not ragged = today's", tag);
    else {
        CHECK(I.units < T.units && I.rem == rem && I.npair == rw / 32 && I.nsingle == 0 && I.n_single_items == (I.nbands * rem + 15) / 16, "%s: ragged counts", tag);
    }
    // every item is dealt to exactly one wavefront
    for (int W : {3, 4, 12}) {
        std::vector<int> sp(I.n_pair_items, 0), ss(I.n_single_items, 0);
        busiest(I, W, &sp, &ss);
        for (int v : sp) CHECK(v == 1, "%s: W=%d pair item dealt %d times", tag, W, v);
        for (int v : ss) CHECK(v == 1, "%s: W=%d single item dealt %d times", tag, W, v);
    }
    // coverage: key[placement] as the sweep computes it (index of accumulator row 0 + t * rw), against the placement whose bytes the lane reads
    std::vector<int> cover(rh * rw, 0);
    auto visit = [&](int y0, int x, int t, int key) {
        const int row = y0 + t;
        CHECK(row >= 0 && row < rh && x >= 0 && x < rw, "%s: live lane outside the matrix (%d, %d)", tag, row, x);
        if (row < 0 || row >= rh || x < 0 || x >= rw) return;
        CHECK(key == row * rw + x, "%s: placement (%d, %d) scored with key %d", tag, row, x, key);
        ++cover[row * rw + x];
    };
    for (int idx = 0; idx < I.n_pair_items; ++idx) {
        const int order = idx / I.npair, xi = idx - order * I.npair;
        const int bnd = rp_band_of_order(order, I.nbands);
        CHECK(bnd >= 0 && bnd < I.nbands, "%s: band %d", tag, bnd);
        const int y0 = rp_band_y0(bnd, I.nbands, rh, band);
        for (int n = 0; n < 16; ++n)
            for (int k = 0; k < 2; ++k) {
                const int xA = 32 * xi + (n & 3) + 8 * (n >> 2), x = xA + 4 * k, pA = y0 * rw + xA;
                for (int t = 0; t < band; ++t) if (x < rw && y0 + t < rh) visit(y0, x, t, pA + 4 * k + t * rw);
            }
    }
    const int nE = (s + 1) / 2, nO = s / 2 + 1, NS = (nE > nO ? nE : nO) + band / 2 - 1, ncp = (s - 32 + 1) / 2;
    std::vector<int> band_seen(I.nbands, 0);
    const int pitches[2] = {0, rp_class_pitch(N.wpitch)};
    for (int pi = 0; pi < (pitches[1] ? 2 : 1); ++pi) {                   // the natural pitch and the launch class's
        const int pitch = pitches[pi];
        if (pitch && pitch < N.wpitch) continue;
        const RpLdsLayout L = rp_lds_layout(wh, ww, s, true, band, pitch);
        for (int item = 0; item < I.n_single_items; ++item)
            for (int n = 0; n < 16; ++n) {
                const RpSweepLane P = rp_sweep_single_lane(I, rh, rw, item, n);
                CHECK(P.band >= 0 && P.band < I.nbands && P.y0 == rp_band_y0(P.band, I.nbands, rh, band), "%s: item %d lane %d band %d y0 %d", tag, item, n, P.band, P.y0);
                if (I.rem) CHECK(P.x >= 32 * I.npair && P.x < rw, "%s: ragged lane's column %d", tag, P.x);          // (dead lanes too: a valid placement)
                if (P.live) CHECK(P.x >= 32 * I.npair && P.x < rw, "%s: live lane's column %d", tag, P.x);
                if (P.live && pitch == 0) {
                    ++band_seen[P.band];
                    const int pA = P.y0 * rw + P.x;
                    for (int t = 0; t < band; ++t) if (P.y0 + t < rh) visit(P.y0, P.x, t, pA + t * rw);
                }
                // bytes the lane reads, live or not: window (rp_item_main: 5 dwords from the dword of column x + 16 (q & 1), rows
                // y0 + (q >> 1) + 2 j) and transposed strip copy (rp_item_strip: row min(x, rw - 1) + (q & 1) + 2 cp, 20 | 24 bytes)
                for (int q = 0; q < 4; ++q) {
                    const int c0 = (P.x + 16 * (q & 1)) & ~3, rlast = P.y0 + (q >> 1) + 2 * (NS - 1);
                    CHECK(c0 + 20 <= L.wpitch && rlast < L.wrows && rlast * L.wpitch + c0 + 20 <= L.wrows * L.wpitch, "%s: pitch %d: window read row %d byte %d", tag, pitch, rlast, c0);
                    const int v = P.x < rw ? P.x : rw - 1, wrow = v + (q & 1) + 2 * (ncp - 1);
                    const int b0 = P.y0 + 16 * (q >> 1), blast = P.y0 + 32 + (band == 8 ? 24 : 20);
                    CHECK(wrow < L.wp_rows && b0 >= 0 && blast <= L.wp_pitch, "%s: strip read row %d bytes .. %d (%d x %d)", tag, wrow, blast, L.wp_rows, L.wp_pitch);
                }
            }
    }
    for (int i = 0; i < rh * rw; ++i) CHECK(cover[i] >= 1, "%s: placement %d not covered", tag, i);
    // a placement is scored once - except the rows that the pulled-up last 8-row band shares with the one before (same key)
    const int y_last = rp_band_y0(I.nbands - 1, I.nbands, rh, band), overlap_from = y_last, overlap_to = (I.nbands - 1) * band;
    for (int i = 0; i < rh * rw; ++i) {
        const int row = i / rw;
        const bool shared = band >= 8 && row >= overlap_from && row < overlap_to;
        CHECK(cover[i] == (shared ? 2 : 1), "%s: placement %d covered %d times", tag, i, cover[i]);
    }
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "units")) {
        for (int band = 4; band <= 8; band += 4)
            for (int b = 0; b <= 111; ++b) {
                const int r = 2 * b + 2;
                const RpSweepItems T = rp_sweep_items(r, r, band, false), I = rp_sweep_items(r, r, band, true);
                printf("%d %d %d %d %d", band, b, I.rem, T.units, I.units);
                for (int W : {3, 4, 12}) printf(" %d %d", busiest(T, W), busiest(I, W));
                printf(" %d %d %d %d\n", T.n_pair_items, T.n_single_items, I.n_pair_items, I.n_single_items);
            }
        return 0;
    }
    static_assert(rp_sweep_ragged_ok(0) && !rp_sweep_ragged_ok(1) && !rp_sweep_ragged_ok(2), "ragged items: the full-table kernels only");
    for (int s = 34; s <= 35; ++s)
        for (int band = 4; band <= 8; band += 4)
            for (int b = 0; b <= 111; ++b)
                for (int shape = 0; shape < 5; ++shape) {                  // square, narrower, lower, both
                    static const int dws[5] = {0, 3, 0, 6, 11}, dhs[5] = {0, 0, 5, 2, 7};
                    const int hws = s / 2, w = 2 * hws + 2 * b + 1, wh = w - dhs[shape], ww = w - dws[shape];
                    if (wh < s + 1 || ww < s + 1) continue;
                    char tag[96]; snprintf(tag, sizeof tag, "s=%d band=%d b=%d wh=%d ww=%d", s, band, b, wh, ww);
                    check_shape(s, wh, ww, band, tag);
                }
    // the counts DESIGN.md quotes: border 20 (rw = 42, 11 bands of 4 rows) packs 11 x 10 leftover columns into 7 items, and the
    // busiest of three wavefronts goes from 12 to 10 units
    {
        const RpSweepItems I = rp_sweep_items(42, 42, 4, true), T = rp_sweep_items(42, 42, 4, false);
        CHECK(I.rem == 10 && I.n_single_items == 7 && I.units == 29 && T.units == 33 && busiest(T, 3) == 12 && busiest(I, 3) == 10, "border 20");
        // border 24 (rem = 18): 13 pair items become 15 single ones; border 30 (rem = 30, 16 pair items against 30 single ones: 62
        // units against 64, measured 5 % SLOWER) keeps today's tiling
        const RpSweepItems J = rp_sweep_items(50, 50, 4, true), U = rp_sweep_items(50, 50, 4, false);
        CHECK(J.rem == 18 && J.npair == 1 && J.n_single_items == 15 && J.units == 41 && U.units == 52, "border 24");
        CHECK(rp_sweep_items(62, 62, 4, true).rem == 0 && rp_sweep_items(62, 62, 4, true).units == 64, "border 30");
        CHECK(rp_sweep_items(86, 86, 8, true).rem == 22 && rp_sweep_items(94, 94, 8, true).rem == 0, "8-row bands: borders 42, 46");
        // the leftover columns keep the middle-outwards order: the first ragged item starts with the central band
        CHECK(rp_sweep_single_lane(I, 42, 42, 0, 0).band == 5 && rp_sweep_single_lane(I, 42, 42, 0, 10).band == 6 && !rp_sweep_single_lane(I, 42, 42, 6, 14).live, "order of the leftovers");
    }
    printf("%d violations\n", bad);
    return bad > 100 ? 100 : bad;
}
