// pm_kernel_classic.h - the classic PM kernel: template sides 2..64, one template row per matrix instruction (the scheme at the
// top of pm_kernel_mfma.hip).
//
// Holds: ph_window, ph_sums, the operand phases ph_tpl_begin / _general / _table / _fix / _end, sweep_item, ph_sweep,
// ph_winner_stage, ph_winner and the kernel pm_kernel_mfma<S, BAND, PAIRED>.
// Needs: pm_kernel_phases.h.  Instantiated with SID_PM_OCC = 3 only (pm_kernel_mfma.hip).
#pragma once
#include "pm_kernel_phases.h"

namespace sid {

namespace {

__device__ __forceinline__ void ph_window(const uint8_t *img2, long long rows2, long long cols2, long long stride2)
{
    ph_window_t<false>(img2, rows2, cols2, stride2, nullptr, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------
// Phase 1: S_II' = box sums of w'^2 (running sums down the columns, then along the rows).
// ---------------------------------------------------------------------------------------------
__device__ __noinline__ void ph_sums()
{
    SID_PHASE_LOCALS;
    const uint8_t *win = smem + G.win_off;
    u32 *sii = reinterpret_cast<u32 *>(smem + G.sii_off);
    u32 *colsum = reinterpret_cast<u32 *>(smem + G.u_off);
    const int s = G.s, ww = G.ww, rh = G.rh, rw = G.rw, wpitch = G.wpitch;
    // Both passes cut their running sums into segments so that the whole workgroup works and the chain of
    // dependent LDS reads is short: a segment starts from a directly summed value (s independent reads)
    // and slides over its few rows / columns.
    {   // down the columns: thread = (column x, segment of rows)
        int nseg = kBlockM / ww; nseg = nseg < 1 ? 1 : (nseg > rh ? rh : nseg);
        const int per = (rh + nseg - 1) / nseg;
        for (int task = tid; task < ww * nseg; task += kBlockM) {
            const int seg = task / ww, x = task - seg * ww;
            const int ya = seg * per, yb = ya + per < rh ? ya + per : rh;
            if (ya >= yb) continue;
            const int8_t *col = reinterpret_cast<const int8_t *>(win) + x + ya * wpitch;
            int c = 0;
#pragma unroll 8
            for (int i = 0; i < s; ++i) { const int v = col[i * wpitch]; c += v * v; }
            colsum[ya * ww + x] = (u32)c;
#pragma unroll 4
            for (int y = 1; y < yb - ya; ++y) {
                const int vo = col[(y - 1) * wpitch], vn = col[(y + s - 1) * wpitch];
                c += vn * vn - vo * vo;
                colsum[(ya + y) * ww + x] = (u32)c;
            }
        }
    }
    __syncthreads();
    {   // along the rows: thread = (row y, segment of columns)
        int nseg = kBlockM / rh; nseg = nseg < 1 ? 1 : (nseg > rw ? rw : nseg);
        const int per = (rw + nseg - 1) / nseg;
        for (int task = tid; task < rh * nseg; task += kBlockM) {
            const int y = task / nseg, seg = task - y * nseg;
            const int xa = seg * per, xb = xa + per < rw ? xa + per : rw;
            if (xa >= xb) continue;
            const u32 *cr = colsum + y * ww + xa;
            u32 acc = 0;
#pragma unroll 8
            for (int j = 0; j < s; ++j) acc += cr[j];
            sii[y * rw + xa] = acc;
#pragma unroll 4
            for (int x = 1; x < xb - xa; ++x) {
                acc += cr[x + s - 1] - cr[x - 1];
                sii[y * rw + xa + x] = acc;
            }
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// Phase 0c: operands of one group of <= 15 angles.  afrag[i][lane = g*16 + slot][16 bytes], byte jj
// <-> column c = 16 g + jj; slot 15 is the all-ones template; row s is all zero.
// Four small functions (begin / one of the two samplers / end) so that the common sampler - the table
// path - does not inherit the register appetite (and callee-saved spills) of the general one.
// ---------------------------------------------------------------------------------------------
template <int S>
__device__ __noinline__ void ph_tpl_begin(const double *rot, int a0, int Kg, long long *dbg_cycles)
{
    SID_PHASE_LOCALS;
    uint8_t *afrag = smem + G.u_off;
    const int arow = G.arow;
    if (tid < 4 * Kg) (&m->rot[0][0])[tid] = rot[4 * a0 + tid];        // one global round trip for the whole group
    for (int idx = tid; idx < G.tab_rows * arow / 16; idx += kBlockM) reinterpret_cast<uint4 *>(afrag)[idx] = make_uint4(0, 0, 0, 0);
    if (tid < kSlots) { m->isT[tid] = 0; m->isTT[tid] = 0; }
    __syncthreads();                                                   // also: patch complete
    if (dbg_cycles && tid == 0) dbg_cycles[8] = (long long)clock64();
}

// general sampler: any centre, any position relative to the image border
template <int S>
__device__ __noinline__ void ph_tpl_general(int a0, int Kg, long long rows1, long long cols1)
{
    SID_PHASE_LOCALS;
    uint8_t *afrag = smem + G.u_off;
    const uint8_t *patch = smem + G.patch_off;
    const int s = S > 0 ? S : G.s, arow = G.arow;                      // compile-time s: divisions by s become multiplies
    const SampleGeom g = sample_geom(G, s, rows1, cols1, patch);
    const int dump = G.tab_rows * arow;                                // 16 scratch bytes behind the operand table
    // byte offset of (row ig + k*ngrp, column j, slot a) = wbase + k*wstep + 16 a
    const int wbase = G.arow0 + g.ig * arow + (g.j >> 4) * G.gpitch + (g.j & 15), wstep = g.ngrp * arow;
    int sawzero = 0;
    auto run = [&](auto inside_tag) {
        constexpr bool INSIDE = decltype(inside_tag)::value;
        unsigned long long dlo = 0, dhi = 0;
        for (int k0 = 0; k0 * g.ngrp < s; k0 += kRowsPerThread) {
            for (int a = 0; a < Kg; a += 3) {                          // three angles in flight: their chains interleave
                int st[3] = {0, 0, 0}, stt[3] = {0, 0, 0};
                u32 db[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int aa = a + q < Kg ? a + q : Kg - 1;
                    db[q] = sample_fast5<INSIDE>(g, m->rot[aa], a + q < Kg, k0, st[q], stt[q], sawzero,
                        [&](int k, int, int v, bool take) { afrag[take ? wbase + k * wstep + 16 * aa : dump] = (uint8_t)(v ^ 0x80); });
                }
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    if (a + q < Kg) {                                  // wavefront-uniform
                        const int ws = wave_sum_dpp(st[q]), wss = wave_sum_dpp(stt[q]);
                        if (lane == 0) { atomicAdd(&m->isT[a + q], ws); atomicAdd(&m->isTT[a + q], wss); }
                        // remember the doubtful samples: bit 5*(a+q) + u of a 128-bit mask
                        const int pos = 5 * (a + q);
                        const unsigned long long d = (unsigned long long)db[q];
                        if (pos < 64) { dlo |= d << pos; if (pos > 59) dhi |= d >> (64 - pos); }
                        else dhi |= d << (pos - 64);
                    }
                }
            }
            // rare: redo the doubtful samples of this chunk with scipy's double arithmetic (kept apart
            // from the DPP reductions above: no divergent code between them)
            if (dlo | dhi) {
                for (int aa = 0; aa < Kg; ++aa) {
                    const int pos = 5 * aa;
                    const u32 dbits = (u32)((pos < 64 ? (dlo >> pos) | (pos > 59 ? dhi << (64 - pos) : 0ull) : dhi >> (pos - 64)) & 31ull);
                    for (int u = 0; u < kRowsPerThread; ++u) {
                        if ((dbits >> u) & 1u) {
                            const int i = g.ig + (k0 + u) * g.ngrp;
                            const int v = sample_exact(g, m->rot[aa], i, g.j, a0 + aa);
                            sawzero |= (v == 0) ? 1 : 0;
                            afrag[wbase + (k0 + u) * wstep + 16 * aa] = (uint8_t)(v ^ 0x80);
                            atomicAdd(&m->isT[aa], v - 128); atomicAdd(&m->isTT[aa], (v - 128) * (v - 128));
                        }
                    }
                }
            }
            dlo = 0; dhi = 0;
        }
    };
    if (g.inside) run(std::true_type{}); else run(std::false_type{});
    if (sawzero) m->zero_flag = 1;
}

// table sampler: integral template centre, patch inside image 1 (table_usable)
template <int S>
__device__ __noinline__ void ph_tpl_table(const uint16_t *samp, int a0, int Kg, long long rows1, long long cols1)
{
    SID_PHASE_LOCALS;
    uint8_t *afrag = smem + G.u_off;
    const uint8_t *patch = smem + G.patch_off;
    const int s = S > 0 ? S : G.s, arow = G.arow;
    int sawzero = 0;
    {
        // one wavefront per angle: four samples per lane and step through the offset table, one dword store
        // into the operand table; pixel sums by v_dot4 on the packed raw bytes, converted to the re-centred
        // domain per angle: sum(v-128) = sum v - 128 N, sum(v-128)^2 = sum v^2 - 256 sum v + 16384 N
        const int sp = samp_pitch(s), nq = sp >> 2, upa = s * nq;
        const u32 tailmask = (s & 3) ? (1u << (8 * (s & 3))) - 1u : 0xffffffffu;
        // table entries are fetched a whole chunk (kCh steps of 64 lanes) ahead - those of the next angle while
        // this one is gathered - so that the L2 latency of the table is paid once per wavefront, not per step
        constexpr int kCh = S > 0 ? (S * ((S + 3) / 4) + 63) / 64 : 4;
        auto fetch = [&](int a, int u0, uint2 (&e)[kCh]) {
            const uint2 *ta = reinterpret_cast<const uint2 *>(samp + (size_t)(a0 + a) * s * sp);
#pragma unroll
            for (int c = 0; c < kCh; ++c) {
                const int u = u0 + 64 * c + lane;
                e[c] = ta[u < upa ? u : 0];
            }
        };
        uint2 cur[kCh] = {}, nxt[kCh] = {};
        if (wv < Kg) fetch(wv, 0, cur);
        for (int a = wv; a < Kg; a += kWavesM) {
            u32 sv = 0, svv = 0, zero = 0;
            for (int u0 = 0; u0 < upa; u0 += 64 * kCh) {
                // what comes next: the following chunk of this angle, else the first chunk of the next angle
                const bool more = u0 + 64 * kCh < upa;
                if (more) fetch(a, u0 + 64 * kCh, nxt);
                else if (a + kWavesM < Kg) fetch(a + kWavesM, 0, nxt);
                // all gathers of the chunk first (branch-free: their LDS latencies overlap)
                u32 rawv[kCh];
#pragma unroll
                for (int c = 0; c < kCh; ++c) rawv[c] = gather_quad(patch, cur[c]);
#pragma unroll
                for (int c = 0; c < kCh; ++c) {
                    const int u = u0 + 64 * c + lane;
                    if (u < upa) {
                        const int i = u / nq, jq = u - i * nq;
                        const u32 vm = jq == nq - 1 ? tailmask : 0xffffffffu;
                        const u32 raw = rawv[c] & vm;
                        const u32 z = raw | ~vm;
                        zero |= (z - 0x01010101u) & ~z & 0x80808080u;  // some valid byte == 0
                        sv = __builtin_amdgcn_udot4(raw, 0x01010101u, sv, false);
                        svv = __builtin_amdgcn_udot4(raw, raw, svv, false);
                        *reinterpret_cast<u32 *>(afrag + G.arow0 + i * arow + (jq >> 2) * G.gpitch + a * 16 + (jq & 3) * 4) = (raw ^ 0x80808080u) & vm;
                    }
                }
#pragma unroll
                for (int c = 0; c < kCh; ++c) cur[c] = nxt[c];
            }
            const int ws = wave_sum_dpp((int)sv), wss = wave_sum_dpp((int)svv);
            if (lane == 0) { m->isT[a] = ws - 128 * s * s; m->isTT[a] = wss - 256 * ws + 16384 * s * s; }
            sawzero |= zero != 0u ? 1 : 0;
        }
    }
    if (sawzero) m->zero_flag = 1;
}

// Rare (only when the host flagged table entries, A.samp_nflag > 0): the samples whose coordinate sits
// within kSampGuard of a rounding boundary, recomputed with the reference's float64 operation order.
// winner_ka < 0: operand table of the angle group (+ template sums, zero guard); else: the winner's operands.
template <int S>
__device__ __noinline__ void ph_tpl_fix(const uint16_t *samp, int a0, int Kg, long long rows1, long long cols1, int winner_ka)
{
    SID_PHASE_LOCALS;
    __syncthreads();                                                   // the sampler's stores and sums are complete
    const uint8_t *patch = smem + G.patch_off;
    const int s = S > 0 ? S : G.s, arow = G.arow, sp = samp_pitch(s);
    const SampleGeom g = sample_geom(G, s, rows1, cols1, patch);
    const int a_lo = winner_ka < 0 ? 0 : 0, a_n = winner_ka < 0 ? Kg : 1;
    for (int idx = tid; idx < a_n * s * sp; idx += kBlockM) {
        const int a = idx / (s * sp), rem = idx - a * s * sp;
        const int i = rem / sp, j = rem - i * sp;
        const int ag = winner_ka < 0 ? a0 + a_lo + a : winner_ka;      // angle index in the table
        if (j >= s || !(samp[(size_t)ag * s * sp + rem] & 0x8000u)) continue;
        const double *rot4 = winner_ka < 0 ? m->rot[a] : m->rot[0];
        const int v = sample_exact(g, rot4, i, j, -1);                  // (table path: never with pre-sampled templates)
        if (winner_ka < 0) {
            (smem + G.u_off)[G.arow0 + i * arow + (j >> 4) * G.gpitch + a * 16 + (j & 15)] = (uint8_t)(v ^ 0x80);
            atomicAdd(&m->isT[a], v - 128); atomicAdd(&m->isTT[a], (v - 128) * (v - 128));
            if (v == 0) m->zero_flag = 1;
        } else {
            const int trows = s + kTrowPad;
            (smem + G.u_off)[((j >> 4) * trows + 16 + i) * 16 + (j & 15)] = (uint8_t)(v ^ 0x80);
        }
    }
}

template <int S>
__device__ __noinline__ void ph_tpl_end(int a0, int Kg, uint8_t *dbg_templates, long long *dbg_cycles)
{
    SID_PHASE_LOCALS;
    uint8_t *afrag = smem + G.u_off;
    const int s = S > 0 ? S : G.s, arow = G.arow;
    const double nd = G.nd;
    if (dbg_cycles && tid == 0) dbg_cycles[15] = (long long)clock64();
    for (int idx = tid; idx < s * s; idx += kBlockM) {                  // slot 15: all-ones template
        const int i = idx / s, j = idx - i * s;
        afrag[G.arow0 + i * arow + (j >> 4) * G.gpitch + G.ones_slot * 16 + (j & 15)] = 1;
    }
    __syncthreads();
    if (dbg_cycles && tid == 0) dbg_cycles[9] = (long long)clock64();
    if (dbg_templates) {
        for (int idx = tid; idx < Kg * s * s; idx += kBlockM) {
            const int a = idx / (s * s), rem = idx - a * s * s;
            const int i = rem / s, j = rem - i * s;
            dbg_templates[(a0 + a) * s * s + rem] = afrag[G.arow0 + i * arow + (j >> 4) * G.gpitch + a * 16 + (j & 15)] ^ 0x80;
        }
    }
    if (tid < Kg) {                                                    // per-angle terms (signed domain)
        const double st = (double)m->isT[tid], stt = (double)m->isTT[tid];
        const double dT = nd * stt - st * st;                          // exact
        const double rT = 1.0 / sqrt(dT);
        m->sTd[a0 + tid] = st;
        m->constT[a0 + tid] = dT == 0.0 ? 1 : 0;
        m->rTd[a0 + tid] = rT;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// One sweep work item: kBand output rows x 16 placements x 16 template slots.
// Window row rho = y0 + step feeds output row y0 + t through template row i = step - t, whose
// fragment sits in ring slot (i & (kBand-1)).  S > 0: template side known at compile time - the whole
// schedule is static (no branch, exactly kBand*S MFMAs).  S == 0: runtime side; the ring holds zero
// fragments for i outside [0, s) so the MFMAs of a step are unconditional.
// Lane (n = l&15, g = l>>4): B fragment = bytes W'[row][x0+n+16g .. +15], built from 5 dwords read at
// the lane's dword-aligned address + v_alignbyte_b32; A fragment = 16 bytes of the operand table
// (lanes of k-group 3 read the all-zero row when s <= 48: their per-lane row stride is 0).
// ---------------------------------------------------------------------------------------------
template <int S, int kBand>
__device__ __forceinline__ void sweep_item(v4i (&acc)[kBand], const uint8_t *ap, int arow_l, const uint8_t *bp,
                                           int wpitch, int s, u32 sh)
{
#pragma unroll
    for (int t = 0; t < kBand; ++t) acc[t] = v4i{0, 0, 0, 0};
    v4i ring[kBand];
#pragma unroll
    for (int t = 0; t < kBand; ++t) ring[t] = v4i{0, 0, 0, 0};
    if (S > 0) {
        constexpr int NS = kBand + (S > 0 ? S : 1) - 1;
        // Software pipeline of depth 2, interleaved with the MFMAs of the current step (a single
        // wavefront issues in order: anything not placed between two MFMAs adds to the step time):
        //   step k:  MFMAs(k)  ||  finish the window fragment of k+1 (alignbyte x4)  ||  issue LDS reads of k+2
        ring[0] = *reinterpret_cast<const v4i *>(ap);
        v4i b_cur = align_raw(read_raw(bp), sh);
        v4i a_nxt = *reinterpret_cast<const v4i *>(ap + arow_l);
        Raw5 b_raw = read_raw(bp + wpitch);
        ap += 2 * arow_l; bp += 2 * wpitch;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int step = 0; step < NS; ++step) {
            const v4i a_fin = a_nxt;
            const v4i b_nxt = align_raw(b_raw, sh);                  // reads were issued during step-1
            if (step + 2 < NS) {                                     // reads of step+2
                if (step + 2 < S) a_nxt = *reinterpret_cast<const v4i *>(ap);
                b_raw = read_raw(bp);
                ap += arow_l; bp += wpitch;
            }
#pragma unroll
            for (int t = 0; t < kBand; ++t) {
                const int i = step - t;
                if (i >= 0 && i < S)
                    acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ring[i & (kBand - 1)], b_cur, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int g = 0; g < kBand; ++g) {                        // one MFMA, then up to four of the others
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x106, 4, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (step + 1 < S) ring[(step + 1) & (kBand - 1)] = a_fin;
            b_cur = b_nxt;
        }
    } else {
        const int nsteps = kBand + s - 1;
        for (int cbase = 0; cbase < nsteps; cbase += kBand) {
#pragma unroll
            for (int u = 0; u < kBand; ++u) {
                const int step = cbase + u;
                const int ia = step < s ? step : s;                   // row s of the operand table is all zero
                ring[u] = *reinterpret_cast<const v4i *>(ap + ia * arow_l);
                const v4i b = align_raw(read_raw(bp + step * wpitch), sh);
#pragma unroll
                for (int t = 0; t < kBand; ++t)
                    acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ring[(u - t) & (kBand - 1)], b, acc[t], 0, 0, 0);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Phase 2: angle-major sweep of one group.  Every wavefront takes work items wv, wv+W, ... and scores
// the kBand x 16 x 15 results of each item:
//   pass A (always, branch-free): float32 estimate of this lane's kBand x 4 values and their maximum;
//   pass B (only if the item can hold an arg-max candidate: its maximum is within kMargin of the
//   running maximum, or an estimate is NaN = degenerate window/template): estimates within kMargin
//   of the running maximum are queued for exact evaluation.  |estimate - value| <= 4e-7, so the
//   true arg-max is always queued.
// ---------------------------------------------------------------------------------------------
// PAIRED (at most 7 angles, one group): the 16 MFMA slots hold the angles + the all-ones template twice;
// the lanes of slots 8..15 read the operand table four rows earlier, so their accumulators belong to the
// output rows kBand below those of slots 0..7 - an item covers 2 * kBand rows with the same kBand
// accumulators, i.e. nearly half the MFMAs, window fragments and LDS traffic per output row.
template <int S, int kBand, bool PAIRED>
__device__ __forceinline__ Score ph_sweep(Score sc, int a0, int Kg, long long *dbg_cycles)
{
    static_assert(!PAIRED || kBand == 4, "the operand table of the paired mode is shifted by four rows");
    SID_PHASE_LOCALS;
    const uint8_t *afrag = smem + G.u_off;
    const uint8_t *win = smem + G.win_off;
    const u32 *sii = reinterpret_cast<const u32 *>(smem + G.sii_off);
    uint4 *queue = reinterpret_cast<uint4 *>(smem + G.queue_off);
    const int s = S > 0 ? S : G.s, rh = G.rh, rw = G.rw, wpitch = G.wpitch, arow = G.arow;
    const double nd = G.nd;
    const bool zero_a = (s <= 48) && q_l == 3;
    // lanes of k-group 3 sit on a zero row with stride 0
    const uint8_t *abase = PAIRED ? (zero_a ? afrag : afrag + (n_l >= 8 ? 0 : 4) * arow + q_l * 128 + (n_l & 7) * 16)
                                  : (zero_a ? afrag + s * arow : afrag + lane * 16);
    const int arow_l = zero_a ? 0 : arow;
    constexpr int kRows = PAIRED ? 2 * kBand : kBand;                  // output rows per work item
    const int yq = PAIRED ? kBand * (q_l >> 1) : 0;                    // this lane's accumulators: rows y0 + yq + t
    // accumulator register r of this lane belongs to slot 4 q + r: angle index (the ones slot never is < Kg)
    auto angle_of = [&](int r) { return PAIRED ? ((4 * q_l + r) & 7) : 4 * q_l + r; };

    // estimate of slot r at a placement: float(acc * A4[r] - Sw' * B4[r]) * rsq(dI), with the template's
    // 1/sqrt(dT) folded into both per-slot factors (NaN for a constant template => always a candidate)
    double A4[4], B4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int a = angle_of(r);
        const double rTa = a < Kg ? (m->constT[a0 + a] ? (double)NAN : m->rTd[a0 + a]) : 0.0;
        A4[r] = nd * rTa;
        B4[r] = (a < Kg ? m->sTd[a0 + a] : 0.0) * rTa;
    }
    const u32 livebits = (angle_of(0) < Kg ? 1u : 0u) | (angle_of(1) < Kg ? 2u : 0u) |
                         (angle_of(2) < Kg ? 4u : 0u) | (angle_of(3) < Kg ? 8u : 0u);
#define STAMP2(k) do { if (dbg_cycles && tid == 0) dbg_cycles[k] = (long long)clock64(); } while (0)

    const int nbands = (rh + kRows - 1) / kRows, ntx = (rw + 15) / 16;
    for (int item = wv; item < nbands * ntx; item += kWavesM) {
        const int band = item / ntx, xt = item - band * ntx;
        const int y0 = band * kRows, x0 = xt * 16;
        // k-group 3 multiplies the all-zero template columns (s <= 48): its lanes read the window bytes of
        // k-group 0 (same addresses = LDS broadcast, and the window pitch needs no room for columns 48..63)
        const u32 sbyte = (u32)(x0 + n_l + 16 * (zero_a ? 0 : q_l));
        const u32 sh = sbyte & 3u;
        if (item == wv) STAMP2(10);
        v4i acc[kBand];
        sweep_item<(PAIRED && S > 0) ? S + 4 : S, kBand>(acc, abase, arow_l, win + y0 * wpitch + (sbyte & ~3u), wpitch,
                                                         PAIRED ? s + 4 : s, sh);
        if (item == wv) STAMP2(11);

        {
            const float gm = key2f(m->gmax_key);
            sc.lmax = gm > sc.lmax ? gm : sc.lmax;
        }
        const int x = x0 + n_l;
        const bool xok = x < rw;
        // operands of all rows first (one LDS round trip), then straight-line arithmetic
        int swp[kBand];
        u32 siiv[kBand];
#pragma unroll
        for (int t = 0; t < kBand; ++t) {
            // the ones slot = sum of w': slot 15 (lanes 48..63, register 3), or slots 7 / 15 in paired mode
            swp[t] = __builtin_amdgcn_ds_bpermute((PAIRED ? n_l + 16 + 32 * (q_l >> 1) : n_l + 48) << 2, acc[t][3]);
            const int y = y0 + yq + t;
            siiv[t] = sii[(xok & (y < rh)) ? y * rw + x : 0];
        }
        auto estimate_row = [&](int t, float (&e)[4]) {
            const double swd = (double)swp[t], siid = (double)siiv[t];
            const double dI = nd * siid - swd * swd;                  // exact
            float rIf = __builtin_amdgcn_rsqf((float)dI);
            rIf = (2.0 * dI <= nd) ? NAN : rIf;                       // (nearly) flat window: the exact path decides
            const u32 lv = (xok & (y0 + yq + t < rh)) ? livebits : 0u;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = (float)__builtin_fma((double)acc[t][r], A4[r], -(swd * B4[r])) * rIf;
                e[r] = ((lv >> r) & 1u) ? v : -INFINITY;
            }
        };
        float itemmax = -INFINITY;
        u32 nanbits = 0;
#pragma unroll
        for (int t = 0; t < kBand; ++t) {
            float e[4];
            estimate_row(t, e);
#pragma unroll
            for (int r = 0; r < 4; ++r) { itemmax = fmaxf(itemmax, e[r]); nanbits |= (e[r] != e[r]) ? 1u : 0u; }
        }
        const float wavemax = wave_max_dpp(itemmax);
        const bool need_b = (wavemax >= sc.lmax - kMargin) || (__ballot(nanbits != 0) != 0ull);   // wavefront-uniform
        sc.lmax = fmaxf(sc.lmax, wavemax);
        if (need_b) {
            const float thr = sc.lmax - kMargin;
            u32 ovf = 0;                                              // candidates that found the queue full
#pragma unroll
            for (int t = 0; t < kBand; ++t) {
                float e[4];
                estimate_row(t, e);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (e[r] != -INFINITY && !(e[r] < thr)) {         // live, and true for NaN
                        const int a = angle_of(r);
                        const int key = ((a0 + a) * rh + y0 + yq + t) * rw + x;
                        const u32 slot = atomicAdd(&m->qcount, 1u);
                        if (slot < (u32)kQueueCap) queue[slot] = make_uint4((u32)acc[t][r], (u32)swp[t], siiv[t], (u32)key);
                        else ovf |= 1u << (4 * t + r);
                    }
                }
            }
            // Cold path (queue full: massive exact ties, flat windows): evaluate the left-over candidates
            // here, one at a time.  A rolled loop with one copy of the double-precision sequence and
            // operand selection by compare chains - no call, so the sweep stays a leaf function and
            // needs no callee-saved registers.
            if (ovf) {
#pragma unroll 1
                for (int b = 0; b < 4 * kBand; ++b) {
                    if (!((ovf >> b) & 1u)) continue;
                    const int t = b >> 2, r = b & 3;
                    int pv = 0, sw = 0; u32 si = 0;
#pragma unroll
                    for (int tt = 0; tt < kBand; ++tt) {
                        sw = t == tt ? swp[tt] : sw;
                        si = t == tt ? siiv[tt] : si;
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) pv = b == 4 * tt + rr ? acc[tt][rr] : pv;
                    }
                    const int a = angle_of(r);
                    const int key = ((a0 + a) * rh + y0 + yq + t) * rw + x;
                    take_better(sc, exact_from_sums(pv, sw, si, nd, m->sTd[a0 + a], m->rTd[a0 + a], m->constT[a0 + a] != 0), key);
                }
            }
        }
        if (lane == 0) atomicMax(&m->gmax_key, f2key(sc.lmax));
        if (item == wv) STAMP2(12);
    }
#undef STAMP2
    __syncthreads();
    // exact (double) evaluation of the queued candidates of this group
    {
        const int nq = (int)(m->qcount < (u32)kQueueCap ? m->qcount : (u32)kQueueCap);
        for (int idx = tid; idx < nq; idx += kBlockM) {
            const uint4 rec = queue[idx];
            const int key = (int)rec.w;
            const int a = key / G.npos;
            take_better(sc, exact_from_sums((int)rec.x, (int)rec.y, rec.z, nd, m->sTd[a], m->rTd[a], m->constT[a] != 0), key);
        }
    }
    __syncthreads();                                                   // operands / queue are rewritten by the next group
    if (tid == 0) m->qcount = 0;
    return sc;
}

// ---------------------------------------------------------------------------------------------
// Phase 4: NCC matrix of the winning angle, row-major MFMA (M = 16 output rows): ph_winner_stage builds the
// operands, ph_winner runs the tiles.
// trow[g][16 + i][16 B] holds the winner's template, trow1 the all-ones one; zero rows around.
// ---------------------------------------------------------------------------------------------
template <int S>
__device__ __noinline__ void ph_winner_stage(const double *rot4, const uint16_t *samp, long long rows1, long long cols1, int ka)
{
    SID_PHASE_LOCALS;
    const uint8_t *patch = smem + G.patch_off;
    uint8_t *trow = smem + G.u_off;
    uint8_t *trow1 = trow + G.trow_bytes;
    const int s = S > 0 ? S : G.s;
    const int trows = s + kTrowPad;
    for (int idx = tid; idx < 2 * G.trow_bytes / 4; idx += kBlockM) reinterpret_cast<u32 *>(trow)[idx] = 0;
    __syncthreads();
    {
        if (tid < 4) m->rot[0][tid] = rot4[tid];
        __syncthreads();
        const SampleGeom g = sample_geom(G, s, rows1, cols1, patch);
        const int pdump = 0;                                           // row 0 of k-group 0 is never read
        auto put = [&](int i, int j, int v, bool take = true) {
            const int off = take ? ((j >> 4) * trows + 16 + i) * 16 + (j & 15) : pdump;
            trow[off] = (uint8_t)(v ^ 0x80);
            trow1[off] = take ? 1 : 0;
        };
        if (samp) {                                                    // caller checked table_usable
            const int sp = samp_pitch(s), nq = sp >> 2, upa = s * nq;
            const u32 tailmask = (s & 3) ? (1u << (8 * (s & 3))) - 1u : 0xffffffffu;
            const uint2 *ta = reinterpret_cast<const uint2 *>(samp + (size_t)ka * s * sp);
            for (int u = tid; u < upa; u += kBlockM) {
                const int i = u / nq, jq = u - i * nq;
                const u32 vm = jq == nq - 1 ? tailmask : 0xffffffffu;
                const u32 raw = gather_quad(patch, ta[u]);
                const int off = ((jq >> 2) * trows + 16 + i) * 16 + (jq & 3) * 4;
                *reinterpret_cast<u32 *>(trow + off) = (raw ^ 0x80808080u) & vm;
                *reinterpret_cast<u32 *>(trow1 + off) = 0x01010101u & vm;
            }
        } else
        for (int k0 = 0; k0 * g.ngrp < s; k0 += kRowsPerThread) {
            int st = 0, stt = 0, sz = 0;
            const u32 db = sample_fast5<false>(g, m->rot[0], true, k0, st, stt, sz,
                                               [&](int, int i, int v, bool take) { put(i, g.j, v, take); });
            for (int u = 0; u < kRowsPerThread; ++u)
                if ((db >> u) & 1u) { const int i = g.ig + (k0 + u) * g.ngrp; put(i, g.j, sample_exact(g, m->rot[0], i, g.j, ka)); }
        }
    }
}

template <int S>
__device__ __noinline__ void ph_winner(int ka, long long *dbg_cycles)
{
    SID_PHASE_LOCALS;
    const uint8_t *win = smem + G.win_off;
    const u32 *sii = reinterpret_cast<const u32 *>(smem + G.sii_off);
    const uint8_t *trow = smem + G.u_off;
    const uint8_t *trow1 = trow + G.trow_bytes;
    float *ccm = reinterpret_cast<float *>(smem + G.u_off + 2 * G.trow_bytes);
    const int s = S > 0 ? S : G.s, rh = G.rh, rw = G.rw, wpitch = G.wpitch;
    const double nd = G.nd;
    const int trows = s + kTrowPad;
    __syncthreads();                                                   // the staged operands (and their fixes) are complete
    if (dbg_cycles && tid == 0) dbg_cycles[13] = (long long)clock64();
    const double sT = m->sTd[ka], rT = m->rTd[ka];
    const bool cT = m->constT[ka] != 0;
    const int nty = (rh + 15) / 16, ntx = (rw + 15) / 16;
    for (int item = wv; item < nty * ntx; item += kWavesM) {
        const int yt = item / ntx, xt = item - yt * ntx;
        const int y0 = yt * 16, x0 = xt * 16;
        const int rows_here = (rh - y0) < 16 ? (rh - y0) : 16;
        const int nsteps = rows_here + s - 1;
        const u32 sbyte = (u32)(x0 + n_l + 16 * ((s <= 48 && q_l == 3) ? 0 : q_l));   // k-group 3: zero template columns
        const u32 sh = sbyte & 3u;
        const uint8_t *bp = win + y0 * wpitch + (sbyte & ~3u);
        // lane (m = n_l, g = q_l): template row i = step - m  ->  trow[g][16 + step - m]
        const uint8_t *ta = trow + (q_l * trows + 16 - n_l) * 16;
        const uint8_t *ta1 = trow1 + (q_l * trows + 16 - n_l) * 16;
        // even and odd steps accumulate separately: four independent MFMA chains instead of two
        v4i accT = {0, 0, 0, 0}, accS = {0, 0, 0, 0}, accT1 = {0, 0, 0, 0}, accS1 = {0, 0, 0, 0};
        // Software pipeline on running pointers: the LDS reads of step k+2 are issued before the MFMAs of
        // step k, three operand sets used in turn.  Five LDS instructions per step keep at most 15 reads in
        // flight - the lgkmcnt counter saturates at 15, beyond that the compiler must wait for everything.
        // S > 0: fixed trip count (a full 16-row tile), fully unrolled, so every wait names exactly the reads
        // of one step; a partial last tile runs the same steps against the zero rows behind the template
        // (kTrowPad).  Reads past the last step are never used.
        struct Ops { Raw5 w; v4i at, a1; };
        auto issue = [&]() {
            Ops o;
            o.w = read_raw(bp);
            o.at = *reinterpret_cast<const v4i *>(ta);
            o.a1 = *reinterpret_cast<const v4i *>(ta1);
            bp += wpitch; ta += 16; ta1 += 16;
            return o;
        };
        auto mma = [&](const Ops &o, v4i &aT, v4i &aS) {
            const v4i bb = align_raw(o.w, sh);
            aT = __builtin_amdgcn_mfma_i32_16x16x64_i8(o.at, bb, aT, 0, 0, 0);
            aS = __builtin_amdgcn_mfma_i32_16x16x64_i8(o.a1, bb, aS, 0, 0, 0);
        };
        Ops o0 = issue(), o1 = issue(), o2;
        constexpr int kStepsFixed = S > 0 ? 16 + S - 1 : 0;
        // six steps per trip (three operand sets x even / odd accumulators), leaving the loop after the last step
#define SID_WINNER_SIX(step, n)                                                                                        \
        o2 = issue(); __builtin_amdgcn_sched_barrier(0); mma(o0, accT, accS); __builtin_amdgcn_sched_barrier(0);      \
        if ((step) + 1 >= (n)) break;                                                                                  \
        o0 = issue(); __builtin_amdgcn_sched_barrier(0); mma(o1, accT1, accS1); __builtin_amdgcn_sched_barrier(0);    \
        if ((step) + 2 >= (n)) break;                                                                                  \
        o1 = issue(); __builtin_amdgcn_sched_barrier(0); mma(o2, accT, accS); __builtin_amdgcn_sched_barrier(0);      \
        if ((step) + 3 >= (n)) break;                                                                                  \
        o2 = issue(); __builtin_amdgcn_sched_barrier(0); mma(o0, accT1, accS1); __builtin_amdgcn_sched_barrier(0);    \
        if ((step) + 4 >= (n)) break;                                                                                  \
        o0 = issue(); __builtin_amdgcn_sched_barrier(0); mma(o1, accT, accS); __builtin_amdgcn_sched_barrier(0);      \
        if ((step) + 5 >= (n)) break;                                                                                  \
        o1 = issue(); __builtin_amdgcn_sched_barrier(0); mma(o2, accT1, accS1); __builtin_amdgcn_sched_barrier(0);
        if (S > 0) {
#pragma unroll
            for (int step = 0; step < kStepsFixed; step += 6) { SID_WINNER_SIX(step, kStepsFixed) }
        } else {
            for (int step = 0; step < nsteps; step += 6) { SID_WINNER_SIX(step, nsteps) }
        }
#undef SID_WINNER_SIX
        accT += accT1; accS += accS1;
        const int x = x0 + n_l;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int y = y0 + 4 * q_l + r;
            if (y < rh && x < rw)
                ccm[y * rw + x] = exact_from_sums(accT[r], accS[r], sii[y * rw + x], nd, sT, rT, cT);
        }
    }
    __syncthreads();
}

// BAND = 4: up to 768 threads, three wavefronts per SIMD (168 VGPRs).  BAND = 8: 256 threads, two per SIMD (the
// class whose LDS footprint admits two workgroups per CU anyway): an 8-row band halves the LDS bytes per MFMA.
template <int S, int BAND, bool PAIRED>
__global__ __launch_bounds__(BAND == 8 ? 512 : kMaxBlockM, BAND == 8 ? 2 : kOccM) void pm_kernel_mfma(const PMArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MiscM *m = reinterpret_cast<MiscM *>(smem);
    Geo *G = reinterpret_cast<Geo *>(smem + kGeoOff);
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // chained launch: this workgroup's arrival, counted once by lane 0 of the last wavefront and settled HERE, above every
    // return of the kernel - a workgroup that left uncounted would leave a stream waiting for ever
    if (A.chain.count != nullptr && tid == (int)blockDim.x - 64) chain_arrive(A.chain.count, A.chain.release, A.chain.epoch, A.n_launch);
    const int pt = A.order[blockIdx.x];
    const int s = S > 0 ? S : A.img_size, K = A.n_angles;

    double *out = A.out + (int64_t)pt * 5;
    int32_t *oij = A.out_ij ? A.out_ij + (int64_t)pt * 3 : nullptr;
#define SID_STAMP(k) do { if (A.dbg_cycles && tid == 0) A.dbg_cycles[k] = (long long)clock64(); } while (0)
    SID_STAMP(0);

    // ---- window geometry (pmlib.py:200-202) ----
    const double c2fg = A.c2fg[pt], r2fg = A.r2fg[pt], border = A.border[pt];
    const int hws = (int)((double)s / 2.0);
    const double r0d = r2fg - hws - border, r1d = r2fg + hws + border + 1;
    const double c0d = c2fg - hws - border, c1d = c2fg + hws + border + 1;
    const bool finite = fabs(r0d) < 1e15 && fabs(r1d) < 1e15 && fabs(c0d) < 1e15 && fabs(c1d) < 1e15;
    // (windows that NumPy slicing would clip at the bottom / right of image 2 never come here: pm_capi.hip classify_points sends
    // them to the large-window pipeline and debug_point refuses them - this kernel keeps rejecting them as a safety net)
    const int64_t r0 = finite ? (int64_t)r0d : -1, r1e = finite ? (int64_t)r1d : -1;
    const int64_t c0 = finite ? (int64_t)c0d : -1, c1e = finite ? (int64_t)c1d : -1;
    const bool inside = finite && r0 >= 0 && c0 >= 0 && r1e <= A.rows2 && c1e <= A.cols2 &&
                        r1e - r0 >= s + 1 && c1e - c0 >= s + 1;
    if (!inside) {
        if (tid < 5) out[tid] = NAN;
        if (oij && tid < 3) oij[tid] = -1;
        return;
    }
    const int wh = (int)(r1e - r0), ww = (int)(c1e - c0);
    const int rh = wh - s + 1, rw = ww - s + 1, npos = rh * rw;
    // the launch was sized by the host for the image shape it classified the points with (pm_capi.hip
    // classify_points); a window that needs more LDS than that must never be touched
    if (mfma_lds_layout(wh, ww, s, BAND, PAIRED).total > A.lds_bytes) {
        if (tid == 0 && A.refused) atomicAdd(A.refused, 1);            // an error the host reports (PMArgs::refused), never a silent NaN
        if (tid < 5) out[tid] = NAN;
        if (oij && tid < 3) oij[tid] = -1;
        return;
    }
    if (tid == 0) {
        const MfmaLdsLayout L = mfma_lds_layout(wh, ww, s, BAND, PAIRED);
        const double c1 = A.c1[pt], r1 = A.r1[pt];
        G->band = PAIRED ? 2 * BAND : BAND;
        G->wh = wh; G->ww = ww; G->rh = rh; G->rw = rw; G->npos = npos; G->wpitch = L.wpitch; G->arow = L.arow;
        G->gpitch = L.gpitch; G->arow0 = L.arow0; G->tab_rows = L.tab_rows; G->ones_slot = PAIRED ? 7 : 15;
        G->s = s; G->K = K;
        G->win_off = L.win_off; G->sii_off = L.sii_off; G->u_off = L.u_off; G->patch_off = L.patch_off;
        G->hes_off = L.sii_off; G->ccm_off = L.u_off + 2 * L.trow_bytes;   // (the sums' LDS holds the Hessian magnitudes later)
        G->ppitch = L.ppitch; G->pdim = L.pdim; G->pradius = L.pradius; G->queue_off = L.queue_off;
        G->trow_bytes = L.trow_bytes;
        G->pr0 = (int)floor(r1) - L.pradius; G->pc0 = (int)floor(c1) - L.pradius;
        G->win_magic = 0xffffffffu / (u32)((ww + 3) >> 2) + 1u; G->patch_magic = 0xffffffffu / (u32)(L.ppitch >> 2) + 1u;
        G->rw_magic = 0xffffffffu / (u32)rw + 1u;
        G->r0 = r0; G->c0 = c0; G->c1 = c1; G->r1 = r1; G->nd = (double)(s * s);
        G->hist_off = 0; G->lin = (int)((A.flags >> 3) & 7u); G->pre = A.pre ? (unsigned long long)(A.pre + (size_t)pt * K * s * s) : 0ull;
        m->zero_flag = 0; m->gmax_key = 0x007fffffu /* f2key(-inf) */; m->qcount = 0;
        for (int k = 0; k < 5; ++k) m->gw[k] = A.gauss_w[k];
    }
    __syncthreads();

    ph_window(A.img2, A.rows2, A.cols2, A.stride2);
    __syncthreads();
    SID_STAMP(1);
#ifndef SID_ABLATE_SUMS
    ph_sums();
#endif
    SID_STAMP(2);
    ph_patch(A.img1, A.rows1, A.cols1, A.stride1);

    // offset table for the samplers, or null: on-the-fly sampling (block-uniform)
    const uint16_t *samp = (A.samp && table_usable(*G, A.rows1, A.cols1)) ? A.samp : nullptr;
    Score sc{-INFINITY, -INFINITY, 0x7fffffff};
    for (int a0 = 0; a0 < K; a0 += kAnglesPerGroup) {
        const int Kg = (K - a0) < kAnglesPerGroup ? (K - a0) : kAnglesPerGroup;
        ph_tpl_begin<S>(A.rot, a0, Kg, A.dbg_cycles);
        if (samp) ph_tpl_table<S>(samp, a0, Kg, A.rows1, A.cols1);
        else ph_tpl_general<S>(a0, Kg, A.rows1, A.cols1);
        if (samp && A.samp_nflag > 0) ph_tpl_fix<S>(samp, a0, Kg, A.rows1, A.cols1, -1);
        ph_tpl_end<S>(a0, Kg, A.dbg_templates, A.dbg_cycles);
        if (m->zero_flag) {                                            // pmlib.py:152-154
            if (tid < 5) out[tid] = NAN;
            if (oij && tid < 3) oij[tid] = -1;
            if (A.dbg_shape && tid == 0) { A.dbg_shape[0] = rh; A.dbg_shape[1] = rw; }
            return;
        }
        SID_STAMP(3);
#ifndef SID_ABLATE_SWEEP
        sc = ph_sweep<S, BAND, PAIRED>(sc, a0, Kg, A.dbg_cycles);
#else
        sc.bestv = 0.5f; sc.bestkey = 17;
#endif
        SID_STAMP(4);
    }

    // ---- P3: block arg-max (first angle, then first row-major index on ties) ----
    {
        const float wbest = wave_max_dpp(sc.bestv);                    // exact values: never NaN
        sc.bestkey = wave_min_dpp(sc.bestv == wbest ? sc.bestkey : 0x7fffffff);
        sc.bestv = wbest;
    }
    if (lane == 0) { m->red_f[wv] = sc.bestv; m->red_i[wv] = sc.bestkey; }
    __syncthreads();
    if (tid == 0) {
        float bv = m->red_f[0]; int bk = m->red_i[0];
        for (int w = 1; w < kWavesM; ++w) {
            const float ov = m->red_f[w]; const int ok = m->red_i[w];
            if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
        }
        m->best_val = bv; m->best_key = bk;
    }
    __syncthreads();
    const float best_r = m->best_val;
    const int best_key = m->best_key;
    const int ka = best_key / npos;
    const int bidx = best_key - ka * npos;
    const int iy = bidx / rw, ix = bidx - iy * rw;
    SID_STAMP(5);

#ifndef SID_ABLATE_WINNER
    ph_winner_stage<S>(A.rot + 4 * ka, samp, A.rows1, A.cols1, ka);
    if (samp && A.samp_nflag > 0) ph_tpl_fix<S>(samp, 0, 0, A.rows1, A.cols1, ka);
    ph_winner<S>(ka, A.dbg_cycles);
#endif
    SID_STAMP(6);
    if (A.dbg_shape && tid == 0) { A.dbg_shape[0] = rh; A.dbg_shape[1] = rw; }
#ifndef SID_ABLATE_HESSIAN
    ph_hessian<>(A.flags, iy, ix, best_r, A.dbg_ccm, A.dbg_hes, A.dbg_cap, A.dbg_cycles);
#endif
    SID_STAMP(7);
    if (tid == 0) {
        double c2 = c2fg + ((double)ix - (double)(ww - s) / 2.0);
        double r2 = r2fg + ((double)iy - (double)(wh - s) / 2.0);
        if (A.flags & kSubpixel) { c2 += m->sub[0]; r2 += m->sub[1]; }
        out[0] = c2;
        out[1] = r2;
        out[2] = A.angles[ka];
        out[3] = (double)m->red_f[1];
        out[4] = (double)m->red_f[0];
        if (oij) { oij[0] = iy; oij[1] = ix; oij[2] = ka; }
    }
}
#undef SID_STAMP

// the instantiation of a row of SID_PM_CLASSIC_INSTANCES (side_arg: mfma_side_arg of the template side), nullptr: no such row
inline PmKernel classic_kernel(int side_arg, int band, bool paired)
{
#define SID_ROW(S, BAND, PAIRED) if (side_arg == S && band == BAND && paired == PAIRED) return pm_kernel_mfma<S, BAND, PAIRED>;
    SID_PM_CLASSIC_INSTANCES(SID_ROW)
#undef SID_ROW
    return nullptr;
}

}  // namespace

}  // namespace sid
