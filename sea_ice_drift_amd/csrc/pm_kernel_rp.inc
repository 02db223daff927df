// pm_kernel_rp.inc - the "row-pair" kernel for template sides 34 and 35: pm_kernel_rp<S, BAND, PAIRED, PITCH, BIG> and its own
// sums, operand, sweep and winner phases.  Needs pm_kernel_phases.h (the window / patch / Hessian phases, the sampler's helpers and
// the five-dword window fragment it shares with the classic kernel) and, through it, SID_PM_OCC.  Included by pm_kernel_mfma.hip
// (three wavefronts per SIMD) and pm_kernel_rp_occ4.hip (four).
//
// Why: the classic sweep multiplies one template row per MFMA - K = 64 window columns for a 34-column row, 47 %
// zeros - builds every window fragment from five ds_read_b32 (LDS-bound: 29 cycles per MFMA instead of 16) and
// scores every accumulator value in double precision (4.5 VALU instructions per MFMA).  Here
//
//   * K = 64 = two consecutive template rows x 32 columns:  A[slot][k] = T'_slot[i + (k >> 5)][k & 31],
//     B[k][x] = W'[rho + (k >> 5)][x + (k & 31)].  A band of 4 output rows y0 .. y0+3 walks the window two rows at a
//     time (rho = y0 + 2 j); even rows of the band use the row pairs (0,1), (2,3), ... ("E" operands), odd rows the
//     pairs (-1,0), (1,2), ... ("O" operands, rows -1 and s.. are zero), so one window fragment still feeds all
//     four rows of the band: 17.5 MFMAs per 16 placements and output row instead of 34;
//   * the remaining template columns 32.. ("strip") are multiplied through a transposed copy of the window columns 32..,
//     WT[v][rho] = W'[rho][32 + v]: K = 64 = 2 window columns x 32 rows (k-group g: column g & 1, rows 16 (g >> 1) ..),
//     the operand of a lane is 16 contiguous bytes of one WT row, and the four rows of a band are byte shifts 0 .. 3 of
//     one 20-byte read (rounds 2-3 kept column PAIRS, WP[u][rho] = (W'[rho][u], W'[rho][u + 1]): twice the LDS);
//   * a work item covers 32 adjacent placements as two interleaved MFMA tiles - tile A: x offsets {0-3, 8-11, 16-19,
//     24-27}, tile B: the same + 4 - so that lane (n, g) of BOTH tiles needs bytes of the same 8-aligned 24-byte
//     run: three ds_read_b64 (256 B/clk) + 8 v_alignbyte_b32 build two fragments (the classic form: 5 ds_read_b32 at
//     128 B/clk + 4 v_alignbyte_b32 for one); a leftover of at most 16 placements runs as a single classic tile;
//   * the arg-max pre-filter works in float32 on exactly re-centred integers: with m = round(S_T'/N) per slot,
//     numer / N = (acc - m Sw') - Sw' (S_T' - N m) / N, whose first term is an exact int32 and whose second is
//     below 2^17, so the float32 error of the estimate stays below 1e-6 for every window with N sigma_T sigma_I >=
//     4.5e3 (anything flatter goes straight to the exact path).  5 VALU instructions per value instead of ~24.
//
// Variants of the same code (template parameters of pm_kernel_rp / rp_sweep / rp_item_main):
//   BAND = 8    eight output rows per item, 256 VGPRs: the class that runs two workgroups of four wavefronts per CU;
//   PAIRED      slot groups for small angle sets.  1: at most 7 angles - slots 8..15 repeat the angles of slots 0..7 for
//               the output rows four further down (operand address lagging two row pairs), i.e. eight output rows per item
//               in the 4-row form's registers.  2: at most 3 angles (the reference's default, pmlib.py:118) - four groups
//               of 3 angles + ones, group g working 4 g output rows down: sixteen output rows per item.
//
// The exact evaluation of the candidates (exact_from_sums) and the Hessian are those of the classic kernel; the NCC
// matrix of the winning angle has a row-pair form of its own (rp_winner).  The integers are the same everywhere, so
// the results are bit-identical.

#pragma once
#include "pm_kernel_phases.h"

namespace sid {

namespace {

// Wave priorities by phase (s_setprio).  The short phases between the barriers of a workgroup are latency chains; the sweep
// is throughput work that can fill whatever issue slots the other workgroups of the CU leave.  With the phases before the
// sweep and the arg-max at priority 3, the Hessian at 2, the winner's matrix at 1 and the sweep at 0 the 15-angle step is
// 1.7 % faster (same box: 4.267 -> 4.195 ms; border 20 -1.9 %, s = 35 -2.6 %, border 50 unchanged); the other way round
// (sweep high) +0.7 %.  The slot-group kernels (<= 7 angles: little sweep per point) gain nothing from it (7 angles +-0,
// 3 angles +0.9 %) and keep one priority.  SID_P_*: the priorities of the full-table kernels (-D, A/B builds); SID_Q_*: of
// the slot-group kernels.
#ifndef SID_P_PRE
#define SID_P_PRE 3
#define SID_P_SWEEP 0
#define SID_P_POST 3
#define SID_P_WIN 1
#define SID_P_HES 2
#endif
#ifndef SID_Q_PRE
#define SID_Q_PRE 0
#define SID_Q_SWEEP 0
#define SID_Q_POST 0
#define SID_Q_WIN 0
#define SID_Q_HES 0
#endif
// Set inside the NON-INLINED phase functions where a phase boundary coincides with one (round 4): s_setprio has side effects
// the register allocator must respect, and in the kernel body - around the sweep, whose loop needs all 168 VGPRs - three of them
// cost three 8-byte spills per lane (a scratch store each per point: 60 of the 93 MB the largest launch wrote per step).  The
// sweep's priority is set at the end of rp_tpl_end, the winner's at the start of rp_winner_stage_tab; the arg-max between them
// runs at the sweep's priority.  TS = 9: full operand table (the kernels that use priorities).
#define SID_SETPRIO_TS(phase) do { if (TS == 9 && ((SID_P_PRE) | (SID_P_SWEEP) | (SID_P_POST) | (SID_P_WIN) | (SID_P_HES))) __builtin_amdgcn_s_setprio(SID_P_##phase); } while (0)
#define SID_SETPRIO(phase) do { \
    if (PAIRED == 0 && ((SID_P_PRE) | (SID_P_SWEEP) | (SID_P_POST) | (SID_P_WIN) | (SID_P_HES))) __builtin_amdgcn_s_setprio(SID_P_##phase); \
    if (PAIRED != 0 && ((SID_Q_PRE) | (SID_Q_SWEEP) | (SID_Q_POST) | (SID_Q_WIN) | (SID_Q_HES))) __builtin_amdgcn_s_setprio(SID_Q_##phase); } while (0)

// Kept accumulators (PMArgs::gs_keep_acc) are compiled into the slot-group kernels only: the full-table kernels would carry the
// stores and the second winner through their 168 registers for a launch flag that is off by default
// (tools/patches/keep_acc_full.patch compiled them into every gs instantiation: +12 %, DESIGN.md section 5.2).

struct Raw6 { u32 d[6]; };
// 24 bytes at an 8-aligned LDS offset as three ds_read_b64.  The three offsets (o, o + 8, o + 16) are kept in
// separate registers that the compiler cannot relate (Off3::make launders two of them): it would otherwise merge
// neighbours into ds_read2_b64, which moves 128 B/clk instead of 256.
struct Off3 {
    u32 o0, o1, o2;
    static __device__ __forceinline__ Off3 make(u32 o)
    {
        Off3 r; r.o0 = o; r.o1 = o + 8; r.o2 = o + 16;
        asm("" : "+v"(r.o1)); asm("" : "+v"(r.o2));
        return r;
    }
    __device__ __forceinline__ void advance(u32 d) { o0 += d; o1 += d; o2 += d; }
    __device__ __forceinline__ Off3 plus(u32 d) const { Off3 r; r.o0 = o0 + d; r.o1 = o1 + d; r.o2 = o2 + d; return r; }
};
__device__ __forceinline__ Raw6 read_raw6(const Off3 &p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint2 a = *reinterpret_cast<const uint2 *>(smem + p.o0), b = *reinterpret_cast<const uint2 *>(smem + p.o1),
                c = *reinterpret_cast<const uint2 *>(smem + p.o2);
    Raw6 w;
    w.d[0] = a.x; w.d[1] = a.y; w.d[2] = b.x; w.d[3] = b.y; w.d[4] = c.x; w.d[5] = c.y;
    return w;
}
// The five dwords of a single tile's window fragment as five ds_read_b32 on five address registers the compiler cannot relate:
// every step's offset is then a 16-bit immediate of its instruction.  Read as consecutive dwords of ONE address the compiler
// pairs them into ds_read2_b32, whose two 8-bit offsets (1020 bytes) do not reach a step's row: two v_add_u32 per step in a
// VALU-bound loop (round 5; 38 per single item).
struct Off5 {
    u32 o[5];
    static __device__ __forceinline__ Off5 make(u32 b)
    {
        Off5 r;
#pragma unroll
        for (int i = 0; i < 5; ++i) { r.o[i] = b + 4u * (u32)i; if (i) asm("" : "+v"(r.o[i])); }
        return r;
    }
    __device__ __forceinline__ void advance(u32 d) {
#pragma unroll
        for (int i = 0; i < 5; ++i) o[i] += d;
    }
};
__device__ __forceinline__ Raw5 read_raw5(const Off5 &p, u32 d)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Raw5 w;
#pragma unroll
    for (int i = 0; i < 5; ++i) w.r[i] = *reinterpret_cast<const u32 *>(smem + p.o[i] + d);
    return w;
}
// 32 bytes (four ds_read_b64) for the strip of an 8-row band
struct Raw8 { u32 d[8]; };
__device__ __forceinline__ Raw8 read_raw8(u32 o)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32 o1 = o + 8, o2 = o + 16, o3 = o + 24;
    asm("" : "+v"(o1)); asm("" : "+v"(o2)); asm("" : "+v"(o3));
    const uint2 a = *reinterpret_cast<const uint2 *>(smem + o), b = *reinterpret_cast<const uint2 *>(smem + o1),
                c = *reinterpret_cast<const uint2 *>(smem + o2), d = *reinterpret_cast<const uint2 *>(smem + o3);
    Raw8 w;
    w.d[0] = a.x; w.d[1] = a.y; w.d[2] = b.x; w.d[3] = b.y; w.d[4] = c.x; w.d[5] = c.y; w.d[6] = d.x; w.d[7] = d.y;
    return w;
}
// b in the lanes of `mask` (a wavefront-uniform constant), a elsewhere: one v_cndmask_b32 on a scalar mask
__device__ __forceinline__ int sel_lanes(int a, int b, unsigned long long mask)
{
    int o;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "s"(mask));
    return o;
}
template <int FIRST>
__device__ __forceinline__ v4i align_raw6(const Raw6 &w, u32 sh)
{
    v4i b;
    b[0] = (int)__builtin_amdgcn_alignbyte(w.d[FIRST + 1], w.d[FIRST + 0], sh);
    b[1] = (int)__builtin_amdgcn_alignbyte(w.d[FIRST + 2], w.d[FIRST + 1], sh);
    b[2] = (int)__builtin_amdgcn_alignbyte(w.d[FIRST + 3], w.d[FIRST + 2], sh);
    b[3] = (int)__builtin_amdgcn_alignbyte(w.d[FIRST + 4], w.d[FIRST + 3], sh);
    return b;
}

// slot groups of a PAIRED mode (0: one group of 16 slots, 1: two groups of 8, 2: four groups of 4)
__host__ __device__ constexpr int rp_ngroups(int paired) { return paired == 2 ? 4 : paired == 1 ? 2 : 1; }

template <int S, int BAND = 4>
struct RpShape {
    static constexpr int nE = (S + 1) / 2;          // pairs (2p, 2p+1), p = 0 .. nE-1
    static constexpr int nO = S / 2 + 1;            // pairs (2p-1, 2p), p = 0 .. nO-1
    // steps j = 0 .. NS-1 (window rows y0 + 2j, y0 + 2j + 1); output row t of the band uses pair j - (t >> 1)
    static constexpr int NS = (nE > nO ? nE : nO) + BAND / 2 - 1;
    static constexpr int ncp = (S - 32 + 1) / 2;    // strip column pairs
    static constexpr int nrg = 2;                   // strip row groups of 32 template rows
};

// byte offset (from the LDS base) of template sample (row i, column j) of slot a in the row-pair operands
// TS: log2 of the bytes per operand-table row (rp_tab_pitch; a template parameter of everything that touches the table)
template <int TS, typename GeoT>
__device__ __forceinline__ int rp_off(const GeoT &G, int i, int j, int a)
{
    if (j < 32) return G.u_off + ((i + 1) << TS) + a * 32 + j;
    // strip fragment (column pair c >> 1, row group i >> 5): lane 16 g + a with g = 2 ((i & 31) >> 4) + (c & 1), byte i & 15
    const int c = j - 32;
    return G.strip_off + ((((c >> 1) << 1) + (i >> 5)) << 10) + (((((((i & 31) >> 4) << 1) + (c & 1)) << 4) + a) << 4) + (i & 15);
}

// Entry `idx` of a point's sum w'^2 values through a 32-bit BYTE offset: with the values in global memory the access is then
// "scalar base + 32-bit lane offset" (one shift) instead of a 64-bit address per lane (idx * 4 cannot be proven to fit 32 bits
// by the compiler; it does: a point has fewer than 2^16 placements)
__device__ __forceinline__ u32 sii_at(const u32 *base, int idx)
{
    return *reinterpret_cast<const u32 *>(reinterpret_cast<const unsigned char *>(base) + ((u32)idx << 2));
}
__device__ __forceinline__ void sii_put(u32 *base, int idx, u32 v)
{
    *reinterpret_cast<u32 *>(reinterpret_cast<unsigned char *>(base) + ((u32)idx << 2)) = v;
}

// ---------------------------------------------------------------------------------------------
// S_II' = box sums of w'^2: running sums along the rows into LDS, then down the columns into `out` - LDS (sii_off) or, in
// the gs instantiations, GLOBAL memory (PMArgs::gsii).  The second pass has one thread per column pair and run of rows, so
// the lanes of a wavefront write consecutive placements: coalesced stores.  The global values are read back by this workgroup
// only (scoring of the sweep, the winner's matrix), from L2.  In LDS they are the largest item of a point with a large border
// (42 KB at border 50) and what decides the residency class of most borders above 27 (rp_lds_layout).
//
// Both passes work on tasks of a COMPILE-TIME length (straight-line code, every LDS offset an immediate or one scalar
// multiple of the row pitch): a task fetches everything it needs with wide reads issued up front, then works in registers -
// no output waits on an LDS round trip of its own (the form of rounds 2-7 read two bytes, or two dwords, per output and
// waited for them: ~21 dependent round trips per thread and pass at border 20).
//   rows:    task = (window row y, SEG placements from x = SEG seg, SEG a multiple of 8): SEG + s - 1 bytes as ds_read_b64,
//            the first sum as v_dot4_i32_i8 of whole dwords, then one square in and one out per placement.  The last segment
//            of a row may hang over rw: it reads on into bytes the window phase wrote (zeros, the next rows - the window
//            has three rows or more below its last) and stores under a mask; tasks are numbered segment by segment, so
//            that only the wavefronts of the last segment run the masked stores.
//   columns: task = (placement columns x, x + 1; SEGR output rows).  The last segment of a column is pulled up so that it
//            ends on the last output row, and the last pair of an odd rw back by one column (both recompute values another
//            task stores as well: the same integers), so no read leaves the rh + s - 1 = wh rows of row sums and no
//            store needs a mask.
// The lengths are chosen per point (wavefront-uniform) as those that issue the fewest wavefront-instructions: whole
// wavefronts of tasks x instructions per task.  The kernels are bound by instruction issue (DESIGN.md section 5.1), so a
// long task in one wavefront beats short tasks in all of them, whose first sums - s terms for every segment - repeat.
// ---------------------------------------------------------------------------------------------
template <int S, int SEG>
__device__ __forceinline__ void rp_sums_row_task(const uint8_t *src, u32 *dst, int nvalid)
{
    static_assert(SEG % 8 == 0 && SEG + S - 1 <= 72, "segments start on 8-byte boundaries; 18 dwords per task at most");
    constexpr int NQ = (SEG + S - 1 + 7) / 8;
    u32 d[2 * NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { const uint2 t = reinterpret_cast<const uint2 *>(src)[q]; d[2 * q] = t.x; d[2 * q + 1] = t.y; }
    int c = 0;
#pragma unroll
    for (int j = 0; j < S / 4; ++j) c = __builtin_amdgcn_sdot4((int)d[j], (int)d[j], c, false);
    if (S & 3) { const int t = (int)(d[S / 4] & ((1u << (8 * (S & 3))) - 1u)); c = __builtin_amdgcn_sdot4(t, t, c, false); }
    u32 o[SEG];
    o[0] = (u32)c;
#pragma unroll
    for (int k = 1; k < SEG; ++k) {                                    // (k is a constant after unrolling: v_bfe_i32 / SDWA selects)
        const int bi = k + S - 1, bo = k - 1;
        const int vi = (int)(d[bi >> 2] << (24 - 8 * (bi & 3))) >> 24, vo = (int)(d[bo >> 2] << (24 - 8 * (bo & 3))) >> 24;
        c += vi * vi - vo * vo;
        o[k] = (u32)c;
    }
    if (nvalid >= SEG) {
#pragma unroll
        for (int k = 0; k < SEG; ++k) dst[k] = o[k];
    } else {
#pragma unroll
        for (int k = 0; k < SEG; ++k) if (k < nvalid) dst[k] = o[k];
    }
}

template <int S, int SEG>
__device__ __forceinline__ void rp_sums_rows(const uint8_t *win, u32 *rowsum, int wh, int rw, int wpitch)
{
    const int tid = threadIdx.x;
    const int nseg = (rw + SEG - 1) / SEG, ntask = wh * nseg;
    const u32 magic = 0xffffffffu / (u32)wh + 1u;                      // task / wh == umulhi(task, magic): task < 2^16
    for (int task = tid; task < ntask; task += kBlockM) {
        const int seg = (int)__umulhi((u32)task, magic), y = task - seg * wh, xa = seg * SEG;
        rp_sums_row_task<S, SEG>(win + y * wpitch + xa, rowsum + y * rw + xa, rw - xa);
    }
}

template <int S, int SEGR, bool GS>
__device__ __forceinline__ void rp_sums_col_task(const u32 *col, int rw, u32 *gs, int o0)
{
    // rows 0 .. SEGR-2 leave the running sum, rows S .. S+SEGR-2 enter it; the rows between are only part of the first sum
    u32 a0 = 0, a1 = 0, out0[SEGR > 1 ? SEGR - 1 : 1], out1[SEGR > 1 ? SEGR - 1 : 1], in0[SEGR > 1 ? SEGR - 1 : 1], in1[SEGR > 1 ? SEGR - 1 : 1];
#pragma unroll
    for (int i = 0; i < S + SEGR - 1; ++i) {
        const u32 v0 = col[i * rw], v1 = col[i * rw + 1];
        if (i < S) { a0 += v0; a1 += v1; }
        if (i < SEGR - 1) { out0[i] = v0; out1[i] = v1; }
        if (i >= S) { in0[i - S] = v0; in1[i - S] = v1; }
    }
    static_assert(SEGR - 1 <= S, "a row leaves the sum or enters it, not both");
    u32 r0[SEGR], r1[SEGR];
    r0[0] = a0; r1[0] = a1;
#pragma unroll
    for (int k = 1; k < SEGR; ++k) {
        a0 += in0[k - 1] - out0[k - 1]; a1 += in1[k - 1] - out1[k - 1];
        r0[k] = a0; r1[k] = a1;
    }
#pragma unroll
    for (int k = 0; k < SEGR; ++k) { sii_put(gs, o0 + k * rw, r0[k]); sii_put(gs, o0 + k * rw + 1, r1[k]); }
}

template <int S, int SEGR, bool GS>
__device__ __forceinline__ void rp_sums_cols(const u32 *rowsum, u32 *gs, int rh, int rw)
{
    const int tid = threadIdx.x;
    const int npr = (rw + 1) >> 1, nseg = (rh + SEGR - 1) / SEGR, ntask = npr * nseg;
    const u32 magic = 0xffffffffu / (u32)npr + 1u;
    for (int task = tid; task < ntask; task += kBlockM) {
        const int seg = npr > 1 ? (int)__umulhi((u32)task, magic) : task, pr = task - seg * npr;   // (one column pair - a matrix two wide -: 2^32 / 1 + 1 is no 32-bit magic)
        const int x = 2 * pr < rw - 2 ? 2 * pr : rw - 2, ya = seg * SEGR < rh - SEGR ? seg * SEGR : rh - SEGR;
        rp_sums_col_task<S, SEGR, GS>(rowsum + ya * rw + x, rw, gs, ya * rw + x);
    }
}

// wavefront-instructions of a pass: whole wavefronts of tasks x instructions per task (static counts of the task bodies)
// (the other rule - the longest chain of a thread - is tools/patches/sums_by_rounds.patch)
#define SID_SUMS_GROUPS(tasks) (((tasks) + 63) >> 6)
__device__ __forceinline__ int rp_sums_row_cost(int wh, int rw, int seg) { return SID_SUMS_GROUPS(wh * ((rw + seg - 1) / seg)) * (5 * seg + 24); }
__device__ __forceinline__ int rp_sums_col_cost(int rh, int rw, int s, int segr)
{
    return SID_SUMS_GROUPS(((rw + 1) >> 1) * ((rh + segr - 1) / segr)) * (2 * (s + segr - 1) + 2 * s + 6 * segr + 12);
}

template <int S, bool GS, bool BIG = false>
__device__ __noinline__ void rp_sums(u32 *gsout)
{
    SID_PHASE_LOCALS;
    u32 *gs = GS ? gsout : reinterpret_cast<u32 *>(smem + G.sii_off);
    const uint8_t *win = smem + G.win_off;
    u32 *rowsum = tab_ptr<BIG, u32>(G, smem, BIG ? G.ccm_off : G.u_off);   // (big layouts: where the NCC matrix will be)
    // (wavefront-uniform: scalar registers, scalar branches)
    const int wh = __builtin_amdgcn_readfirstlane(G.wh), rh = __builtin_amdgcn_readfirstlane(G.rh), rw = __builtin_amdgcn_readfirstlane(G.rw);
    const int wpitch = __builtin_amdgcn_readfirstlane(G.wpitch);
    {   // along the rows
        int seg = 8, best = rp_sums_row_cost(wh, rw, 8);
        for (int c = 16; c <= 32; c += 8) { const int v = rp_sums_row_cost(wh, rw, c); if (v < best) { best = v; seg = c; } }
        if (seg == 8) rp_sums_rows<S, 8>(win, rowsum, wh, rw, wpitch);
        else if (seg == 16) rp_sums_rows<S, 16>(win, rowsum, wh, rw, wpitch);
        else if (seg == 24) rp_sums_rows<S, 24>(win, rowsum, wh, rw, wpitch);
        else rp_sums_rows<S, 32>(win, rowsum, wh, rw, wpitch);
    }
    __syncthreads();
    {   // down the columns (rh >= 2: the kernel refuses windows below s + 1 rows)
        int segr = 2, best = rp_sums_col_cost(rh, rw, S, 2);
        for (int c = 4; c <= 16 && c <= rh; c += c) { const int v = rp_sums_col_cost(rh, rw, S, c); if (v < best) { best = v; segr = c; } }
        if (segr == 2) rp_sums_cols<S, 2, GS>(rowsum, gs, rh, rw);
        else if (segr == 4) rp_sums_cols<S, 4, GS>(rowsum, gs, rh, rw);
        else if (segr == 8) rp_sums_cols<S, 8, GS>(rowsum, gs, rh, rw);
        else rp_sums_cols<S, 16, GS>(rowsum, gs, rh, rw);
    }
    __syncthreads();                                                   // the row sums are dead; the stores are visible to the workgroup
}

// ---------------------------------------------------------------------------------------------
// transposed copy of the window columns 32.. for the strip: WT[v][rho] = W'[rho][32 + v]
// ---------------------------------------------------------------------------------------------
// Built by the wavefronts 1.. of the workgroup inside rp_tpl_end (first angle group), while wavefront 0 forms the per-slot
// terms: the image-1 patch is dead by then (one group of angles), so the copy - like the candidate queue - lies over it.
__device__ __forceinline__ void rp_wt_build(int t0, int nthr)
{
    SID_PHASE_LOCALS;
    const uint8_t *win = smem + G.win_off;
    uint8_t *wt = smem + G.wp_off;
    const int wpitch = G.wpitch, pw = G.wp_pitch, nd = G.wp_pitch >> 2, wrows = G.wrows, ngv = (G.wp_rows + 3) >> 2;
    // one task = a 4 x 4 byte block: window rows rho .. rho + 3 (zero beyond the rows the window phase wrote), window
    // columns 32 + v0 .. + 3 (dword-aligned), transposed in registers (v_perm) and stored as one dword in each of the
    // WT rows v0 .. v0 + 3
    const u32 magic = 0xffffffffu / (u32)nd + 1u;
    const int nrows = G.wp_rows;
    for (int idx = t0; idx < ngv * nd; idx += nthr) {
        const int gv = (int)__umulhi((u32)idx, magic), d = idx - gv * nd;
        const int rho = 4 * d, v0 = 4 * gv;
        const u32 *p = reinterpret_cast<const u32 *>(win + rho * wpitch + 32 + v0);
        const int pd = wpitch >> 2;
        const u32 r0 = rho < wrows ? p[0] : 0u, r1 = rho + 1 < wrows ? p[pd] : 0u;
        const u32 r2 = rho + 2 < wrows ? p[2 * pd] : 0u, r3 = rho + 3 < wrows ? p[3 * pd] : 0u;
        // bytes (r0.k, r1.k, r2.k, r3.k) -> dword k
        const u32 a01 = __builtin_amdgcn_perm(r1, r0, 0x05010400u), b01 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);   // (r0.0 r1.0 r0.1 r1.1), (r0.2 r1.2 r0.3 r1.3)
        const u32 a23 = __builtin_amdgcn_perm(r3, r2, 0x05010400u), b23 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
        uint8_t *q = wt + v0 * pw + 4 * d;
        *reinterpret_cast<u32 *>(q) = __builtin_amdgcn_perm(a23, a01, 0x05040100u);            // column v0: r0.0 r1.0 r2.0 r3.0
        if (v0 + 1 < nrows) *reinterpret_cast<u32 *>(q + pw) = __builtin_amdgcn_perm(a23, a01, 0x07060302u);       // column v0 + 1
        if (v0 + 2 < nrows) *reinterpret_cast<u32 *>(q + 2 * pw) = __builtin_amdgcn_perm(b23, b01, 0x05040100u);
        if (v0 + 3 < nrows) *reinterpret_cast<u32 *>(q + 3 * pw) = __builtin_amdgcn_perm(b23, b01, 0x07060302u);
    }
}

// ---------------------------------------------------------------------------------------------
// template operands of one group of <= 15 angles in the row-pair layout
// ---------------------------------------------------------------------------------------------
template <int S, int TS>
__device__ __noinline__ void rp_tpl_begin(const double *rot, int a0, int Kg, long long *dbg_cycles)
{
    SID_PHASE_LOCALS;
    uint8_t *tab = smem + G.u_off;
    if (tid < 4 * Kg) (&m->rot[0][0])[tid] = rot[4 * a0 + tid];
    const int nz = ((G.tab_rows << TS) + RpShape<S>::ncp * RpShape<S>::nrg * 1024 + 16) / 16;   // table + strip + scratch
    for (int idx = tid; idx < nz; idx += kBlockM) reinterpret_cast<uint4 *>(tab)[idx] = make_uint4(0, 0, 0, 0);
    if (tid < kSlots) { m->isT[tid] = 0; m->isTT[tid] = 0; }
    __syncthreads();                                                   // also: patch complete
    if (dbg_cycles && tid == 0) dbg_cycles[8] = (long long)clock64();
}

template <int S, int TS>
__device__ __noinline__ void rp_tpl_table(const uint16_t *samp, int a0, int Kg)
{
    SID_PHASE_LOCALS;
    const uint8_t *patch = smem + G.patch_off;
    constexpr int s = S;
    int sawzero = 0;
    // (the table offsets by VALUE: read through the reference into LDS, every store of the loop below makes the compiler
    // fetch u_off / strip_off again - fifteen dependent LDS round trips per angle in round 4's code)
    struct { int u_off, strip_off; } GO{G.u_off, G.strip_off};
    const int sp = samp_pitch(s), nq = sp >> 2, upa = s * nq;
    const u32 tailmask = (s & 3) ? (1u << (8 * (s & 3))) - 1u : 0xffffffffu;
    constexpr int kCh = (S * ((S + 3) / 4) + 63) / 64;
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
            const bool more = u0 + 64 * kCh < upa;
            if (more) fetch(a, u0 + 64 * kCh, nxt);
            else if (a + kWavesM < Kg) fetch(a + kWavesM, 0, nxt);
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
                    zero |= (z - 0x01010101u) & ~z & 0x80808080u;      // some valid byte == 0
                    sv = __builtin_amdgcn_udot4(raw, 0x01010101u, sv, false);
                    svv = __builtin_amdgcn_udot4(raw, raw, svv, false);
                    const u32 v = (raw ^ 0x80808080u) & vm;
                    if (jq < 8) {
                        *reinterpret_cast<u32 *>(smem + GO.u_off + ((i + 1) << TS) + a * 32 + jq * 4) = v;
                    } else {                                           // strip columns 32, 33 (, 34)
                        smem[rp_off<TS>(GO, i, 32, a)] = (uint8_t)v;
                        smem[rp_off<TS>(GO, i, 33, a)] = (uint8_t)(v >> 8);
                        if (S > 34) smem[rp_off<TS>(GO, i, 34, a)] = (uint8_t)(v >> 16);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < kCh; ++c) cur[c] = nxt[c];
        }
        const int ws = wave_sum_dpp((int)sv), wss = wave_sum_dpp((int)svv);
        if (lane == 0) { m->isT[a] = ws - 128 * s * s; m->isTT[a] = wss - 256 * ws + 16384 * s * s; }
        sawzero |= zero != 0u ? 1 : 0;
    }
    if (sawzero) m->zero_flag = 1;
}

// The same through the SORTED table (PMArgs::samp2, round 5): run records - four consecutive patch bytes: two aligned dwords
// and a v_alignbyte - then gather records.  The records of a wavefront's NEXT angle are fetched while it works on the current
// one (one global round trip per angle otherwise: the phase is a latency chain).
template <int S, int TS>
__device__ __noinline__ void rp_tpl_table2(const u32 *samp2, int a0, int Kg)
{
    SID_PHASE_LOCALS;
    const uint8_t *patch = smem + G.patch_off;
    constexpr int s = S, sp = (S + 3) / 4 * 4, nq = sp >> 2;
    constexpr int kCh = kSamp2Cap / 64;
    const int u_off = G.u_off, strip_off = G.strip_off;                // (by value: see rp_tpl_table)
    struct { int u_off, strip_off; } GO{u_off, strip_off};
    const u32 tailmask = (s & 3) ? (1u << (8 * (s & 3))) - 1u : 0xffffffffu;
    int sawzero = 0;
    struct Recs { u32 run[kCh]; uint2 gat[kCh]; u32 gid[kCh]; int nrun, ngat; };
    auto fetch = [&](int a, Recs &r) {
        const u32 *blk = samp2 + (size_t)(a0 + a) * kSamp2Words;
        r.nrun = __builtin_amdgcn_readfirstlane((int)blk[0]); r.ngat = __builtin_amdgcn_readfirstlane((int)blk[1]);
        const uint16_t *ids = reinterpret_cast<const uint16_t *>(blk + kSamp2Id);
#pragma unroll
        for (int c = 0; c < kCh; ++c) {
            const int u = 64 * c + lane;
            r.run[c] = blk[kSamp2Run + u];
            r.gat[c] = reinterpret_cast<const uint2 *>(blk + kSamp2Gat)[u];
            r.gid[c] = ids[u];
        }
    };
    Recs cur = {}, nxt = {};
    if (wv < Kg) fetch(wv, cur);
    for (int a = wv; a < Kg; a += kWavesM) {
        if (a + kWavesM < Kg) fetch(a + kWavesM, nxt);
        u32 sv = 0, svv = 0, zero = 0;
#pragma unroll
        for (int c = 0; c < kCh; ++c) {                                // runs
            if (64 * c < cur.nrun) {                                   // wavefront-uniform
                const u32 rec = cur.run[c];
                const u32 *src = reinterpret_cast<const u32 *>(patch + (rec & 0x7ffcu));
                const u32 raw = __builtin_amdgcn_alignbyte(src[1], src[0], (rec >> 15) & 3u);
                if (64 * c + lane < cur.nrun) {
                    zero |= (raw - 0x01010101u) & ~raw & 0x80808080u;  // some byte == 0
                    sv = __builtin_amdgcn_udot4(raw, 0x01010101u, sv, false);
                    svv = __builtin_amdgcn_udot4(raw, raw, svv, false);
                    const u32 i = (rec >> 17) & 63u, jq = (rec >> 23) & 15u;
                    *reinterpret_cast<u32 *>(smem + u_off + ((i + 1u) << TS) + a * 32 + jq * 4u) = raw ^ 0x80808080u;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < kCh; ++c) {                                // gathers (as rp_tpl_table)
            if (64 * c < cur.ngat) {
                const u32 rawv = gather_quad(patch, cur.gat[c]);
                if (64 * c + lane < cur.ngat) {
                    const int u = (int)cur.gid[c];
                    const int i = u / nq, jq = u - i * nq;
                    const u32 vm = jq == nq - 1 ? tailmask : 0xffffffffu;
                    const u32 raw = rawv & vm;
                    const u32 z = raw | ~vm;
                    zero |= (z - 0x01010101u) & ~z & 0x80808080u;
                    sv = __builtin_amdgcn_udot4(raw, 0x01010101u, sv, false);
                    svv = __builtin_amdgcn_udot4(raw, raw, svv, false);
                    const u32 v = (raw ^ 0x80808080u) & vm;
                    if (jq < 8) {
                        *reinterpret_cast<u32 *>(smem + u_off + ((i + 1) << TS) + a * 32 + jq * 4) = v;
                    } else {                                           // strip columns 32, 33 (, 34)
                        smem[rp_off<TS>(GO, i, 32, a)] = (uint8_t)v;
                        smem[rp_off<TS>(GO, i, 33, a)] = (uint8_t)(v >> 8);
                        if (S > 34) smem[rp_off<TS>(GO, i, 34, a)] = (uint8_t)(v >> 16);
                    }
                }
            }
        }
        const int ws = wave_sum_dpp((int)sv), wss = wave_sum_dpp((int)svv);
        if (lane == 0) { m->isT[a] = ws - 128 * s * s; m->isTT[a] = wss - 256 * ws + 16384 * s * s; }
        sawzero |= zero != 0u ? 1 : 0;
        cur = nxt;
    }
    if (sawzero) m->zero_flag = 1;
}

// general sampler (non-integral centre, or the patch touches the image border).  One angle at a time: the classic
// kernel's form keeps three angles in flight, which in this kernel spilled some forty 64-bit lane masks into VGPR
// lanes and produced - only with three workgroups per CU - wrong samples in lanes 48..63 of a wavefront about once
// in 10^4 points (DESIGN.md section 6b); this path is rare (the reference rounds the centres before the dispatch),
// so it is kept simple.
template <int S, int TS>
__device__ __noinline__ void rp_tpl_general(int a0, int Kg, long long rows1, long long cols1)
{
    SID_PHASE_LOCALS;
    const uint8_t *patch = smem + G.patch_off;
    constexpr int s = S;
    const SampleGeom g = sample_geom(G, s, rows1, cols1, patch);
    int sawzero = 0;
    auto run = [&](auto inside_tag) {
        constexpr bool INSIDE = decltype(inside_tag)::value;
        for (int k0 = 0; k0 * g.ngrp < s; k0 += kRowsPerThread) {
            for (int aa = 0; aa < Kg; ++aa) {
                int st = 0, stt = 0;
                const u32 db = sample_fast5<INSIDE>(g, m->rot[aa], true, k0, st, stt, sawzero,
                    [&](int, int i, int v, bool take) { if (take) smem[rp_off<TS>(G, i, g.j, aa)] = (uint8_t)(v ^ 0x80); });
                // the doubtful samples (coordinate within kGuard of a rounding or image boundary): scipy's double arithmetic
                for (int u = 0; u < kRowsPerThread; ++u) {
                    if ((db >> u) & 1u) {
                        const int i = g.ig + (k0 + u) * g.ngrp;
                        const int v = sample_exact(g, m->rot[aa], i, g.j, a0 + aa);
                        sawzero |= (v == 0) ? 1 : 0;
                        smem[rp_off<TS>(G, i, g.j, aa)] = (uint8_t)(v ^ 0x80);
                        st += v - 128; stt += (v - 128) * (v - 128);
                    }
                }
                const int ws = wave_sum_dpp(st), wss = wave_sum_dpp(stt);       // (all lanes active here)
                if (lane == 0) { atomicAdd(&m->isT[aa], ws); atomicAdd(&m->isTT[aa], wss); }
            }
        }
    };
    if (g.inside) run(std::true_type{}); else run(std::false_type{});
    if (sawzero) m->zero_flag = 1;
}

// flagged table entries of the group, recomputed in float64 (rare)
template <int S, int TS>
__device__ __noinline__ void rp_tpl_fix(const uint16_t *samp, int a0, int Kg, long long rows1, long long cols1)
{
    SID_PHASE_LOCALS;
    __syncthreads();
    const uint8_t *patch = smem + G.patch_off;
    constexpr int s = S;
    const int sp = samp_pitch(s);
    const SampleGeom g = sample_geom(G, s, rows1, cols1, patch);
    for (int idx = tid; idx < Kg * s * sp; idx += kBlockM) {
        const int a = idx / (s * sp), rem = idx - a * s * sp;
        const int i = rem / sp, j = rem - i * sp;
        if (j >= s || !(samp[(size_t)(a0 + a) * s * sp + rem] & 0x8000u)) continue;
        const int v = sample_exact(g, m->rot[a], i, j, -1);             // (table path: never with pre-sampled templates)
        smem[rp_off<TS>(G, i, j, a)] = (uint8_t)(v ^ 0x80);
        atomicAdd(&m->isT[a], v - 128); atomicAdd(&m->isTT[a], (v - 128) * (v - 128));
        if (v == 0) m->zero_flag = 1;
    }
}

template <int S, int TS>
__device__ __noinline__ void rp_tpl_end(int a0, int Kg, uint8_t *dbg_templates, long long *dbg_cycles)
{
    SID_PHASE_LOCALS;
    constexpr int s = S;
    const double nd = G.nd;
    if (dbg_cycles && tid == 0) dbg_cycles[15] = (long long)clock64();
    const int ones = G.ones_slot;                                      // 15; 7 with two slot groups (K <= 7); 3 with four (K <= 3)
    const int spg = ones + 1, ng = kSlots / spg;                       // slots per group, groups
    const bool paired = ng > 1;
    struct { int u_off, strip_off; } GO{G.u_off, G.strip_off};         // (by value: see rp_tpl_table)
    for (int idx = tid; idx < s * s; idx += kBlockM) {                  // the all-ones template
        const int i = idx / s, j = idx - i * s;
        smem[rp_off<TS>(GO, i, j, ones)] = 1;
    }
    __syncthreads();
    if (paired) {
        // strip columns of the upper slots: the same column pairs four template rows further down (their accumulators
        // belong to the output rows y0+4 .. y0+7; in the main columns the lag is in the operand address instead)
        constexpr int nc = s - 32;
        for (int idx = tid; idx < spg * s * nc; idx += kBlockM) {
            const int a = idx / (s * nc), rem = idx - a * s * nc;
            const int i = rem / nc, c = rem - i * nc;
            if (a < Kg || a == ones) {
                const uint8_t v = smem[rp_off<TS>(GO, i, 32 + c, a)];
                for (int g = 1; g < ng; ++g) smem[rp_off<TS>(GO, i + 4 * g, 32 + c, a + g * spg)] = v;   // group g: 4 g template rows down
            }
        }
    }
    if (dbg_cycles && tid == 0) dbg_cycles[9] = (long long)clock64();
    if (dbg_templates) {
        for (int idx = tid; idx < Kg * s * s; idx += kBlockM) {
            const int a = idx / (s * s), rem = idx - a * s * s;
            const int i = rem / s, j = rem - i * s;
            dbg_templates[(a0 + a) * s * s + rem] = smem[rp_off<TS>(G, i, j, a)] ^ 0x80;
        }
    }
    if (tid == 0) m->any_const = 0;
    __syncthreads();                                                   // (also: every wavefront is done with the patch)
    if (a0 == 0 && wv != 0) rp_wt_build(tid - 64, kBlockM - 64);       // wavefronts 1..: the transposed window columns
    if (tid < kSlots) {                                                // per-slot terms of this group (signed domain)
        // paired slots: slots 8..15 carry the same angles as 0..7 (for the output rows four further down)
        const int ang = tid & (spg - 1);
        const bool live = ang < Kg, owner = tid == ang;
        const int sti = live ? m->isT[ang] : 0;
        const double st = (double)sti, stt = live ? (double)m->isTT[ang] : 1.0;
        const double dT = nd * stt - st * st;                          // exact
        const double rT = 1.0 / sqrt(dT);
        if (live && owner) {
            m->sTd[a0 + ang] = st;
            m->constT[a0 + ang] = dT == 0.0 ? 1 : 0;
            m->rTd[a0 + ang] = rT;
            if (dT == 0.0) m->any_const = 1;
        }
        // float32 pre-filter terms: mean of the template rounded to an integer, the rest of it, and N / sqrt(dT)
        const int mi = (int)floor(st / nd + 0.5);
        const float aT = !live ? 0.0f : (dT == 0.0 ? NAN : (float)(nd * rT));   // NaN estimate => always a candidate
        m->nmTi[tid] = live ? -mi : 0;
        m->ncTf[tid] = live ? -(float)((st - nd * (double)mi) / nd) : 0.0f;
        m->aTf[tid] = aT;
        m->biasf[tid] = live ? 0.0f : -INFINITY;
    }
    __syncthreads();
    if (tid == 0) {                                                    // largest factor of the group (fmaxf drops a NaN)
        float mx = 0.0f;
        for (int a = 0; a < kSlots; ++a) mx = fmaxf(mx, fabsf(m->aTf[a]));
        m->maxA = mx;
    }
    __syncthreads();
    SID_SETPRIO_TS(SWEEP);                                             // (what follows is the sweep)
}

// ---------------------------------------------------------------------------------------------
// the MFMA part of one work item: 4 output rows x (32 | 16) placements x 16 slots
//   la : this lane's base in the operand table (row -1, its slot, its half row)      E(p) = la + (2p+1) TP, O(p) = la + 2p TP (TP: bytes per table row)
//   bo : LDS offset of this lane's window bytes of step 0 (PAIR: 8-aligned; else dword-aligned)   step j at bo + j * wpitch2
// ---------------------------------------------------------------------------------------------
// PAIRED (at most 7 angles; BAND = 4): the lanes of slots 8..15 read the operands of slots 0..7 two row pairs earlier
// (`la` arrives four table rows lower for them), so their accumulators belong to the output rows y0+4 .. y0+7: 8 output
// rows per item with 4 accumulators.  Two steps more; where one half of the lanes has no template row pair (the first two
// and the last two loads) its operand registers are zeroed - whatever was read there lies inside the workgroup's LDS.
// PITCH: bytes per window row when the launch fixes them at compile time (one value per launch class: every step's LDS
// offset is then an immediate of its ds_read and the loop carries no address arithmetic), 0: run-time value (wpitch2).
// grp: the slot group of this lane's A operand (0 without groups); it lags 2 grp row pairs.
template <int S, bool PAIR, int BAND = 4, int PAIRED = 0, int PITCH = 0>
__device__ __forceinline__ void rp_item_main(v4i (&acc)[BAND][PAIR ? 2 : 1], const uint8_t *la, u32 bo, int wpitch2, u32 sh,
                                             int grp = 0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(!PAIRED || BAND == 4, "slot groups: four accumulators, 4 x groups output rows");
    constexpr int NG = rp_ngroups(PAIRED);
    using Sh = RpShape<S, PAIRED ? 4 * NG : BAND>;                    // (groups: the step count of a band of 4 NG rows)
    constexpr int LAG = 2 * (NG - 1);                                 // row pairs the last slot group lags behind
    constexpr int NT = PAIR ? 2 : 1, ND = BAND / 2;                    // ND: pairs of output rows = depth of the operand ring
    struct Frag { v4i f[NT]; };
    struct RawT { Raw6 p; Raw5 q; };
    Off3 b3 = Off3::make(bo);
    constexpr bool kB32 = !PAIR && rp_pitch_bytes(PITCH) != 0;         // (compile-time pitch: the offsets are immediates)
    Off5 b5 = Off5::make(kB32 ? bo : 0u);
    auto rd = [&](u32 d) { RawT r; if (PAIR) r.p = read_raw6(b3.plus(d)); else if (kB32) r.q = read_raw5(b5, d); else r.q = read_raw(smem + bo + d); return r; };
    auto build = [&](const RawT &r) {
        Frag o;
        if (PAIR) { o.f[0] = align_raw6<0>(r.p, sh); o.f[NT - 1] = align_raw6<1>(r.p, sh); }
        else o.f[0] = align_raw(r.q, sh);
        return o;
    };
    auto half_mask = [&](v4i v, int p, int n) {                       // n = nE or nO: row pairs that exist
        if (!PAIRED) return v;
        // group g holds row pair p - 2 g: it exists for 2 g <= p < n + 2 g.  The groups that fail form a run at one end
        // (compile-time after unrolling): the first steps lack the late groups, the last steps the early ones.
        const int g_hi = p / 2;                                        // groups 0 .. g_hi have started
        const int g_lo = p >= n ? (p - n) / 2 + 1 : 0;                 // groups below g_lo have run out
        if (g_hi >= NG - 1 && g_lo == 0) return v;
        const bool keep = grp <= g_hi && grp >= g_lo;
        v4i o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = keep ? v[i] : 0;
        return o;
    };
    constexpr int TP = rp_tab_pitch(PAIRED);                          // bytes per operand-table row
    auto ldE = [&](int p) { return half_mask(*reinterpret_cast<const v4i *>(la + (2 * p + 1) * TP), p, Sh::nE); };
    auto ldO = [&](int p) { return half_mask(*reinterpret_cast<const v4i *>(la + (2 * p) * TP), p, Sh::nO); };
    // (the accumulators arrive holding the strip columns' sums)  two-deep software pipeline: during the MFMAs of step j the fragments of step j+1 are finished
    // (v_alignbyte) and the LDS reads of step j+2 are issued.  eh[d] / oh[d]: operands E(j - d) / O(j - d) of the rows 2d / 2d+1
    Frag f_cur = build(rd(0));
    v4i eh[ND], oh[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) { eh[d] = v4i{0, 0, 0, 0}; oh[d] = v4i{0, 0, 0, 0}; }
    eh[0] = ldE(0); oh[0] = ldO(0);
    constexpr int PB = rp_pitch_bytes(PITCH);
    RawT raw_nxt = rd(PB ? 2u * PB : (u32)wpitch2);
    v4i e_nxt = ldE(1), o_nxt = ldO(1);
    if (!PB) { if (PAIR) b3.advance(2u * (u32)wpitch2); else bo += 2u * (u32)wpitch2; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < Sh::NS; ++j) {
        const Frag f_nxt = build(raw_nxt);
        const v4i e_n = e_nxt, o_n = o_nxt;
        if (j + 2 < Sh::NS) {
            raw_nxt = rd(PB ? (u32)((j + 2) * 2 * PB) : 0u);
            if (!PB) { if (PAIR) b3.advance((u32)wpitch2); else bo += (u32)wpitch2; }
            if (j + 2 < Sh::nE + LAG) e_nxt = ldE(j + 2);
            if (j + 2 < Sh::nO + LAG) o_nxt = ldO(j + 2);
        }
#pragma unroll
        for (int k = 0; k < NT; ++k) {
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                if (j - d >= 0 && j - d < Sh::nE + LAG) acc[2 * d][k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(eh[d], f_cur.f[k], acc[2 * d][k], 0, 0, 0);
                if (j - d >= 0 && j - d < Sh::nO + LAG) acc[2 * d + 1][k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(oh[d], f_cur.f[k], acc[2 * d + 1][k], 0, 0, 0);
            }
        }
#pragma unroll
        for (int q = 0; q < BAND * NT; ++q) {                        // one MFMA, then up to three of the others
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x106, 3, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int d = ND - 1; d > 0; --d) { eh[d] = eh[d - 1]; oh[d] = oh[d - 1]; }
        eh[0] = e_n; oh[0] = o_n; f_cur = f_nxt;
    }
}

// strip columns of one tile: wtl = LDS offset of this lane's WT byte (row = its placement column + (g & 1), byte y0 +
// 16 (g >> 1): dword-aligned), fl = strip fragments + 16 * lane.  Template rows 32.. (second row group; with slot groups
// the moved-down rows reach 33 + 12 < 48) all lie in the k-groups g >> 1 = 0: the others multiply zeros there and read
// along with them (stays inside the WT row).
template <int S, int BAND = 4>
__device__ __forceinline__ void rp_item_strip(v4i (&acc)[BAND], u32 wtl, int wp_pitch, int g16hi, const uint8_t *fl)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Sh = RpShape<S, BAND>;
    constexpr int ND = BAND == 8 ? 6 : 5;                             // dwords per read: shifts 0 .. BAND-1, then 16 bytes
#pragma unroll
    for (int cp = 0; cp < Sh::ncp; ++cp) {
#pragma unroll
        for (int rg = 0; rg < Sh::nrg; ++rg) {
            const u32 off = wtl + (u32)(2 * cp * wp_pitch + 32 * rg) - (rg == Sh::nrg - 1 ? (u32)g16hi : 0u);
            const v4i a = *reinterpret_cast<const v4i *>(fl + (cp * Sh::nrg + rg) * 1024);
            const u32 *src = reinterpret_cast<const u32 *>(smem + off);
            u32 d[ND];
#pragma unroll
            for (int i = 0; i < ND; ++i) d[i] = src[i];
            // output row t of the band = the same 16 bytes t further on
#pragma unroll
            for (int t = 0; t < BAND; ++t) {
                const int q = t >> 2;
                v4i b;
                if (t & 3) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) b[i] = (int)__builtin_amdgcn_alignbyte(d[q + i + 1], d[q + i], (u32)(t & 3));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) b[i] = (int)d[q + i];
                }
                acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[t], 0, 0, 0);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// sweep of one angle group
// ---------------------------------------------------------------------------------------------
constexpr float kGuardA = 2e-4f;        // N / sqrt(dT dI) above this: the float32 estimate is not trusted (flat window / template)

// BAND: output rows per work item - 4 with 168 VGPRs (three wavefronts per SIMD), 8 with 256 (the class that runs two
// workgroups of four wavefronts per CU): a window fragment then feeds 16 MFMAs instead of 8, i.e. 21 steps of fragment
// builds and operand reads per 8 rows instead of 38 - for a class whose wavefronts are bound by their own instruction stream.
// PAIRED: see rp_item_main - accumulator row t of a lane belongs to output row y0 + t (slots 0..7: k-groups 0, 1) or
// y0 + 4 + t (slots 8..15: k-groups 2, 3); items cover 8 output rows, the LDS layout is that of an 8-row band.
template <int S, int BAND, int PAIRED, int PITCH = 0>
__device__ __forceinline__ Score rp_sweep(Score sc, int a0, int Kg, const u32 *sii, long long *dbg_cycles)
{
    SID_PHASE_LOCALS;
    uint4 *queue = reinterpret_cast<uint4 *>(smem + G.queue_off);
    const int rh = G.rh, rw = G.rw, wpitch = rp_pitch_bytes(PITCH) ? rp_pitch_bytes(PITCH) : G.wpitch, wp_pitch = G.wp_pitch;
    const double nd = G.nd;
    // this lane's operand-table base: slot n_l, template row offset g >> 1, columns 16 (g & 1)
    constexpr int NG = rp_ngroups(PAIRED), SPG = kSlots / NG;          // slot groups, slots per group
    const int a_grp = PAIRED ? n_l / SPG : 0;                          // slot group of this lane's A operand (slot n_l)
    constexpr int TP = rp_tab_pitch(PAIRED);
    const uint8_t *la = smem + G.u_off + (q_l >> 1) * TP + (n_l & (SPG - 1)) * 32 + (q_l & 1) * 16 - a_grp * 4 * TP;
    constexpr int ROWS = PAIRED ? 4 * NG : BAND;                       // output rows per item
    const int c_grp = PAIRED ? (4 * q_l) / SPG : 0;                    // slot group of this lane's accumulators (slots 4 q .. 4 q + 3)
    // share of the accumulator rows t = 0 .. BAND-1 whose per-placement scoring terms this lane computes: the lanes of the
    // other quarters with the same placement column AND rows (all four; the two of a half with two slot groups; none with
    // four groups - every quarter then has rows of its own) take the rest
    constexpr int NSH = PAIRED == 2 ? 4 : PAIRED == 1 ? 2 : BAND / 4;
    const int sh_q = PAIRED == 2 ? 0 : PAIRED == 1 ? (q_l & 1) : q_l;  // this lane's index among the sharing quarters
    auto row_of = [&](int j) { return PAIRED == 2 ? j : PAIRED == 1 ? 2 * sh_q + j : sh_q + 4 * j; };
    // lane (byte address for ds_bpermute) of the quarter that computes row t for this lane's column, and the j it has there
    auto src_of = [&](int t) { return PAIRED ? ((16 * ((q_l & 2) + (t >> 1)) + n_l) << 2) : ((16 * (t & 3) + n_l) << 2); };
    auto j_of = [](int t) { return PAIRED == 2 ? t : PAIRED == 1 ? (t & 1) : (t >> 2); };
    const int yup = 4 * c_grp;                                         // ... and this lane's accumulators start this many rows down
    // lane holding the ones slot of this lane's rows (register 3): slot SPG - 1 of its group (four groups: the lane itself)
    const int sw_src = (n_l + 16 * ((c_grp * SPG + SPG - 1) >> 2)) << 2;
    const uint8_t *fl = smem + G.strip_off + lane * 16;
    // The per-slot terms of the scoring (accumulator register r of this lane belongs to slot 4 q + r) are fetched
    // from LDS after every item's MFMAs rather than kept in registers across them: the kernel body must not spill
    // (DESIGN.md section 6b - values parked in scratch did not survive three workgroups per CU).
    typedef float v2f __attribute__((ext_vector_type(2)));
    typedef float v4f __attribute__((ext_vector_type(4)));
    constexpr bool GSW = rp_pitch_is_gs(PITCH);                        // sum w' kept for the winner: in LDS (si_off), or - gs launches - behind sum w'^2 in global memory (gsi)
    const bool keep_si = GSW ? G.gsi != 0 : G.si_off != 0;
    int *si_tab = GSW ? reinterpret_cast<int *>(const_cast<u32 *>(sii) + G.gsi) : reinterpret_cast<int *>(smem + G.si_off);
    // kept accumulators (PMArgs::gs_keep_acc; gs launches): every lane stores its four slots of every (row, placement) it holds
    // - 16 bytes each - for rp_winner_kept
    constexpr bool KEEPC = GSW && PAIRED != 0;
    const int gsa = KEEPC ? __builtin_amdgcn_readfirstlane(G.gsa) : 0, gsa_rw = KEEPC ? __builtin_amdgcn_readfirstlane(G.gsa_rw) : 0;
    const float maxA = __builtin_amdgcn_readfirstlane(__float_as_int(m->maxA)) == 0 ? 0.0f
                     : __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m->maxA)));
    const bool force_b = m->any_const != 0;
#define STAMP2(k) do { if (dbg_cycles && tid == 0) dbg_cycles[k] = (long long)clock64(); } while (0)

    // Work items (rp_sweep_items): nbands x npair pair items (32 placements, cost 2), then the single items (16 placements,
    // cost 1) - one per band for its leftover columns, or (full-table kernels, where that is fewer units) RAGGED ones that
    // pack the leftover columns of all bands, every lane in a band of its own (rp_sweep_single_lane).  A wavefront takes
    // every W-th pair item and then every W-th single item counted from the other end of the wavefronts, so that the ones
    // that got one pair item fewer get one single item more (dealing items w, w + W, ... of the mixed list gave half the
    // wavefronts only pair items and the others only single ones).
    // Bands run from the middle of the window outwards (the leftover columns in the ragged items too): the peak is near the
    // first guess, so the running maximum is high early and most items never reach the candidate pass.
    constexpr bool RAG = rp_sweep_ragged_ok(PAIRED);
    RpSweepItems I;
    I.rows = ROWS; I.nbands = (rh + ROWS - 1) / ROWS; I.npair = RAG ? G.sw_npair : G.npair; I.rem = RAG ? G.sw_rem : 0;
    const int nbands = I.nbands;
    const int npair = I.npair, win_off = G.win_off, wp_off = G.wp_off, npos = G.npos;   // (LDS reads: once)
    const int n_pair_items = nbands * npair, n_single_items = RAG ? G.sw_nsing : nbands * G.nsingle;
    const int my_pairs = wv < n_pair_items ? (n_pair_items - wv + kWavesM - 1) / kWavesM : 0;
    const int wr = kWavesM - 1 - wv;
    const int my_singles = wr < n_single_items ? (n_single_items - wr + kWavesM - 1) / kWavesM : 0;
    // (band order, x tile) of the item walked without a division per item: item index += W means
    // x tile += W mod npair (with carry), band order += W div npair
    const int np1 = npair > 0 ? npair : 1;
    const int step_bo = kWavesM / np1, step_xi = kWavesM - step_bo * np1;
    int p_bo = wv / np1, p_xi = wv - p_bo * np1;
    for (int it = 0; it < my_pairs + my_singles; ++it) {
        const bool pair = it < my_pairs;                               // wavefront-uniform
        const int item = it == 0 ? wv : -1;                            // (phase-cycle stamps: first item of wavefront 0)
        const int ntile = pair ? 2 : 1;
        if (RAG && item == wv) STAMP2(10);
        // This lane's share of the item.  pA: row-major index of the placement of its accumulator row 0 in tile A (or the single
        // tile); row t is t * rw further on, tile B four columns.  okbits, bit BAND k + t: accumulator row t of tile k lies
        // inside the matrix.  In a pair item the rows are a mask of the band - wavefront-uniform without slot groups: scalar
        // arithmetic - and the column one compare per tile; in a single item band and mask belong to the lane.
        // wtlA / wtlB: the lane's byte of the transposed strip copy, mbo / msh: its window bytes of step 0 (rp_item_strip, rp_item_main).
        // The slot-group kernels (and kept accumulators) have no ragged items: every item has ONE band, y0u, and the placement
        // is kept as (y0u, xAu) - their lanes' rows differ by slot group (yup) and the accumulator table has a pitch of its own.
        int pA = 0, y0u = 0, xAu = 0, xBu = 0, x0u = 0; u32 okbits, wtlA = 0, wtlB = 0, mbo = 0, msh = 0;
        if (!RAG) {
            int bo, xi;
            if (pair) {
                bo = p_bo; xi = p_xi;
                p_bo += step_bo; p_xi += step_xi;
                if (p_xi >= np1) { p_xi -= np1; ++p_bo; }
            } else { bo = wr + (it - my_pairs) * kWavesM; xi = npair; }    // (one single item per band)
            const int y0 = rp_band_y0(rp_band_of_order(bo, nbands), nbands, rh, ROWS), x0 = xi * 32;
            if (item == wv) STAMP2(10);
            const int xA = pair ? x0 + (n_l & 3) + 8 * (n_l >> 2) : x0 + n_l, xB = pair ? xA + 4 : rw;   // xB = rw: no tile B
            const int rleft = rh - (y0 + yup);
            const u32 rowmask = rleft >= BAND ? (1u << BAND) - 1u : rleft <= 0 ? 0u : (1u << rleft) - 1u;
            okbits = (xA < rw ? rowmask : 0u) | (xB < rw ? rowmask << BAND : 0u);
            y0u = y0; xAu = xA; xBu = xB; x0u = x0;
        } else if (pair) {
            const int bo = p_bo, xi = p_xi;
            p_bo += step_bo; p_xi += step_xi;
            if (p_xi >= np1) { p_xi -= np1; ++p_bo; }
            const int y0 = rp_band_y0(rp_band_of_order(bo, nbands), nbands, rh, ROWS), x0 = xi * 32;
            const int xA = x0 + (n_l & 3) + 8 * (n_l >> 2), xB = xA + 4;
            const int rleft = rh - (y0 + yup);
            const u32 rowmask = rleft >= BAND ? (1u << BAND) - 1u : rleft <= 0 ? 0u : (1u << rleft) - 1u;
            okbits = (xA < rw ? rowmask : 0u) | (xB < rw ? rowmask << BAND : 0u);
            pA = (y0 + yup) * rw + xA;
            const int vA = xA < rw ? xA : rw - 1, vB = xB < rw ? xB : rw - 1;
            wtlA = (u32)(wp_off + (vA + (q_l & 1)) * wp_pitch + y0 + 16 * (q_l >> 1));
            wtlB = (u32)(wp_off + (vB + (q_l & 1)) * wp_pitch + y0 + 16 * (q_l >> 1));
            mbo = (u32)(win_off + (y0 + (q_l >> 1)) * wpitch + x0 + 8 * (n_l >> 2) + 16 * (q_l & 1));
            msh = (u32)(n_l & 3);
        } else {
            const RpSweepLane P = rp_sweep_single_lane(I, rh, rw, wr + (it - my_pairs) * kWavesM, n_l);
            const int y0 = P.y0, xA = P.x;
            const int rleft = rh - (y0 + yup);
            const u32 rowmask = rleft >= BAND ? (1u << BAND) - 1u : rleft <= 0 ? 0u : (1u << rleft) - 1u;
            okbits = P.live ? rowmask : 0u;
            pA = (y0 + yup) * rw + xA;
            const int vA = xA < rw ? xA : rw - 1;
            wtlA = (u32)(wp_off + (vA + (q_l & 1)) * wp_pitch + y0 + 16 * (q_l >> 1));
            const u32 sbyte = (u32)(xA + 16 * (q_l & 1));
            mbo = (u32)(win_off + (y0 + (q_l >> 1)) * wpitch) + (sbyte & ~3u);
            msh = sbyte & 3u;
        }
        // operands of the scoring that do not depend on the MFMAs: issued now, landed long before they are needed.
        // The per-placement part of the scoring (dI, 1 / sqrt(dI)) is the same in the four lane quarters that hold the
        // slots of one placement column: every quarter computes it for its SHARE of the band's rows only (row_of(j))
        // and the quarters exchange the results (ds_bpermute), so sum w'^2 is fetched for the share alone.
        auto pidx = [&](int k, int t) { return RAG ? pA + 4 * k + t * rw : (y0u + yup + t) * rw + (k == 0 ? xAu : xBu); };   // placement of accumulator row t, tile k
        u32 siis[2][NSH];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int j = 0; j < NSH; ++j) {
                const int t = row_of(j);
                const bool ok = RAG ? ((okbits >> (BAND * k + t)) & 1u) != 0u : ((k == 0 ? xAu : xBu) < rw) & (y0u + yup + t < rh);
                siis[k][j] = sii_at(sii, ok ? pidx(k, t) : 0);
            }
        }
        const u32 gkey = m->gmax_key;
        v4i accA[BAND], accB[BAND];                                    // tile A (or the single tile), tile B
#pragma unroll
        for (int t = 0; t < BAND; ++t) { accA[t] = v4i{0, 0, 0, 0}; accB[t] = v4i{0, 0, 0, 0}; }
        // strip columns first (their LDS latency overlaps the first reads of the main loop), then the 32 main columns
        if (!RAG) {
            const int vA = xAu < rw ? xAu : rw - 1;
            rp_item_strip<S, BAND>(accA, (u32)(wp_off + (vA + (q_l & 1)) * wp_pitch + y0u + 16 * (q_l >> 1)), wp_pitch, 16 * (q_l >> 1), fl);
            if (pair) {
                const int vB = xBu < rw ? xBu : rw - 1;
                rp_item_strip<S, BAND>(accB, (u32)(wp_off + (vB + (q_l & 1)) * wp_pitch + y0u + 16 * (q_l >> 1)), wp_pitch, 16 * (q_l >> 1), fl);
            }
        } else {
            rp_item_strip<S, BAND>(accA, wtlA, wp_pitch, 16 * (q_l >> 1), fl);
            if (pair) rp_item_strip<S, BAND>(accB, wtlB, wp_pitch, 16 * (q_l >> 1), fl);
        }
        if (pair) {
            v4i acc[BAND][2];
#pragma unroll
            for (int t = 0; t < BAND; ++t) { acc[t][0] = accA[t]; acc[t][1] = accB[t]; }
            if (!RAG) { mbo = (u32)(win_off + (y0u + (q_l >> 1)) * wpitch + x0u + 8 * (n_l >> 2) + 16 * (q_l & 1)); msh = (u32)(n_l & 3); }
            rp_item_main<S, true, BAND, PAIRED, PITCH>(acc, la, mbo, 2 * wpitch, msh, a_grp);
#pragma unroll
            for (int t = 0; t < BAND; ++t) { accA[t] = acc[t][0]; accB[t] = acc[t][1]; }
        } else {
            v4i acc[BAND][1];
#pragma unroll
            for (int t = 0; t < BAND; ++t) acc[t][0] = accA[t];
            if (!RAG) {
                const u32 sbyte = (u32)(x0u + n_l + 16 * (q_l & 1));
                mbo = (u32)(win_off + (y0u + (q_l >> 1)) * wpitch) + (sbyte & ~3u); msh = sbyte & 3u;
            }
            rp_item_main<S, false, BAND, PAIRED, PITCH>(acc, la, mbo, 2 * wpitch, msh, a_grp);
#pragma unroll
            for (int t = 0; t < BAND; ++t) accA[t] = acc[t][0];
        }
        if (item == wv) STAMP2(11);
        if (KEEPC && gsa != 0) {
            // (the table is padded to whole items: no predicates)
            unsigned char *ab = reinterpret_cast<unsigned char *>(const_cast<u32 *>(sii) + gsa) + 16u * (u32)(q_l & (SPG / 4 - 1));
            const u32 pitchb = (u32)gsa_rw * (4u * SPG);
            u32 o = (u32)((y0u + yup) * gsa_rw + xAu) * (4u * SPG);
#pragma unroll
            for (int t = 0; t < BAND; ++t) {
                *reinterpret_cast<v4i *>(ab + o) = accA[t];
                if (pair) *reinterpret_cast<v4i *>(ab + o + 16u * SPG) = accB[t];   // (tile B: the placement four columns on)
                o += pitchb;
            }
        }
        {
            const float gm = key2f(gkey);
            sc.lmax = gm > sc.lmax ? gm : sc.lmax;
        }
        // ---- scoring, pass A (always, branch-free): float32 estimates, their maximum per output row and per lane ----
        int swp[2][BAND]; float rIf[2][BAND], rowv[2][BAND];
        float itemmax = -INFINITY;
        u32 nanbits = 0;
        const v4i nmT = *reinterpret_cast<const v4i *>(&m->nmTi[4 * q_l]);
        const v4f cT = *reinterpret_cast<const v4f *>(&m->ncTf[4 * q_l]), aT = *reinterpret_cast<const v4f *>(&m->aTf[4 * q_l]),
                  bias = *reinterpret_cast<const v4f *>(&m->biasf[4 * q_l]);
        const v2f cT01 = {cT[0], cT[1]}, cT23 = {cT[2], cT[3]}, aT01 = {aT[0], aT[1]}, aT23 = {aT[2], aT[3]},
                  bias01 = {bias[0], bias[1]}, bias23 = {bias[2], bias[3]};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k < ntile) {                                           // wavefront-uniform
                const v4i (&acc)[BAND] = k == 0 ? accA : accB;
#pragma unroll
                for (int t = 0; t < BAND; ++t)                         // the ones slot = sum of w': slot 15 (lanes 48..63, register 3)
                    swp[k][t] = PAIRED == 2 ? acc[t][3] : __builtin_amdgcn_ds_bpermute(sw_src, acc[t][3]);
                // this lane's share of the per-placement terms
                float ris[NSH];
#pragma unroll
                for (int j = 0; j < NSH; ++j) {
                    const int tj = row_of(j);
                    // swp[k][row_of(j)]: the row varies with the lane QUARTER, i.e. with constant lane masks - explicit
                    // v_cndmask on those masks (written as a chain of ?: the compiler turns the selection into an indexed
                    // array in scratch memory: a store and a dependent load per tile in the hottest loop of the kernel)
                    int sw = swp[k][PAIRED ? j : 4 * j];
                    if (PAIRED == 2) { /* row_of(j) = j */ }
                    else if (PAIRED) sw = sel_lanes(sw, swp[k][2 + j], 0xffff0000ffff0000ull);          // quarters 1, 3
                    else {
                        sw = sel_lanes(sw, swp[k][4 * j + 1], 0x00000000ffff0000ull);                   // quarter 1
                        sw = sel_lanes(sw, swp[k][4 * j + 2], 0x0000ffff00000000ull);                   // quarter 2
                        sw = sel_lanes(sw, swp[k][4 * j + 3], 0xffff000000000000ull);                   // quarter 3
                    }
                    // (where the residency class has room: sum w' of the placement kept for the winner's matrix, rp_lds_layout)
                    if (keep_si && ((okbits >> (BAND * k + tj)) & 1u))
                        sii_put(reinterpret_cast<u32 *>(si_tab), pidx(k, tj), (u32)sw);
                    const double swd = (double)sw, siid = (double)siis[k][j];
                    const double dI = nd * siid - swd * swd;          // exact
                    float ri = __builtin_amdgcn_rsqf((float)dI);
                    // (nearly) flat window or template - also every dI <= N / 2 of the spec's low-variance rule, since
                    // N / sqrt(dT) >= 1 / 128: the float32 estimate is not trusted, the exact path decides
                    const bool flat = !(ri * maxA <= kGuardA);
                    ris[j] = flat ? NAN : ri;
                    const bool ok = (okbits >> (BAND * k + tj)) & 1u;
                    nanbits |= (ok && flat) ? 1u : 0u;
                }
#pragma unroll
                for (int t = 0; t < BAND; ++t)
                    rIf[k][t] = PAIRED == 2 ? ris[j_of(t)] : __int_as_float(__builtin_amdgcn_ds_bpermute(src_of(t), __float_as_int(ris[j_of(t)])));
#pragma unroll
                for (int t = 0; t < BAND; ++t) {
                    const float ri = rIf[k][t];                       // NaN for a flat window
                    const float swf = (float)swp[k][t];
                    // exact acc - m Sw' (v_mad_i32_i24), then two packed float32 FMAs per pair of slots
                    v2f ai01, ai23;
                    ai01[0] = (float)(__mul24(nmT[0], swp[k][t]) + acc[t][0]); ai01[1] = (float)(__mul24(nmT[1], swp[k][t]) + acc[t][1]);
                    ai23[0] = (float)(__mul24(nmT[2], swp[k][t]) + acc[t][2]); ai23[1] = (float)(__mul24(nmT[3], swp[k][t]) + acc[t][3]);
                    const v2f sw2 = {swf, swf};
                    const v2f e01 = __builtin_elementwise_fma(__builtin_elementwise_fma(sw2, cT01, ai01), aT01, bias01);
                    const v2f e23 = __builtin_elementwise_fma(__builtin_elementwise_fma(sw2, cT23, ai23), aT23, bias23);
                    const float rowmax = fmaxf(fmaxf(e01[0], e01[1]), fmaxf(e23[0], e23[1]));
                    const bool ok = (okbits >> (BAND * k + t)) & 1u;
                    const float rv = ok ? rowmax * ri : -INFINITY;    // NaN for a flat window
                    rowv[k][t] = rv;
                    itemmax = fmaxf(itemmax, rv);                     // (fmaxf drops the NaN; nanbits carries it)
                }
            } else {
#pragma unroll
                for (int t = 0; t < BAND; ++t) { swp[k][t] = 0; rIf[k][t] = 0.0f; rowv[k][t] = -INFINITY; }
            }
        }
        // The candidate pass runs when some lane holds an estimate within kMargin of the running maximum (or a NaN).  If
        // none does, the item cannot raise the maximum either: the wavefront-wide maximum (a chain of DPP steps) and the
        // update of the maximum shared between the wavefronts are only needed inside.
        const bool need_b = force_b || (__ballot(!(itemmax < sc.lmax - kMargin) || nanbits != 0) != 0ull);     // wavefront-uniform
        if (need_b) {
            sc.lmax = fmaxf(sc.lmax, wave_max_dpp(itemmax));
            // ---- pass B: queue the values within kMargin of the running maximum (and every NaN estimate);
            //      only the output rows in which some lane holds such a value are looked at value by value ----
            const float thr = sc.lmax - kMargin;
            unsigned long long ovf = 0;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (k < ntile) {
                    const v4i (&acc)[BAND] = k == 0 ? accA : accB;
#pragma unroll
                    for (int t = 0; t < BAND; ++t) {
                        const bool ok = (okbits >> (BAND * k + t)) & 1u;
                        const bool rowhit = ok && (force_b || !(rowv[k][t] < thr));  // true for NaN
                        if (__ballot(rowhit) == 0ull) continue;       // wavefront-uniform
                        const float swf = (float)swp[k][t];
                        const u32 siiv_kt = sii_at(sii, ok ? pidx(k, t) : 0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ai = __mul24(nmT[r], swp[k][t]) + acc[t][r];
                            const float v = fmaf(swf, cT[r], (float)ai);
                            const float e = fmaf(v, aT[r], bias[r]) * rIf[k][t];
                            if (ok && bias[r] == 0.0f && !(e < thr)) {                 // live slot; true for NaN
                                const int key = (a0 + ((4 * q_l + r) & (SPG - 1))) * npos + pidx(k, t);
                                const u32 slot = atomicAdd(&m->qcount, 1u);
                                if (slot < (u32)G.queue_cap) queue[slot] = make_uint4((u32)acc[t][r], (u32)swp[k][t], siiv_kt, (u32)key);
                                else ovf |= 1ull << (4 * BAND * k + 4 * t + r);
                            }
                        }
                    }
                }
            }
            // cold path (queue full: massive ties, flat windows, constant templates): evaluate in place, one at a time
            if (ovf) {
#pragma unroll 1
                for (int b = 0; b < 8 * BAND; ++b) {
                    if (!((ovf >> b) & 1ull)) continue;
                    const int k = b / (4 * BAND), t = (b >> 2) & (BAND - 1), r = b & 3;
                    int pv = 0, sw = 0;
                    const u32 si = sii_at(sii, pidx(k, t));   // (flagged values are valid placements)
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                        for (int tt = 0; tt < BAND; ++tt) {
                            const bool hit = (k == kk) & (t == tt);
                            sw = hit ? swp[kk][tt] : sw;
#pragma unroll
                            for (int rr = 0; rr < 4; ++rr) pv = (hit & (r == rr)) ? (kk == 0 ? accA[tt][rr] : accB[tt][rr]) : pv;
                        }
                    const int a = (4 * q_l + r) & (SPG - 1);
                    const int key = (a0 + a) * npos + pidx(k, t);
                    take_better(sc, exact_from_sums(pv, sw, si, nd, m->sTd[a0 + a], m->rTd[a0 + a], m->constT[a0 + a] != 0), key);
                }
            }
        }
        if (need_b && lane == 0) atomicMax(&m->gmax_key, f2key(sc.lmax));
        if (item == wv) STAMP2(12);
    }
#undef STAMP2
    __syncthreads();
    {
        const int nq = (int)(m->qcount < (u32)G.queue_cap ? m->qcount : (u32)G.queue_cap);
        for (int idx = tid; idx < nq; idx += kBlockM) {
            const uint4 rec = queue[idx];
            const int key = (int)rec.w;
            const int a = key / G.npos;
            take_better(sc, exact_from_sums((int)rec.x, (int)rec.y, rec.z, nd, m->sTd[a], m->rTd[a], m->constT[a] != 0), key);
        }
    }
    __syncthreads();
    if (tid == 0) m->qcount = 0;
    return sc;
}

#ifdef SID_DBG_CHECK
// debugging builds: the operand table against the template sums (tag = where in the kernel)
template <int S, int TS>
__device__ __noinline__ void rp_dbg_check(int Kg, int tag, int pt, int32_t *err, const uint8_t *img1, long long rows1, long long cols1, long long stride1)
{
    SID_PHASE_LOCALS;
    int32_t *err_list = err ? err + 64 : nullptr;
    if (tag == 0 && err) {                                             // patch against image 1
        int nb = 0;
        for (int idx = tid; idx < G.pdim * G.pdim; idx += kBlockM) {
            const int pr = idx / G.pdim, pc = idx - pr * G.pdim;
            const long long gr = G.pr0 + pr, gc = G.pc0 + pc;
            if (gr >= 0 && gc >= 0 && gr < rows1 && gc < cols1) nb += smem[G.patch_off + pr * G.ppitch + pc] != img1[gr * stride1 + gc];
        }
        nb = wave_sum_dpp(nb);
        if (lane == 0 && nb) atomicAdd(&err[3], nb);
    }
    for (int a = wv; a < Kg; a += kWavesM) {
        int st = 0, stt = 0;
        for (int idx = lane; idx < S * S; idx += 64) {
            const int i = idx / S, j = idx - i * S;
            const int v = (int)(int8_t)smem[rp_off<TS>(G, i, j, a)];
            st += v; stt += v * v;
        }
        st = wave_sum_dpp(st); stt = wave_sum_dpp(stt);
        if (tag == 0 && err) {                                         // table bytes against an exact resampling of the patch
            const SampleGeom g = sample_geom(G, S, rows1, cols1, smem + G.patch_off);
            int nb = 0;
            const bool first = err[2] == 0;
            for (int idx = lane; idx < S * S; idx += 64) {
                const int i = idx / S, j = idx - i * S;
                const int got = (int)(uint8_t)(smem[rp_off<TS>(G, i, j, a)] ^ 0x80), want = sample_exact(g, m->rot[a], i, j, a);
                if (got != want) {
                    ++nb;
                    if (first) { const int k = atomicAdd(&err[4], 1); if (k < 200) err_list[k] = (i << 24) | (j << 16) | (got << 8) | want; }
                }
            }
            nb = wave_sum_dpp(nb);
            if (lane == 0 && nb) { atomicAdd(&err[2], nb); err[40] = pt; err[41] = a; err[42] = nb; }
        }
        if (lane == 0 && (st != m->isT[a] || stt != m->isTT[a]) && err) {
            const int k = atomicAdd(&err[tag], 1);
            if (k < 4) { err[8 + 16 * tag + 4 * k] = pt; err[9 + 16 * tag + 4 * k] = a; err[10 + 16 * tag + 4 * k] = st - m->isT[a]; err[11 + 16 * tag + 4 * k] = stt - m->isTT[a]; }
        }
    }
    __syncthreads();
}
#endif

// ---------------------------------------------------------------------------------------------
// NCC matrix of the winning angle, row-pair form.  M = 16 output rows y0 .. y0+15, N = placements (pair items of
// 32 = two interleaved tiles, or a single tile of 16, as in the sweep), and
//   main columns 0..31:  K = window rows (rho, rho + 1) x 32 columns,  A[m][k] = T'[rho + (k >> 5) - y0 - m][k & 31]
//   strip columns 32.. : K = window rows rho .. rho + 3 x 16 columns (2 or 3 of them carry template),
//                        A[m][k] = T'[rho + (k >> 4) - y0 - m][32 + (k & 15)]
// with an all-ones operand next to each for S_I'.  Operand rows live in LDS with 16 zero rows above and 18 below,
// so every lane's fragment is an aligned ds_read_b128 at base + 64 * step.
//   TR, TR1: [kWRows][32 B] main columns (template, ones);  TS, TS1: [kWRows][16 B] strip columns.
// ---------------------------------------------------------------------------------------------
constexpr int kWPad = 16, kWRows = 68;                                 // 16 + s (<= 35) + >= 17 zero rows
constexpr int kTrOff = 0, kTr1Off = kWRows * 32, kTsOff = 2 * kWRows * 32, kTs1Off = 2 * kWRows * 32 + kWRows * 16;
static_assert(kTs1Off + kWRows * 16 <= 8192, "winner operands exceed their 8 KB");

// (Round 5 also measured an "x-shift" form of this matrix - M = 16 x-shifts of one template row, aligned window fragments, 306
// matrix instructions instead of 342 -: no faster, tools/patches/winner_x.patch)

template <int S>
__device__ __noinline__ void rp_winner_stage(const double *rot4, const uint16_t *samp, long long rows1, long long cols1, int ka)
{
    SID_PHASE_LOCALS;
    const uint8_t *patch = smem + G.patch_off;
    uint8_t *base = smem + G.u_off;
    constexpr int s = S;
    for (int idx = tid; idx < 8192 / 16; idx += kBlockM) reinterpret_cast<uint4 *>(base)[idx] = make_uint4(0, 0, 0, 0);
    if (tid < 4) m->rot[0][tid] = rot4[tid];
    __syncthreads();
    const SampleGeom g = sample_geom(G, s, rows1, cols1, patch);
    auto put = [&](int i, int j, int v) {
        if (j < 32) { base[kTrOff + (i + kWPad) * 32 + j] = (uint8_t)(v ^ 0x80); base[kTr1Off + (i + kWPad) * 32 + j] = 1; }
        else { base[kTsOff + (i + kWPad) * 16 + (j - 32)] = (uint8_t)(v ^ 0x80); base[kTs1Off + (i + kWPad) * 16 + (j - 32)] = 1; }
    };
    if (samp) {                                                        // offset table (caller checked table_usable)
        const int sp = samp_pitch(s), nq = sp >> 2, upa = s * nq;
        const u32 tailmask = (s & 3) ? (1u << (8 * (s & 3))) - 1u : 0xffffffffu;
        const uint2 *ta = reinterpret_cast<const uint2 *>(samp + (size_t)ka * s * sp);
        for (int u = tid; u < upa; u += kBlockM) {
            const int i = u / nq, jq = u - i * nq;
            const uint2 e = ta[u];
            const u32 vm = jq == nq - 1 ? tailmask : 0xffffffffu;
            const u32 raw = gather_quad(patch, e);
            if (jq < 8) {
                *reinterpret_cast<u32 *>(base + kTrOff + (i + kWPad) * 32 + 4 * jq) = raw ^ 0x80808080u;
                *reinterpret_cast<u32 *>(base + kTr1Off + (i + kWPad) * 32 + 4 * jq) = 0x01010101u;
            } else {
                *reinterpret_cast<u32 *>(base + kTsOff + (i + kWPad) * 16) = (raw ^ 0x80808080u) & vm;
                *reinterpret_cast<u32 *>(base + kTs1Off + (i + kWPad) * 16) = 0x01010101u & vm;
            }
            // flagged entries (coordinate within kSampGuard of a rounding boundary): the reference's float64 order
            if ((e.x | e.y) & 0x80008000u) {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const u32 ent = b == 0 ? e.x & 0xffffu : b == 1 ? e.x >> 16 : b == 2 ? e.y & 0xffffu : e.y >> 16;
                    const int j = 4 * jq + b;
                    if ((ent & 0x8000u) && j < s) put(i, j, sample_exact(g, m->rot[0], i, j, ka));
                }
            }
        }
    } else {
        for (int idx = tid; idx < s * s; idx += kBlockM) {             // on-the-fly centres: scipy's double arithmetic throughout
            const int i = idx / s, j = idx - i * s;
            put(i, j, sample_exact(g, m->rot[0], i, j, ka));
        }
    }
}

// The same operands copied out of the sweep's table (one group of angles: the table still holds every template, the
// flagged samples already redone): no second pass over the sampling table, no patch.
template <int S, int TS>
__device__ __noinline__ void rp_winner_stage_tab(int a)
{
    SID_SETPRIO_TS(WIN);
    SID_PHASE_LOCALS;
    uint8_t *base = smem + G.u_off;
    constexpr int nu = S * 9;                                          // per template row: 8 dwords + the strip bytes
    constexpr u32 ones_strip = S > 34 ? 0x00010101u : 0x00000101u;
    u32 val[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int u = tid + k * kBlockM;
        if (u < nu) {
            const int i = u / 9, q = u - 9 * i;
            if (q < 8) val[k] = *reinterpret_cast<const u32 *>(smem + G.u_off + ((i + 1) << TS) + a * 32 + 4 * q);
            else val[k] = (u32)smem[rp_off<TS>(G, i, 32, a)] | ((u32)smem[rp_off<TS>(G, i, 33, a)] << 8) |
                          (S > 34 ? (u32)smem[rp_off<TS>(G, i, 32 + (S > 34 ? 2 : 0), a)] << 16 : 0u);
        }
    }
    __syncthreads();                                                   // every wavefront has read its share of the table
    for (int idx = tid; idx < 8192 / 16; idx += kBlockM) reinterpret_cast<uint4 *>(base)[idx] = make_uint4(0, 0, 0, 0);
    if (G.hist_off) {                                                  // ph_hessian_fast's histogram + list fill count
        for (int idx = tid; idx < 4096 / 16; idx += kBlockM) reinterpret_cast<uint4 *>(smem + G.hist_off)[idx] = make_uint4(0, 0, 0, 0);
        if (tid == 0) m->sel_cle = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int u = tid + k * kBlockM;
        if (u < nu) {
            const int i = u / 9, q = u - 9 * i;
            if (q < 8) {
                *reinterpret_cast<u32 *>(base + kTrOff + (i + kWPad) * 32 + 4 * q) = val[k];
                *reinterpret_cast<u32 *>(base + kTr1Off + (i + kWPad) * 32 + 4 * q) = 0x01010101u;
            } else {
                *reinterpret_cast<u32 *>(base + kTsOff + (i + kWPad) * 16) = val[k];
                *reinterpret_cast<u32 *>(base + kTs1Off + (i + kWPad) * 16) = ones_strip;
            }
        }
    }
}

// one tile row of 16 output rows x (32 | 16) placements: main steps, strip steps, exact normalisation
// ONES: the all-ones operand is multiplied along (sum w' per placement); false: that sum comes from the table the sweep kept
// (Geo::si_off) and half of the matrix instructions and operand reads go
template <int S, bool PAIR, int PITCH = 0, bool ONES = true, bool BIG = false>
__device__ __forceinline__ void rp_winner_item(int y0, int x0, const double sT, const double rT, const bool cT, const u32 *sii,
                                               long long *dbg = nullptr)
{
    SID_PHASE_LOCALS;
    constexpr int NT = PAIR ? 2 : 1;
    constexpr int NM = (16 + S - 1 + 1) / 2, NQ = (16 + S - 1 + 3) / 4;  // main steps (2 window rows), strip steps (4 rows)
    float *ccm = tab_ptr<BIG, float>(G, smem, G.ccm_off);
    const uint8_t *base = smem + G.u_off;
    const int rh = G.rh, rw = G.rw, wpitch = rp_pitch_bytes(PITCH) ? rp_pitch_bytes(PITCH) : G.wpitch;
    // operand bases of this lane (m = n_l output row, g = q_l k-group)
    const uint8_t *aM = base + kTrOff + ((q_l >> 1) - n_l + kWPad) * 32 + 16 * (q_l & 1);
    const uint8_t *aS = base + kTsOff + (q_l - n_l + kWPad) * 16;
    // sum w'^2 of this lane's NT x 4 placements: from global memory (gs instantiations) the loads are issued ahead of the MFMA
    // loops; from LDS they are fetched behind them (eight more live registers through the loops cost the 128-VGPR build of
    // the slot-group kernels 5 % at border 20)
    constexpr bool GS = rp_pitch_is_gs(PITCH);
    int idxv[NT][4]; u32 siv[NT][4]; int swv[NT][4];
    const u32 *siw = GS ? sii + G.gsi : reinterpret_cast<const u32 *>(smem + G.si_off);   // (sum w' kept by the sweep: read when !ONES)
    auto fetch_sii = [&]() {
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const int x = PAIR ? x0 + (n_l & 3) + 8 * (n_l >> 2) + 4 * k : x0 + n_l;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = y0 + 4 * q_l + r;
                const bool ok = y < rh && x < rw;
                idxv[k][r] = ok ? y * rw + x : -1;
                siv[k][r] = sii_at(sii, ok ? y * rw + x : 0);
                if (!ONES) swv[k][r] = (int)sii_at(siw, ok ? y * rw + x : 0);
            }
        }
    };
    if (GS) fetch_sii();
    v4i accT[NT], accS[NT], accT1[NT], accS1[NT];                       // even / odd steps: independent MFMA chains
#pragma unroll
    for (int k = 0; k < NT; ++k) { accT[k] = v4i{0, 0, 0, 0}; accS[k] = v4i{0, 0, 0, 0}; accT1[k] = v4i{0, 0, 0, 0}; accS1[k] = v4i{0, 0, 0, 0}; }
    struct Frag { v4i f[NT]; };
    auto run = [&](u32 bo, u32 stride_rt, const uint8_t *ap, int a1off, int nsteps, auto rows_tag) {
        // stride: a compile-time constant when the launch fixes the window pitch (all step offsets become immediates)
        constexpr int kRowsPerStep = decltype(rows_tag)::value;
        const u32 stride = rp_pitch_bytes(PITCH) ? (u32)(kRowsPerStep * rp_pitch_bytes(PITCH)) : stride_rt;
        // window bytes of step t at LDS offset bo + t * stride; operands at ap + 64 t (template) and + a1off (ones)
        Off3 b3 = Off3::make(bo);
        const u32 sh = PAIR ? (u32)(n_l & 3) : (bo & 3u);
        const u32 bo4 = bo & ~3u;
        constexpr bool kB32 = !PAIR && rp_pitch_bytes(PITCH) != 0;     // (as in rp_item_main: five ds_read_b32 with immediate offsets)
        Off5 b5 = Off5::make(kB32 ? bo4 : 0u);
        auto rd = [&](u32 d, Raw6 &p6, Raw5 &p5) { if (PAIR) p6 = read_raw6(b3.plus(d)); else if (kB32) p5 = read_raw5(b5, d); else p5 = read_raw(smem + bo4 + d); };
        auto build = [&](const Raw6 &p6, const Raw5 &p5) {
            Frag o;
            if (PAIR) { o.f[0] = align_raw6<0>(p6, sh); o.f[NT - 1] = align_raw6<1>(p6, sh); } else o.f[0] = align_raw(p5, sh);
            return o;
        };
        // operands and window bytes are fetched kDepth steps ahead: with four wavefronts reading ~3.5 KB of LDS per step
        // each, a round trip takes longer than two steps of four MFMAs
        constexpr int kDepth = 3;
        Raw6 r6[kDepth]; Raw5 r5[kDepth];
        v4i at_[kDepth], a1_[kDepth];
#pragma unroll
        for (int d = 0; d < kDepth; ++d) {
            if (d < nsteps) {
                rd((u32)d * stride, r6[d], r5[d]);
                at_[d] = *reinterpret_cast<const v4i *>(ap + 64 * d);
                if (ONES) a1_[d] = *reinterpret_cast<const v4i *>(ap + a1off + 64 * d);
            }
        }
#pragma unroll
        for (int t = 0; t < nsteps; ++t) {
            const int sl = t % kDepth;
            const Frag f = build(r6[sl], r5[sl]);
            const v4i at = at_[sl], a1 = a1_[sl];
            if (t + kDepth < nsteps) {
                rd((u32)(t + kDepth) * stride, r6[sl], r5[sl]);
                at_[sl] = *reinterpret_cast<const v4i *>(ap + 64 * (t + kDepth));
                if (ONES) a1_[sl] = *reinterpret_cast<const v4i *>(ap + a1off + 64 * (t + kDepth));
            }
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                if (t & 1) { accT1[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(at, f.f[k], accT1[k], 0, 0, 0);
                             if (ONES) accS1[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, f.f[k], accS1[k], 0, 0, 0); }
                else       { accT[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(at, f.f[k], accT[k], 0, 0, 0);
                             if (ONES) accS[k] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, f.f[k], accS[k], 0, 0, 0); }
            }
        }
    };
    // main columns: lane reads window row y0 + 2 t + (g >> 1), columns x0 + (16 (g & 1) ..)
    {
        const u32 col = PAIR ? (u32)(x0 + 8 * (n_l >> 2) + 16 * (q_l & 1)) : (u32)(x0 + n_l + 16 * (q_l & 1));
        run((u32)(G.win_off + (y0 + (q_l >> 1)) * wpitch) + col, (u32)(2 * wpitch), aM, kTr1Off - kTrOff, NM, std::integral_constant<int, 2>{});
    }
    // strip columns: window row y0 + 4 t + g, columns x0 + 32 ..
    {
        const u32 col = PAIR ? (u32)(x0 + 32 + 8 * (n_l >> 2)) : (u32)(x0 + 32 + n_l);
        run((u32)(G.win_off + (y0 + q_l) * wpitch) + col, (u32)(4 * wpitch), aS, kTs1Off - kTsOff, NQ, std::integral_constant<int, 4>{});
    }
    const double nd = G.nd;
    if (dbg && tid == 0) dbg[17] = (long long)clock64();
    // normalisation of the NT x 4 values of this lane as one branch-free batch (ncc_fast_nobranch); the few that need the
    // specification's own route are redone afterwards
    if (!GS) fetch_sii();
    int pv[NT][4], sv[NT][4]; float res[NT][4];
    u32 slowbits = 0;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const v4i aT = accT[k] + accT1[k], aS1 = accS[k] + accS1[k];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pv[k][r] = aT[r];
            sv[k][r] = ONES ? aS1[r] : swv[k][r];
        }
    }
    if (cT) {                                                          // a constant template: 1 everywhere (uniform for the angle)
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) res[k][r] = 1.0f;
    } else {
        const ncc_norm::Hoisted hc = ncc_norm::Hoisted::make(nd, sT, rT);
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bool sl;
                res[k][r] = ncc_fast_nobranch(pv[k][r], sv[k][r], siv[k][r], hc, sl);
                slowbits |= (sl && idxv[k][r] >= 0) ? (1u << (4 * k + r)) : 0u;
            }
        if (slowbits) {                                                // rare: low-variance windows, rounding boundaries, |q| at or beyond a clamp threshold
#pragma unroll
            for (int k = 0; k < NT; ++k)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if ((slowbits >> (4 * k + r)) & 1u) res[k][r] = ncc_flagged(pv[k][r], sv[k][r], siv[k][r], hc, rT);
        }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (idxv[k][r] >= 0) ccm[idxv[k][r]] = res[k][r];
    if (dbg && tid == 0) dbg[18] = (long long)clock64();
}

template <int S, int PITCH = 0, bool BIG = false>
__device__ __forceinline__ void rp_winner(int ka, const u32 *gs, long long *dbg_cycles)
{
    SID_PHASE_LOCALS;
    __syncthreads();                                                   // the staged operands are complete
    if (dbg_cycles && tid == 0) dbg_cycles[13] = (long long)clock64();
    const double sT = m->sTd[ka], rT = m->rTd[ka];
    const bool cT = m->constT[ka] != 0;
    const int nty = (G.rh + 15) >> 4;
    // pair items first, single items dealt from the other end of the wavefronts (as in the sweep)
    const int n_pair_items = nty * G.npair, n_single_items = nty * G.nsingle;
    // (sum w' kept by the sweep - full table with the sums in LDS and room in the residency class: no all-ones operand)
    const bool ones = rp_pitch_is_gs(PITCH) ? G.gsi == 0 : G.si_off == 0;
    for (int idx = wv; idx < n_pair_items; idx += kWavesM) {
        const int yt = idx / G.npair, xi = idx - yt * G.npair;
        if (ones) rp_winner_item<S, true, PITCH, true, BIG>(16 * yt, 32 * xi, sT, rT, cT, gs, idx == 0 ? dbg_cycles : nullptr);
        else rp_winner_item<S, true, PITCH, BIG, BIG>(16 * yt, 32 * xi, sT, rT, cT, gs, idx == 0 ? dbg_cycles : nullptr);   // (big layouts keep no sum w')
    }
    for (int idx = kWavesM - 1 - wv; idx < n_single_items; idx += kWavesM) {
        if (ones) rp_winner_item<S, false, PITCH, true, BIG>(16 * idx, 32 * G.npair, sT, rT, cT, gs);
        else rp_winner_item<S, false, PITCH, BIG, BIG>(16 * idx, 32 * G.npair, sT, rT, cT, gs);
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// NCC matrix of the winning angle from the accumulators the sweep kept (PMArgs::gs_keep_acc): the exact S_IT' of slot `ka` and
// sum w' (the group's ones slot) of every placement are read back from the point's block of global memory - written by this
// workgroup, still in L2 - and normalised exactly as rp_winner_item does.  No operand staging, no matrix instructions, no
// fragment builds: what is left of the winner is its normalisation.  Same integers, same arithmetic: same matrix bit for bit.
// ---------------------------------------------------------------------------------------------
template <int TS, int SPGK>
__device__ __noinline__ void rp_winner_kept(int ka, const u32 *gs)
{
    SID_SETPRIO_TS(WIN);
    SID_PHASE_LOCALS;
    if (G.hist_off) {                                                  // ph_hessian_fast's histogram + list fill count (as rp_winner_stage_tab)
        for (int idx = tid; idx < 4096 / 16; idx += kBlockM) reinterpret_cast<uint4 *>(smem + G.hist_off)[idx] = make_uint4(0, 0, 0, 0);
        if (tid == 0) m->sel_cle = 0;
    }
    const double sT = m->sTd[ka], rT = m->rTd[ka], nd = G.nd;
    const bool cT = m->constT[ka] != 0;
    const int npos = G.npos, rw = G.rw, prw = G.gsa_rw;
    const u32 magic = G.rw_magic;
    const u32 *acc = gs + G.gsa;
    float *ccm = reinterpret_cast<float *>(smem + G.ccm_off);
    constexpr int kB = 4;                                              // values per thread and batch: independent double-precision chains interleave
    const ncc_norm::Hoisted hc = ncc_norm::Hoisted::make(nd, sT, rT);
    for (int base = 0; base < npos; base += kB * kBlockM) {
        int idx[kB], pv[kB], sv[kB]; u32 si[kB]; float res[kB];
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            idx[u] = base + u * kBlockM + tid;
            const int i = idx[u] < npos ? idx[u] : 0;
            // the 16 bytes that hold slot ka, and those of the ones slot (the same with four slot groups): one load each
            const int y = (int)__umulhi((u32)i, magic), x = i - y * rw;
            const u32 o = (u32)(y * prw + x) * (u32)SPGK;
            const uint4 a = *reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned char *>(acc) + ((o + ((u32)ka & ~3u)) << 2));
            const uint4 b = SPGK == 4 ? a : *reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned char *>(acc) + ((o + (u32)(SPGK - 4)) << 2));
            const u32 kr = (u32)ka & 3u;
            pv[u] = (int)(kr == 0 ? a.x : kr == 1 ? a.y : kr == 2 ? a.z : a.w); sv[u] = (int)b.w;
            si[u] = sii_at(gs, i);
        }
        u32 slowbits = 0;
        if (cT) {                                                      // a constant template: 1 everywhere
#pragma unroll
            for (int u = 0; u < kB; ++u) res[u] = 1.0f;
        } else {
#pragma unroll
            for (int u = 0; u < kB; ++u) {
                bool sl;
                res[u] = ncc_fast_nobranch(pv[u], sv[u], si[u], hc, sl);
                slowbits |= (sl && idx[u] < npos) ? (1u << u) : 0u;
            }
            if (slowbits) {                                            // rare: low-variance windows, rounding boundaries, |q| at or beyond a clamp threshold
#pragma unroll
                for (int u = 0; u < kB; ++u)
                    if ((slowbits >> u) & 1u) res[u] = ncc_flagged(pv[u], sv[u], si[u], hc, rT);
            }
        }
#pragma unroll
        for (int u = 0; u < kB; ++u)
            if (idx[u] < npos) ccm[idx[u]] = res[u];
    }
    __syncthreads();
}

// ---- free lists of recycled blocks (PMArgs::ring): bitmaps, kRingWordsPerXcd 64-bit words per XCD (pm_kernel.h) ----
// Agent-scope atomics keep the words consistent whatever XCD their users run on.  No DATA is handed from one owner of a block
// to the next - the new owner writes every entry before it reads it, and the old owner's last read returned before the barrier
// that precedes its push - so relaxed ordering suffices and the push needs no return value.
constexpr u32 kNoBlock = 0xffffffffu;
__device__ __forceinline__ unsigned long long *ring_word(u32 *ring, u32 w) { return reinterpret_cast<unsigned long long *>(ring) + (size_t)w * kRingStride; }
__device__ __forceinline__ unsigned long long ring_peek(u32 *ring, u32 w) { return __hip_atomic_load(ring_word(ring, w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a block for the workgroup whose home word is `home` (xcd * kRingWordsPerXcd + k): its home word, then its XCD's others.
// `peek` = the home word as read first thing in the kernel (that round trip is covered by the geometry arithmetic; a word that
// has changed since only makes the first AND miss, and its return value is the fresh copy)
__device__ __forceinline__ u32 ring_pop(u32 *ring, u32 home, unsigned long long peek, int32_t *diag)
{
    const u32 x0 = home & ~(u32)(kRingWordsPerXcd - 1);
    for (u32 k = 0; k < (u32)kRingWordsPerXcd; ++k) {
        const u32 w = x0 + ((home + k) & (u32)(kRingWordsPerXcd - 1));
        unsigned long long cur = k == 0 ? peek : ring_peek(ring, w);
        while (cur) {
            const u32 bit = (u32)__builtin_ctzll(cur);
            const unsigned long long m = 1ull << bit;
            const unsigned long long prev = __hip_atomic_fetch_and(ring_word(ring, w), ~m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (prev & m) { if (k >= (u32)kRingHomeWords && diag) atomicAdd(diag, 1); return w * 64u + bit; }
            cur = prev & ~m;
        }
    }
    return kNoBlock;
}
__device__ __forceinline__ void ring_push(u32 *ring, u32 block)
{
    (void)__hip_atomic_fetch_or(ring_word(ring, block >> 6), 1ull << (block & 63u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// NaN x 5 / -1 x 3 for an invalid point (pmlib.py:152-154).  A function of uniform arguments, so that the kernel
// keeps no per-lane result address alive (or parked in scratch) from its first lines to its last.
__device__ __noinline__ void rp_write_nan(double *out, int32_t *oij)
{
    const int tid = threadIdx.x;
    if (tid < 5) out[tid] = NAN;
    if (oij && tid < 3) oij[tid] = -1;
}

template <int S, int BAND = 4, int PAIRED = 0, int PITCH = 0, bool BIG = false>
__global__ __launch_bounds__(BAND == 8 ? 256 : kMaxBlockM, BAND == 8 ? 2 : kOccM) void pm_kernel_rp(const PMArgs A)
{
    // (wave priorities: set inside the non-inlined phases - none in this body, see SID_SETPRIO_TS)
    // (three wavefronts per point: 9 window dwords per thread - the pixel dwords of borders up to 23, the class's last - and 5
    // patch dwords cover what 10 + 4 do with four)
    constexpr int kWin = rp_pitch_is_w3(PITCH) ? 9 : 10, kPat = rp_pitch_is_w3(PITCH) ? 5 : 4;
    constexpr bool kPrio = PAIRED == 0 && ((SID_P_PRE) | (SID_P_SWEEP) | (SID_P_POST) | (SID_P_WIN) | (SID_P_HES)) != 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MiscM *m = reinterpret_cast<MiscM *>(smem);
    Geo *G = reinterpret_cast<Geo *>(smem + kGeoOff);
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // one record per launch position: the point's index and inputs in one round trip (uniform address: scalar loads)
    const PointRec *rec = A.rec + blockIdx.x;
    const int pt = rec->pt;
    constexpr int s = S;
    const int K = A.n_angles;

    double *out = A.out + (int64_t)pt * 5;
    int32_t *oij = A.out_ij ? A.out_ij + (int64_t)pt * 3 : nullptr;
    // recycled blocks (PMArgs::ring; compiled into the kernels that keep accumulators): lane 0 of the LAST wavefront takes its
    // ticket first thing - the atomic's round trip is covered by the geometry arithmetic below - and the block before the
    // first barrier
    constexpr bool POOL = rp_pitch_is_gs(PITCH) && !BIG;             // (every launch that keeps per-placement tables in global memory may take recycled blocks)
    const bool pooled = POOL && A.ring != nullptr;
    const bool popper = pooled && tid == (int)blockDim.x - 64;
    u32 stack = 0; unsigned long long peek = 0;
    if (popper) {
        // home word: this XCD (HW_REG_XCC_ID; a block is then written and read through ONE XCD's L2 as long as the workgroup
        // stays there - it does, slot_life.hip - and nothing breaks if it does not), one of its first kRingHomeWords by launch position
        stack = (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u) * (u32)kRingWordsPerXcd + (((u32)blockIdx.x >> 3) & (u32)(kRingHomeWords - 1));
        peek = ring_peek(A.ring, stack);
    }
    // chained launch (PMArgs::chain): this workgroup's arrival, counted once, by the lane that waits for a round trip here
    // anyway - lane 0 of the last wavefront, pool or no pool; the add goes out while the peek above is in flight.  Counted
    // and settled HERE, above every return of the kernel: a workgroup that left uncounted would leave a stream waiting for ever
    if (A.chain.count != nullptr && tid == (int)blockDim.x - 64) chain_arrive(A.chain.count, A.chain.release, A.chain.epoch, A.n_launch);
#define SID_STAMP(k) do { if (A.dbg_cycles && tid == 0) A.dbg_cycles[k] = (long long)clock64(); } while (0)
    SID_STAMP(0);

    // ---- window geometry (pmlib.py:200-202) ----
    const double c2fg = rec->c2fg, r2fg = rec->r2fg, border = rec->border;
    const double c1 = rec->c1, r1 = rec->r1;
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
    const int wh = inside ? (int)(r1e - r0) : s + 1, ww = inside ? (int)(c1e - c0) : s + 1;
    // (the general Hessian - hes_smth / mcc_norm, several groups of angles - wants LDS of its own for the magnitudes)
    const bool own_hes = K > kAnglesPerGroup || (A.flags & 6u) != 0u;
    constexpr bool GS = rp_pitch_is_gs(PITCH);                        // sum w'^2 per placement in global memory (else LDS)
    static_assert(!BIG || (GS && PAIRED == 0 && BAND == 4), "big layouts: the full-table 4-row kernel with the run-time pitch");
    const RpLdsLayout L = rp_lds_layout(wh, ww, s, K <= kAnglesPerGroup, PAIRED ? 4 * rp_ngroups(PAIRED) : BAND, rp_pitch_bytes(PITCH), rp_tab_pitch(PAIRED), own_hes, GS, BIG);
    if ((PAIRED && K > kSlots / rp_ngroups(PAIRED) - 1) ||             // (the launcher checked)
        !inside || L.total > A.lds_bytes || L.wpitch != (rp_pitch_bytes(PITCH) ? rp_pitch_bytes(PITCH) : L.wpitch)) {   // (the launch was sized by classify_points)
        if (inside && tid == 0 && A.refused) atomicAdd(A.refused, 1);  // host and device disagree about the layout: an error
        // (no block was taken yet)
        rp_write_nan(out, oij);
        return;
    }
    const int rh = wh - s + 1, rw = ww - s + 1, npos = rh * rw;
    // the image-1 patch travels with the window when it lies inside image 1 and its LDS region is clear of the
    // column sums (borders up to 28 for s = 34)
    const int pr0 = (int)floor(r1) - L.pradius, pc0 = (int)floor(c1) - L.pradius;
    const bool patch_early = fabs(r1) < 1e9 && fabs(c1) < 1e9 && (BIG || L.patch_off >= L.u_off + wh * rw * 4) && pr0 >= 0 && pc0 >= 0 &&
                             pr0 + L.pdim <= A.rows1 && pc0 + L.ppitch <= A.cols1 && L.pdim * (L.ppitch >> 2) <= kPat * (int)blockDim.x;
    if (tid == 0) {
        G->band = L.wrows - wh + 1;                                    // ph_window writes wh + band - 1 rows
        G->wh = wh; G->ww = ww; G->rh = rh; G->rw = rw; G->npos = npos; G->wpitch = L.wpitch; G->arow = L.tab_pitch;
        G->gpitch = 0; G->arow0 = L.tab_pitch; G->tab_rows = L.tab_rows; G->ones_slot = kSlots / rp_ngroups(PAIRED) - 1;
        G->s = s; G->K = K;
        G->win_off = L.win_off; G->sii_off = L.sii_off; G->u_off = L.u_off; G->patch_off = L.patch_off;
        G->hes_off = L.hes_off; G->ccm_off = L.ccm_off; G->si_off = L.si_off; G->lin = (int)((A.flags >> 3) & 7u); G->pre = A.pre ? (unsigned long long)(A.pre + (size_t)pt * K * s * s) : 0ull;
        // (full table with the sums in global memory: the point's block holds sum w' behind sum w'^2 - pm_capi.hip sizes it so)
        G->gsi = (GS && !BIG && A.gs_keep_si) ? (u32)round_up(npos, 64) : 0;
        // (kept accumulators - one group of angles, launch by launch, PMArgs::gs_keep_acc: the table follows sum w'^2, and sum w'
        // is its ones slot)
        G->gsa = 0; G->gsa_rw = 0;
        if (GS && !BIG && PAIRED != 0 && A.gs_keep_acc && K <= kAnglesPerGroup) {
            int cp, rpad;
            rp_acc_dims(rh, rw, PAIRED ? 4 * rp_ngroups(PAIRED) : BAND, cp, rpad);
            G->gsa = round_up(npos, 64); G->gsa_rw = cp; G->gsi = 0;
        }
        G->ppitch = L.ppitch; G->pdim = L.pdim; G->pradius = L.pradius; G->queue_off = L.queue_off;
        G->trow_bytes = L.trow_bytes; G->queue_cap = L.queue_cap;
        G->wp_off = L.wp_off; G->wp_pitch = L.wp_pitch; G->wp_rows = L.wp_rows; G->strip_off = L.strip_off;
        G->wrows = L.wrows; G->npair = L.npair; G->nsingle = L.nsingle;
        if (rp_sweep_ragged_ok(PAIRED)) {                              // (the other kernels sweep the tiling above)
            const RpSweepItems I = rp_sweep_items(rh, rw, BAND, true);
            G->sw_npair = I.npair; G->sw_rem = I.rem; G->sw_nsing = I.n_single_items;
        }
        // 5 KB for the Hessian's histogram and key list behind the NCC matrix of the winning angle, when the winner is
        // staged from the operand table (one group of angles) and the fused Hessian may run (no hes_smth / mcc_norm)
        const int hist_off = BIG ? L.u_off + 2 * L.trow_bytes : L.ccm_off + round_up(rh * rw * 4, 16);
        G->hist_off = (K <= kAnglesPerGroup && !(GS && own_hes) && hist_off + 5120 <= L.total) ? hist_off : 0;
        G->pr0 = pr0; G->pc0 = pc0;
        G->win_magic = 0xffffffffu / (u32)((ww + 3) >> 2) + 1u; G->patch_magic = 0xffffffffu / (u32)(L.ppitch >> 2) + 1u;
        G->rw_magic = 0xffffffffu / (u32)rw + 1u;
        G->r0 = r0; G->c0 = c0; G->c1 = c1; G->r1 = r1; G->nd = (double)(s * s);
        m->zero_flag = 0; m->gmax_key = 0x007fffffu /* f2key(-inf) */; m->qcount = 0; m->any_const = 0;
        for (int k = 0; k < 5; ++k) m->gw[k] = A.gauss_w[k];
        if (BIG) G->big = (unsigned long long)(A.gsii + (size_t)rec->gsii_off * 64u);   // the point's block of global memory (as `gs` below)
        if (!pooled) { G->blk = -1; G->blk_xcd = 0; }
    }
    if (popper) { G->blk = (int)ring_pop(A.ring, stack, peek, A.refused ? A.refused + 1 : nullptr); G->blk_xcd = (int)stack; }   // ((int)kNoBlock = -1 with pooled: every word of the XCD empty)
    __syncthreads();
    if (pooled && G->blk < 0) {                                        // no block anywhere: refuse the point, loudly
        if (tid == 0 && A.refused) atomicAdd(A.refused, 1);
        rp_write_nan(out, oij);
        return;
    }
    // this point's sum w'^2 values: its LDS, or (gs launches) the block of global memory of its launch position.  The base
    // address goes through readfirstlane: it then lives in scalar registers and every access is "scalar base + 32-bit lane
    // offset" (with the base in vector registers the 64-bit address arithmetic of the loads cost 3.7 % more VALU instructions)

    if (patch_early) ph_window_t<true, kPrio ? SID_P_PRE : -1, kWin, kPat>(A.img2, A.rows2, A.cols2, A.stride2, A.img1, A.rows1, A.cols1, A.stride1);
    else ph_window_t<false, kPrio ? SID_P_PRE : -1, kWin, kPat>(A.img2, A.rows2, A.cols2, A.stride2, nullptr, 0, 0, 0);
    __syncthreads();
    u32 *gs = !GS ? reinterpret_cast<u32 *>(smem + L.sii_off)
            : pooled ? A.pool + (size_t)(u32)__builtin_amdgcn_readfirstlane(G->blk) * A.pool_stride
                     : A.gsii + (size_t)(u32)__builtin_amdgcn_readfirstlane((int)rec->gsii_off) * 64u;
    SID_STAMP(1);
    SID_STAMP(16);
#ifndef SID_ABLATE_SUMS
    rp_sums<S, GS, BIG>(gs);                                                   // ends with a barrier: the row sums are dead
#endif
    SID_STAMP(2);
    if (!patch_early) ph_patch(A.img1, A.rows1, A.cols1, A.stride1);

    const uint16_t *samp = (A.samp && table_usable(*G, A.rows1, A.cols1)) ? A.samp : nullptr;
    Score sc{-INFINITY, -INFINITY, 0x7fffffff};
    for (int a0 = 0; a0 < K; a0 += kAnglesPerGroup) {
        const int Kg = (K - a0) < kAnglesPerGroup ? (K - a0) : kAnglesPerGroup;
        rp_tpl_begin<S, rp_tab_shift(PAIRED)>(A.rot, a0, Kg, A.dbg_cycles);                  // (barrier inside: patch and WP complete)
#ifndef SID_ABLATE_TPL
        if (samp && A.samp2) rp_tpl_table2<S, rp_tab_shift(PAIRED)>(A.samp2, a0, Kg);
        else if (samp) rp_tpl_table<S, rp_tab_shift(PAIRED)>(samp, a0, Kg);
        else rp_tpl_general<S, rp_tab_shift(PAIRED)>(a0, Kg, A.rows1, A.cols1);
        if (samp && A.samp_nflag > 0) rp_tpl_fix<S, rp_tab_shift(PAIRED)>(samp, a0, Kg, A.rows1, A.cols1);
#endif
        rp_tpl_end<S, rp_tab_shift(PAIRED)>(a0, Kg, A.dbg_templates, A.dbg_cycles);
        if (m->zero_flag) {                                            // pmlib.py:152-154
            if (popper) ring_push(A.ring, (u32)G->blk);
            rp_write_nan(out, oij);
            if (A.dbg_shape && tid == 0) { A.dbg_shape[0] = rh; A.dbg_shape[1] = rw; }
            return;
        }
        SID_STAMP(3);
#ifdef SID_DBG_CHECK
        rp_dbg_check<S, rp_tab_shift(PAIRED)>(Kg, 0, pt, A.dbg_err, A.img1, A.rows1, A.cols1, A.stride1);
#endif
#ifndef SID_ABLATE_SWEEP
        sc = rp_sweep<S, BAND, PAIRED, PITCH>(sc, a0, Kg, gs, A.dbg_cycles);
#else
        sc.bestv = 0.5f; sc.bestkey = 17;
#endif
#ifdef SID_DBG_CHECK
        rp_dbg_check<S, rp_tab_shift(PAIRED)>(Kg, 1, pt, A.dbg_err, A.img1, A.rows1, A.cols1, A.stride1);
#endif
        SID_STAMP(4);
    }

    // ---- block arg-max (first angle, then first row-major index on ties) ----
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
    if (GS && !BIG && PAIRED != 0 && G->gsa != 0) rp_winner_kept<rp_tab_shift(PAIRED), kSlots / rp_ngroups(PAIRED)>(ka, gs);
    else {
        if (K <= kAnglesPerGroup) rp_winner_stage_tab<S, rp_tab_shift(PAIRED)>(ka);
        else rp_winner_stage<S>(A.rot + 4 * ka, samp, A.rows1, A.cols1, ka);
        rp_winner<S, PITCH, BIG>(ka, gs, A.dbg_cycles);
    }
#endif
    SID_STAMP(6);
    if (A.dbg_shape && tid == 0) { A.dbg_shape[0] = rh; A.dbg_shape[1] = rw; }
#ifndef SID_ABLATE_HESSIAN
    if ((A.flags & 6u) == 0u && G->hist_off != 0) ph_hessian_fast<kPrio ? SID_P_HES : -1, BIG>(A.flags, iy, ix, best_r, A.dbg_ccm, A.dbg_hes, A.dbg_cap, A.dbg_cycles);
    else ph_hessian<kPrio ? SID_P_HES : -1, BIG>(A.flags, iy, ix, best_r, A.dbg_ccm, A.dbg_hes, A.dbg_cap, A.dbg_cycles);
#endif
    SID_STAMP(7);
    // the block goes back to its XCD's list: its last reader was the winner's matrix, which ended with a barrier
    if (popper) ring_push(A.ring, (u32)G->blk);
    if (tid == 0) {
        // (reloaded rather than kept in registers - or parked in scratch - through the whole kernel)
        const double c2fg_e = *reinterpret_cast<const volatile double *>(A.c2fg + pt);
        const double r2fg_e = *reinterpret_cast<const volatile double *>(A.r2fg + pt);
        const int ww_e = G->ww, wh_e = G->wh;
        double c2 = c2fg_e + ((double)ix - (double)(ww_e - s) / 2.0);
        double r2 = r2fg_e + ((double)iy - (double)(wh_e - s) / 2.0);
        if (A.flags & kSubpixel) { c2 += m->sub[0]; r2 += m->sub[1]; }
        out[0] = c2;
        out[1] = r2;
        out[2] = A.angles[ka];
        out[3] = (double)m->red_f[1];
        out[4] = (double)m->red_f[0];
        if (oij) { oij[0] = iy; oij[1] = ix; oij[2] = ka; }
    }
#undef SID_STAMP
}

// the instantiation of a row of SID_PM_RP_INSTANCES in this translation unit (rows of its register budget only), nullptr: no such row
template <int OCC = kOccM>
PmKernel rp_kernel(int s, int band, int paired, int pitch, bool big)
{
#define SID_ROW(S, BAND, PAIRED, PITCH, ROW_OCC, BIG)                                                         \
    if constexpr (ROW_OCC == OCC) {                                                                           \
        if (s == S && band == BAND && paired == PAIRED && pitch == PITCH && big == BIG) return pm_kernel_rp<S, BAND, PAIRED, PITCH, BIG>; \
    }
    SID_PM_RP_INSTANCES(SID_ROW)
#undef SID_ROW
    return nullptr;
}

}  // namespace

}  // namespace sid
