// pm_kernel_phases.h - the phases that the classic kernel (pm_kernel_classic.h) and the row-pair kernel (pm_kernel_rp.inc) share.
//
// Holds: ph_window_t (search window of image 2 -> LDS, optionally with the image-1 patch in the same round trip), ph_patch, the
// template sampler's helpers (SampleGeom, sample_geom, sample_exact, sample_fast5, gather_quad, table_usable), the five-dword
// window fragment (Raw5, read_raw, align_raw), ph_subpixel, ph_hessian, hypot_spec / hypot_fast, ph_hessian_fast and chain_arrive.
// Needs: pm_kernel_base.h (and through it SID_PM_OCC).
#pragma once
#include "pm_kernel_base.h"

namespace sid {

namespace {

// ---------------------------------------------------------------------------------------------
// Phase 0a: search window of image 2 -> LDS, re-centred to int8 (w ^ 0x80), zero beyond the window.
// Loads are issued four dwords deep before any is consumed (HBM/L2 latency overlaps).
// ---------------------------------------------------------------------------------------------
// PATCH: the image-1 patch (ph_patch's fast path; the caller checked that it lies inside image 1 and that its LDS
// region is free already) is fetched in the same round trip: its loads are issued before the window's.
// PRIO >= 0: the wave priority of the phases up to the sweep, set here - inside a non-inlined phase - rather than in the kernel
// body (pm_kernel_rp.inc: SID_SETPRIO_TS)
// (the image bytes of a point are read once by its workgroup, and neighbouring points re-read the overlap within microseconds;
// loading them non-temporally, so that they do not push the recycled blocks' dirty lines out of L2, is tools/patches/img_nt.patch)
template <bool PATCH, int PRIO = -1, int KWIN = 10, int KPAT = 4>
__device__ __noinline__ void ph_window_t(const uint8_t *img2, long long rows2, long long cols2, long long stride2,
                                         const uint8_t *img1, long long rows1, long long cols1, long long stride1)
{
    if (PRIO >= 0) __builtin_amdgcn_s_setprio(PRIO);
    SID_PHASE_LOCALS;
    constexpr int kPat = KPAT;                                         // patch dwords per thread and trip (ph_patch)
    u32 plo[kPat] = {}, phi[kPat] = {}, psh[kPat] = {};
    const int pdw = G.ppitch >> 2, pndw = G.pdim * pdw;
    if (PATCH) {
        const u32 pmagic = G.patch_magic;
        const int pst = (int)stride1;
        const uint8_t *porg = img1 + (long long)G.pr0 * stride1 + G.pc0;
        const u32 pmis = (u32)(reinterpret_cast<uintptr_t>(porg) & 3);
        const uintptr_t porg4u = reinterpret_cast<uintptr_t>(porg) - pmis;                       // (scalar, as the window's origin below)
        const uint8_t *porg4 = reinterpret_cast<const uint8_t *>(((uintptr_t)(u32)__builtin_amdgcn_readfirstlane((int)(porg4u >> 32)) << 32) |
                                                                 (uintptr_t)(u32)__builtin_amdgcn_readfirstlane((int)(u32)porg4u));
        const long long plast_ll = (long long)((reinterpret_cast<uintptr_t>(img1 + (rows1 - 1) * stride1 + cols1) - 1) & ~(uintptr_t)3) -
                                   (long long)reinterpret_cast<uintptr_t>(porg4);
        const u32 plast = plast_ll > 0x7ffffff0ll ? 0x7ffffff0u : (u32)plast_ll;
#pragma unroll
        for (int u = 0; u < kPat; ++u) {
            const int idx = u * kBlockM + tid;
            const int idc = idx < pndw ? idx : 0;
            const int row = (int)__umulhi((u32)idc, pmagic);
            const int dq = idc - row * pdw;
            const u32 o = (u32)(row * pst + 4 * dq) + pmis;
            const u32 oa = o & ~3u;
            const u32 ob = oa + 4 <= plast ? oa + 4 : plast;
            psh[u] = o & 3u;
            plo[u] = *reinterpret_cast<const u32 *>(porg4 + oa);
            phi[u] = *reinterpret_cast<const u32 *>(porg4 + ob);
        }
    }
    uint8_t *win = smem + G.win_off;
    const int wpitch = G.wpitch, ww = G.ww, wh = G.wh;
    // Only the dwords that hold pixels are loaded: dwr per window row.  The rest of the pitch (the class pitch of the row-pair
    // kernels is 104 .. 136 bytes for 75 .. 107 pixels) and the band - 1 zero rows below the window are plain LDS stores.
    const int dw_per_row = wpitch >> 2, dwr = (ww + 3) >> 2, ndw = wh * dwr;
    const u32 magic = G.win_magic;                                     // idx / dwr
    const int st = (int)stride2;
    // all addresses as 32-bit offsets from the (dword-aligned) window origin: no 64-bit multiplies, no divisions
    const uint8_t *org = img2 + G.r0 * stride2 + G.c0;
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(org) & 3);
    // (the origin is the same for every thread: kept in scalar registers, so that a load is "scalar base + 32-bit lane offset"
    // and costs no 64-bit address arithmetic per dword)
    const uintptr_t org4u = reinterpret_cast<uintptr_t>(org) - mis;
    const uint8_t *org4 = reinterpret_cast<const uint8_t *>(((uintptr_t)(u32)__builtin_amdgcn_readfirstlane((int)(org4u >> 32)) << 32) |
                                                            (uintptr_t)(u32)__builtin_amdgcn_readfirstlane((int)(u32)org4u));
    const long long last_ll = (long long)((reinterpret_cast<uintptr_t>(img2 + (rows2 - 1) * stride2 + cols2) - 1) & ~(uintptr_t)3) -
                              (long long)reinterpret_cast<uintptr_t>(org4);
    const u32 last_off = last_ll > 0x7ffffff0ll ? 0x7ffffff0u : (u32)last_ll;  // offset of the last legal dword
    // kWin dwords per thread and round trip: the common small windows (border <= 23 at 192 threads, <= 32 at 256) load in
    // one trip, i.e. one HBM/L2 latency per point.  A slot no thread of the workgroup has a dword for is skipped (uniform).
    constexpr int kWin = KWIN;
    const u32 tailmask = (ww & 3) ? (1u << (8 * (ww & 3))) - 1u : 0xffffffffu;
    for (int base = 0; base < ndw; base += kWin * kBlockM) {
        u32 lo[kWin], hi[kWin], shv[kWin], mskv[kWin];
        int dstv[kWin];
#pragma unroll
        for (int u = 0; u < kWin; ++u) {
            if (base + u * kBlockM < ndw) {
                const int idx = base + u * kBlockM + tid;
                const int idc = idx < ndw ? idx : 0;
                const int row = dwr > 1 ? (int)__umulhi((u32)idc, magic) : idc;   // (one dword per row - a window of at most 4 columns, side 2 at border 0 -: 2^32 / 1 + 1 is no 32-bit magic)
                const int dq = idc - row * dwr;
                dstv[u] = row * dw_per_row + dq;
                mskv[u] = dq == dwr - 1 ? tailmask : 0xffffffffu;      // (every task holds a pixel; the last of a row ww & 3 of them)
                // the dword that holds the task's first pixel lies inside the image; the one behind it is clamped to the
                // last dword that does (its bytes are then shifted out or masked)
                const u32 o = (u32)(row * st + 4 * dq) + mis;
                const u32 oa = o & ~3u;
                const u32 ob = oa + 4 <= last_off ? oa + 4 : last_off;
                shv[u] = o & 3u;
                lo[u] = *reinterpret_cast<const u32 *>(org4 + oa);
                hi[u] = *reinterpret_cast<const u32 *>(org4 + ob);
            }
        }
        if (base == 0) {
            // zeros, while the loads are in flight.  Behind the pixels of every row: thread = row, its dw_per_row - dwr dwords as
            // one ds_write_b32 (odd dwr) and ds_write_b64 (row-pair kernels: dw_per_row is even); the rows below the window: one run of
            // ds_write_b64, taken from the last thread down (the rows' threads are the first ones)
            const int npad = dw_per_row - dwr;
            const bool p8 = (dw_per_row & 1) == 0;                     // (the classic kernels' pitch is a multiple of 4 only: dword stores)
            for (int row = tid; row < wh; row += kBlockM) {
                u32 *p = reinterpret_cast<u32 *>(win) + row * dw_per_row + dwr;
                int k = 0;
                if (p8 && (dwr & 1)) { if (npad > 0) p[0] = 0u; k = 1; }
                if (p8) for (; k + 1 < npad; k += 2) *reinterpret_cast<uint2 *>(p + k) = make_uint2(0u, 0u);
                else for (; k < npad; ++k) p[k] = 0u;
            }
            const int nzd = (G.band - 1) * dw_per_row;
            if (p8) {
                uint2 *z = reinterpret_cast<uint2 *>(win + wh * wpitch);
                for (int i = kBlockM - 1 - tid; i < (nzd >> 1); i += kBlockM) z[i] = make_uint2(0u, 0u);
            } else {
                u32 *z = reinterpret_cast<u32 *>(win + wh * wpitch);
                for (int i = kBlockM - 1 - tid; i < nzd; i += kBlockM) z[i] = 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < kWin; ++u) {
            if (base + u * kBlockM < ndw) {
                const int idx = base + u * kBlockM + tid;
                if (idx < ndw) reinterpret_cast<u32 *>(win)[dstv[u]] = (__builtin_amdgcn_alignbyte(hi[u], lo[u], shv[u]) ^ 0x80808080u) & mskv[u];
            }
        }
    }
    if (PATCH) {
        uint8_t *patch = smem + G.patch_off;
        if (tid == 0) patch[G.pdim * G.ppitch] = 128;                  // (as ph_patch)
#pragma unroll
        for (int u = 0; u < kPat; ++u) {
            const int idx = u * kBlockM + tid;
            if (idx < pndw) reinterpret_cast<u32 *>(patch)[idx] = __builtin_amdgcn_alignbyte(phi[u], plo[u], psh[u]);
        }
        // (larger patches than kPat * blockDim dwords do not occur: pdim <= 58 for s <= 35, 256 threads)
    }
}

// ---------------------------------------------------------------------------------------------
// Phase 0b: neighbourhood of the template centre on image 1 -> LDS patch (8 byte loads in flight).
// ---------------------------------------------------------------------------------------------
__device__ __noinline__ void ph_patch(const uint8_t *img1, long long rows1, long long cols1, long long stride1)
{
    SID_PHASE_LOCALS;
    uint8_t *patch = smem + G.patch_off;
    const int pdim = G.pdim, ppitch = G.ppitch, np = pdim * pdim;
    const long long pr0 = G.pr0, pc0 = G.pc0;
    if (tid == 0) patch[pdim * ppitch] = 128;                          // spare byte: what a flagged table entry gathers
    if (pr0 >= 0 && pc0 >= 0 && pr0 + pdim <= rows1 && pc0 + ppitch <= cols1) {
        // the patch lies inside image 1 (block-uniform): dword loads re-aligned in registers, 32-bit offsets,
        // division by the row pitch through the precomputed reciprocal
        const int pdw = ppitch >> 2, ndw = pdim * pdw;
        const u32 magic = G.patch_magic;
        const int st = (int)stride1;
        const uint8_t *org = img1 + pr0 * stride1 + pc0;
        const u32 mis = (u32)(reinterpret_cast<uintptr_t>(org) & 3);
        const uint8_t *org4 = org - mis;
        const long long last_ll = (long long)((reinterpret_cast<uintptr_t>(img1 + (rows1 - 1) * stride1 + cols1) - 1) & ~(uintptr_t)3) -
                                  (long long)reinterpret_cast<uintptr_t>(org4);
        const u32 last_off = last_ll > 0x7ffffff0ll ? 0x7ffffff0u : (u32)last_ll;
        for (int base = 0; base < ndw; base += 4 * kBlockM) {
            u32 lo[4], hi[4], shv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * kBlockM + tid;
                const int idc = idx < ndw ? idx : 0;
                const int row = (int)__umulhi((u32)idc, magic);
                const int dq = idc - row * pdw;
                const u32 o = (u32)(row * st + 4 * dq) + mis;
                const u32 oa = o & ~3u;
                const u32 ob = oa + 4 <= last_off ? oa + 4 : last_off;
                shv[u] = o & 3u;
                lo[u] = *reinterpret_cast<const u32 *>(org4 + oa);
                hi[u] = *reinterpret_cast<const u32 *>(org4 + ob);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * kBlockM + tid;
                if (idx < ndw) reinterpret_cast<u32 *>(patch)[idx] = __builtin_amdgcn_alignbyte(hi[u], lo[u], shv[u]);
            }
        }
        return;
    }
    // near the image border: byte loads with clamped coordinates
    for (int base = 0; base < np; base += 8 * kBlockM) {
        uint8_t pv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = base + u * kBlockM + tid;
            const int idc = idx < np ? idx : 0;
            const int pr = idc / pdim, pc = idc - pr * pdim;
            long long gr = pr0 + pr, gc = pc0 + pc;
            gr = gr < 0 ? 0 : (gr > rows1 - 1 ? rows1 - 1 : gr);       // clamped rows/cols are never sampled
            gc = gc < 0 ? 0 : (gc > cols1 - 1 ? cols1 - 1 : gc);
            pv[u] = img1[gr * stride1 + gc];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = base + u * kBlockM + tid;
            if (idx < np) { const int pr = idx / pdim, pc = idx - pr * pdim; patch[pr * ppitch + pc] = pv[u]; }
        }
    }
}

// Rotated-template sampling (reference pmlib.py:105-113; scipy order-0 arithmetic) from the LDS patch.
// Thread -> one template column j and every ngrp-th row.  Fast pass in float32 on patch-relative
// coordinates (one fma per coordinate and sample; branch-free so that several angles interleave);
// whenever the rounding or the image-bounds decision could depend on the last bits (|doubt| < kGuard,
// float error < 2.5e-5) the sample is flagged and redone afterwards with scipy's double arithmetic.
struct SampleGeom {
    const uint8_t *patch; const uint8_t *pre; int ppitch, pr0, pc0, s, ngrp, ig, j; bool act, inside, lin;
    float lo_r, hi_r, lo_c, hi_c;
    double c1, r1, rmax1, cmax1;
};
constexpr float kGuard = 1e-4f;
constexpr int kRowsPerThread = 5;       // rows of one template column a thread samples per chunk

__device__ __forceinline__ SampleGeom sample_geom(const Geo &G, int s, long long rows1, long long cols1, const uint8_t *patch)
{
    SampleGeom g;
    g.patch = patch; g.ppitch = G.ppitch; g.pr0 = G.pr0; g.pc0 = G.pc0; g.s = s;
    g.ngrp = kBlockM / s;
    g.ig = (int)threadIdx.x / s; g.j = (int)threadIdx.x - g.ig * s;
    g.act = g.ig < g.ngrp;
    // whole patch at least one pixel inside image 1: the image-bounds tests can be skipped (block-uniform)
    g.inside = G.pr0 >= 1 && G.pc0 >= 1 && (long long)G.pr0 + G.pdim <= rows1 - 1 && (long long)G.pc0 + G.pdim <= cols1 - 1;
    g.lo_r = (float)(-G.pr0); g.hi_r = (float)(rows1 - 1 - G.pr0);
    g.lo_c = (float)(-G.pc0); g.hi_c = (float)(cols1 - 1 - G.pc0);
    g.c1 = G.c1; g.r1 = G.r1; g.rmax1 = (double)(rows1 - 1); g.cmax1 = (double)(cols1 - 1);
    g.lin = G.lin != 0;
    g.pre = reinterpret_cast<const uint8_t *>(G.pre);
    return g;
}

// exact coordinates of sample (i, j) -> pixel value (0 outside image 1)
// ka = index of the angle in the run's list (needed for pre-sampled templates only: rot_order 2..5)
__device__ __forceinline__ int sample_exact(const SampleGeom &g, const double *rot4, int i, int j, int ka)
{
    if (g.pre) return g.pre[((size_t)ka * g.s + i) * g.s + j];         // sampled from the spline coefficients by lw_presample
    const double cosa = rot4[0], sina = rot4[1];
    const double off0 = g.r1 - rot4[2], off1 = g.c1 - rot4[3];
    double rr = 0.0 + (double)i * cosa;                                // NI_GeometricTransform order (matrix = transform.T)
    rr = rr + (double)j * sina;
    rr = rr + off0;
    double cc = 0.0 + (double)i * (-sina);
    cc = cc + (double)j * cosa;
    cc = cc + off1;
    int v = 0;
    if (rr >= 0.0 && rr <= g.rmax1 && cc >= 0.0 && cc <= g.cmax1) {
        if (g.lin) {
            // rot_order = 1: scipy's spline order 1 (NI_GeometricTransform, mode 'constant', cval 0, uint8 output) - weights
            // (1 - y, y), the four taps accumulated in float64 in the order (0,0) (0,1) (1,0) (1,1) as ((v w_row) w_col), then
            // t > 0 ? t + 0.5 : 0, clamped to 255, truncated.  A tap behind the last image row / column carries the weight 0
            // (the coordinate is then integral) and reads a finite patch byte.  Oracle: get_template_order1, fixture G1b.
            const double fr = floor(rr), fc = floor(cc);
            const double yr = rr - fr, yc = cc - fc;
            const double w0r = 1.0 - yr, w0c = 1.0 - yc;
            const uint8_t *p = g.patch + ((int)fr - g.pr0) * g.ppitch + ((int)fc - g.pc0);
            double t = 0.0;
            t = t + ((double)p[0] * w0r) * w0c;
            t = t + ((double)p[1] * w0r) * yc;
            t = t + ((double)p[g.ppitch] * yr) * w0c;
            t = t + ((double)p[g.ppitch + 1] * yr) * yc;
            t = t > 0.0 ? t + 0.5 : 0.0;
            t = t > 255.0 ? 255.0 : t;
            return (int)t;
        }
        const int ri = (int)floor(rr + 0.5) - g.pr0, ci = (int)floor(cc + 0.5) - g.pc0;
        v = g.patch[ri * g.ppitch + ci];
    }
    return v;
}

// Fast pass for rows ig + (k0..k0+4)*ngrp of column j of one angle.  Returns the doubt bits; sure
// samples are stored and summed, doubtful ones are left to the caller.  Branch-free: a rejected sample
// is handed to `store` with take = false (it writes a scratch byte), so that all the chains of a chunk
// - and of the angles in flight - sit in one basic block and overlap.  INSIDE: the patch lies wholly
// inside image 1, no bounds tests.
template <bool INSIDE, typename Store>
__device__ __forceinline__ u32 sample_fast5(const SampleGeom &g, const double *rot4, bool angle_ok, int k0,
                                            int &st, int &stt, int &sawzero, Store store)
{
    const double cosa = rot4[0], sina = rot4[1];
    const float cf = (float)cosa, sf = (float)sina;
    const float orf = (float)((g.r1 - rot4[2]) - (double)g.pr0), ocf = (float)((g.c1 - rot4[3]) - (double)g.pc0);
    const float fj = (float)g.j, fig = (float)g.ig;
    const float base_r = fmaf(fig, cf, fmaf(fj, sf, orf)) + 0.5f, step_r = (float)g.ngrp * cf;
    const float base_c = fmaf(fig, -sf, fmaf(fj, cf, ocf)) + 0.5f, step_c = -(float)g.ngrp * sf;
    const bool lane_ok = angle_ok && g.act;
    u32 doubt = 0;
#pragma unroll
    for (int u = 0; u < kRowsPerThread; ++u) {
        const int k = k0 + u;
        const int i = g.ig + k * g.ngrp;
        const bool valid = lane_ok && i < g.s;
        const float fk = (float)k;
        const float tr = fmaf(fk, step_r, base_r), tc_ = fmaf(fk, step_c, base_c);   // coordinate + 0.5
        const float flr = floorf(tr), flc = floorf(tc_);
        // doubtful when the coordinate is within kGuard of a rounding boundary
        bool sure = fabsf((tr - flr) - 0.5f) < 0.5f - kGuard && fabsf((tc_ - flc) - 0.5f) < 0.5f - kGuard;
        sure = sure && !g.lin;                                         // (bilinear sampling: every sample takes the float64 route)
        bool in_f = true;
        if (!INSIDE) {
            const float rrf = tr - 0.5f, ccf = tc_ - 0.5f;
            in_f = rrf >= g.lo_r + kGuard && rrf <= g.hi_r - kGuard && ccf >= g.lo_c + kGuard && ccf <= g.hi_c - kGuard;
            const bool out_f = rrf < g.lo_r - kGuard || rrf > g.hi_r + kGuard || ccf < g.lo_c - kGuard || ccf > g.hi_c + kGuard;
            sure = sure && (in_f || out_f);
        }
        const int ri = in_f ? (int)flr : 0, ci = in_f ? (int)flc : 0; // in-image samples always lie inside the patch
        int v = g.patch[ri * g.ppitch + ci];
        v = in_f ? v : 0;
        const bool take = valid && sure;
        doubt |= ((valid && !sure) ? 1u : 0u) << u;
        sawzero |= (take && v == 0) ? 1 : 0;
        store(k, i, v, take);
        const int sv = take ? v - 128 : 0;
        st += sv; stt += sv * sv;
    }
    return doubt;
}

// Table path (integral template centre, patch inside image 1): four samples of one template row through the
// host-built offset table (pm_capi.hip make_samp) -> packed raw pixels j = 4*jq .. 4*jq+3.  A flagged entry
// points at the spare byte behind the patch (128 = re-centred 0); ph_tpl_fix supplies the real sample.
__device__ __forceinline__ u32 gather_quad(const uint8_t *patch, const uint2 e)
{
    return (u32)patch[e.x & 0x7fffu] | ((u32)patch[(e.x >> 16) & 0x7fffu] << 8) |
           ((u32)patch[e.y & 0x7fffu] << 16) | ((u32)patch[(e.y >> 16) & 0x7fffu] << 24);
}
// block-uniform: integral template centre and the patch at least one pixel inside image 1
__device__ __forceinline__ bool table_usable(const Geo &G, long long rows1, long long cols1)
{
    const bool inside = G.pr0 >= 1 && G.pc0 >= 1 && (long long)G.pr0 + G.pdim <= rows1 - 1 && (long long)G.pc0 + G.pdim <= cols1 - 1;
    return inside && G.c1 == floor(G.c1) && G.r1 == floor(G.r1) && fabs(G.c1) < 1e9 && fabs(G.r1) < 1e9;
}

// ---- window fragment of one MFMA tile: five dwords read at the lane's dword-aligned address + v_alignbyte_b32 ----
struct Raw5 { u32 r[5]; };
__device__ __forceinline__ Raw5 read_raw(const uint8_t *p)
{
    const u32 *q = reinterpret_cast<const u32 *>(p);
    Raw5 w;
    w.r[0] = q[0]; w.r[1] = q[1]; w.r[2] = q[2]; w.r[3] = q[3]; w.r[4] = q[4];
    return w;
}
__device__ __forceinline__ v4i align_raw(const Raw5 &w, u32 sh)
{
    v4i b;
    b[0] = (int)__builtin_amdgcn_alignbyte(w.r[1], w.r[0], sh);
    b[1] = (int)__builtin_amdgcn_alignbyte(w.r[2], w.r[1], sh);
    b[2] = (int)__builtin_amdgcn_alignbyte(w.r[3], w.r[2], sh);
    b[3] = (int)__builtin_amdgcn_alignbyte(w.r[4], w.r[3], sh);
    return b;
}

// ---------------------------------------------------------------------------------------------
// SID_PM_SUBPIXEL: the parabolic offsets of the peak (subpixel_fit, pm_kernel.h) from the winner's NCC matrix wherever it lives
// (LDS - the kept-accumulator winner leaves it there like the others - or the point's block of global memory: tab_ptr<BIG>),
// left in m->sub[0..1] for the thread that writes the result row.  First thing in ph_hessian and ph_hessian_fast: every form of
// the winner's matrix ends with a barrier, and ph_hessian smooths the matrix IN PLACE under hes_smth (behind a barrier of its
// own) - the offsets are those of the RAW matrix.  Five loads and two double divisions by one thread; nothing else of MiscM
// that the Hessian code touches lies near m->sub.
// ---------------------------------------------------------------------------------------------
template <bool BIG = false>
__device__ __forceinline__ void ph_subpixel(int iy, int ix)
{
    SID_PHASE_LOCALS;
    if (tid != 0) return;
    double dx, dy;
    subpixel_offsets(tab_ptr<BIG, float>(G, smem, G.ccm_off), G.rh, G.rw, iy, ix, dx, dy);
    m->sub[0] = dx; m->sub[1] = dy;
}

// ---------------------------------------------------------------------------------------------
// Phase 5: Hessian at the peak (pmlib.py:36-59, :167) and the optional MCC normalisation.
// hes aliases sii.  Returns h, r in m->red_f[0..1].
// ---------------------------------------------------------------------------------------------
template <int PRIO = -1, bool BIG = false>
__device__ __noinline__ void ph_hessian(unsigned flags, int iy, int ix, float best_r, float *dbg_ccm, float *dbg_hes,
                                        long long dbg_cap, long long *dbg_cycles)
{
    if (PRIO >= 0) __builtin_amdgcn_s_setprio(PRIO);
    SID_PHASE_LOCALS;
    float *hes = tab_ptr<BIG, float>(G, smem, G.hes_off);
    const float *ccm = tab_ptr<BIG, float>(G, smem, G.ccm_off);
    u32 *hist4 = reinterpret_cast<u32 *>(smem + G.u_off);             // winner operands are dead: 4 KB of histograms
    u32 *medlist = hist4 + 1024;                                       // + 1 KB of keys (2 * trow_bytes >= 5 KB for every s: mfma_lds_layout)
    if (flags & kSubpixel) ph_subpixel<BIG>(iy, ix);
    const int rh = G.rh, rw = G.rw, npos = G.npos;
    float rr = best_r;
    if (flags & 4u) {                                                  // mcc_norm (pmlib.py:171-172): on the unsmoothed matrix
        double cx = 0.0, cxx = 0.0;
        float cmin = INFINITY, cmax = -INFINITY;
        for (int idx = tid; idx < npos; idx += kBlockM) {
            const float c = ccm[idx];
            const double v = (double)c;
            cx += v; cxx += v * v;
            cmin = fminf(cmin, c); cmax = fmaxf(cmax, c);
        }
        block_sum2(cx, cxx, m);
        const float sd = std_from_sums(cx, cxx, npos);
        const float med = block_median_fast(ccm, npos, m, hist4, medlist, f2key(cmin), f2key(cmax));
        rr = (best_r - med) / sd;
    }
    if (flags & 2u) {
        // hes_smth (pmlib.py:46-47): scipy.ndimage.gaussian_filter(ccm, 1) in place - per axis a radius-4
        // kernel in double ('reflect' boundary; centre tap first, then the pairs from the outermost inwards,
        // as scipy's correlate1d does for a symmetric kernel), rounded to float32 after each axis
        float *tmp = hes;                                              // the Hessian buffer is free until the gradient pass
        float *cw = tab_ptr<BIG, float>(G, smem, G.ccm_off);
        const double w4 = m->gw[4], w3 = m->gw[3], w2 = m->gw[2], w1 = m->gw[1], w0 = m->gw[0];
        auto refl = [](int q, int n) { while (q < 0 || q >= n) { if (q < 0) q = -q - 1; if (q >= n) q = 2 * n - 1 - q; } return q; };
        __syncthreads();
        for (int pass = 0; pass < 2; ++pass) {
            const float *src = pass == 0 ? ccm : tmp;
            float *dst = pass == 0 ? tmp : cw;
            const int n = pass == 0 ? rh : rw, stride = pass == 0 ? rw : 1;
            for (int idx = tid; idx < npos; idx += kBlockM) {
                const int y = idx / rw, x = idx - y * rw;
                const int p = pass == 0 ? y : x;
                const float *line = src + (pass == 0 ? x : y * rw);
                double acc = (double)line[p * stride] * w4;
                acc += ((double)line[refl(p - 4, n) * stride] + (double)line[refl(p + 4, n) * stride]) * w0;
                acc += ((double)line[refl(p - 3, n) * stride] + (double)line[refl(p + 3, n) * stride]) * w1;
                acc += ((double)line[refl(p - 2, n) * stride] + (double)line[refl(p + 2, n) * stride]) * w2;
                acc += ((double)line[refl(p - 1, n) * stride] + (double)line[refl(p + 1, n) * stride]) * w3;
                dst[idx] = (float)acc;
            }
            __syncthreads();
        }
    }
    double sx = 0.0, sxx = 0.0;
    float hmin = INFINITY, hmax = -INFINITY;
    {
        // np.gradient twice (unit spacing, one-sided edges) without branches:
        //   g(j) = (f[min(j+1,n-1)] - f[max(j-1,0)]) * (0 < j < n-1 ? 0.5 : 1),  d2(k) = same formula on g
        auto d2 = [&](const float *f, int stride, int k, int n) {
            const int kp = k + 1 < n ? k + 1 : n - 1, km = k > 0 ? k - 1 : 0;
            const int kpp = kp + 1 < n ? kp + 1 : n - 1, kpm = kp > 0 ? kp - 1 : 0;
            const int kmp = km + 1 < n ? km + 1 : n - 1, kmm = km > 0 ? km - 1 : 0;
            const float fa = f[kpp * stride], fb = f[kpm * stride], fc = f[kmp * stride], fd = f[kmm * stride];
            const float gp = (fa - fb) * ((kp > 0 && kp < n - 1) ? 0.5f : 1.0f);
            const float gm = (fc - fd) * ((km > 0 && km < n - 1) ? 0.5f : 1.0f);
            return (gp - gm) * ((k > 0 && k < n - 1) ? 0.5f : 1.0f);
        };
        // Interior placements (two or more away from every edge: 80-90 % of the matrix) need no index clamping
        // and only five reads: g(k+1) = (f[k+2] - f[k]) / 2 and g(k-1) = (f[k] - f[k-2]) / 2 are central differences
        // themselves, d2 = (g(k+1) - g(k-1)) / 2 - the same float32 operations np.gradient performs there.
        // The frame of width two around them takes the general form.  Four placements per thread in flight.
        constexpr int kHes = 4;
        auto emit = [&](int idx, float d2x, float d2y) {
            const double hh = (double)d2x * (double)d2x + (double)d2y * (double)d2y;
            const float hv = (float)sqrt(hh);                          // hypotf: double sqrt, narrowed
            hes[idx] = hv;
            sx += (double)hv; sxx += (double)hv * (double)hv;
            hmin = fminf(hmin, hv); hmax = fmaxf(hmax, hv);
        };
        const int iw = rw - 4, ih = rh - 4;
        if (iw > 0 && ih > 0) {
            const u32 imagic = 0xffffffffu / (u32)iw + 1u;
            const int nin = iw * ih;
            for (int base = 0; base < nin; base += kHes * kBlockM) {
                float d2xv[kHes], d2yv[kHes];
#pragma unroll
                for (int u = 0; u < kHes; ++u) {
                    const int q = base + u * kBlockM + tid;
                    const int qc = q < nin ? q : 0;
                    const int yy = iw > 1 ? (int)__umulhi((u32)qc, imagic) : qc, xx = qc - yy * iw;   // (an interior one column wide: 2^32 / 1 + 1 is no 32-bit magic)
                    const float *f = ccm + (yy + 2) * rw + (xx + 2);
                    const float c = f[0], xr = f[2], xl = f[-2], yd = f[2 * rw], yu = f[-2 * rw];
                    d2xv[u] = ((xr - c) * 0.5f - (c - xl) * 0.5f) * 0.5f;
                    d2yv[u] = ((yd - c) * 0.5f - (c - yu) * 0.5f) * 0.5f;
                }
#pragma unroll
                for (int u = 0; u < kHes; ++u) {
                    const int q = base + u * kBlockM + tid;
                    if (q < nin) { const int yy = iw > 1 ? (int)__umulhi((u32)q, imagic) : q, xx = q - yy * iw; emit((yy + 2) * rw + xx + 2, d2xv[u], d2yv[u]); }
                }
            }
        }
        // frame: rows 0, 1, rh-2, rh-1 in full, columns 0, 1, rw-2, rw-1 of the rows between (everything when the
        // matrix is too small to have an interior)
        const bool has_in = iw > 0 && ih > 0;
        const int nfr = has_in ? 4 * rw + 4 * ih : npos;
        for (int q = tid; q < nfr; q += kBlockM) {
            int y, x;
            if (!has_in) { y = q / rw; x = q - y * rw; }
            else if (q < 4 * rw) { const int rr = q / rw; x = q - rr * rw; y = rr < 2 ? rr : rh - 4 + rr; }
            else { const int e = q - 4 * rw; const int yy = e >> 2, cc = e & 3; y = yy + 2; x = cc < 2 ? cc : rw - 4 + cc; }
            emit(y * rw + x, d2(ccm + y * rw, 1, x, rw), d2(ccm + x, rw, y, rh));
        }
    }
    if (dbg_cycles && tid == 0) dbg_cycles[19] = (long long)clock64();
    __syncthreads();
    if (dbg_ccm || dbg_hes) {
        for (int idx = tid; idx < npos && idx < dbg_cap; idx += kBlockM) {
            if (dbg_ccm) dbg_ccm[idx] = ccm[idx];
            if (dbg_hes) dbg_hes[idx] = hes[idx];
        }
    }
    if (dbg_cycles && tid == 0) dbg_cycles[14] = (long long)clock64();
    float h = hes[iy * rw + ix];
    if (flags & 1u) {
        // one reduction round for the two sums and the key range (instead of one for the sums and one for the range)
        const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
        u32 *red_max = reinterpret_cast<u32 *>(m->red_f);
        const double wsx = wave_sum_dpp_d(sx), wsxx = wave_sum_dpp_d(sxx);
        const u32 wmin = wave_umin_dpp(f2key(hmin)), wmax = ~wave_umin_dpp(~f2key(hmax));
        if (lane == 0) { m->rot[w][0] = wsx; m->rot[w][1] = wsxx; m->red_i[w] = (int)wmin; red_max[w] = wmax; }
        for (int i = tid; i < 1024; i += kBlockM) hist4[i] = 0;
        if (tid == 0) m->sel_cle = 0;
        __syncthreads();
        double tx = 0.0, txx = 0.0;
        u32 kmin = 0xffffffffu, kmax = 0u;
        for (int q = 0; q < kWavesM; ++q) {
            tx += m->rot[q][0]; txx += m->rot[q][1];
            const u32 a = (u32)m->red_i[q], b = red_max[q];
            kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
        }
        const float sd = std_from_sums(tx, txx, npos);
        if (dbg_cycles && tid == 0) dbg_cycles[20] = (long long)clock64();
        const float med = block_median_ranged(hes, npos, m, hist4, medlist, kmin, kmax, dbg_cycles);
        h = (h - med) / sd;
    }
    __syncthreads();
    if (tid == 0) { m->red_f[0] = h; m->red_f[1] = rr; }
    __syncthreads();
}

// hypotf as NumPy's float32 np.hypot evaluates it (glibc: (float)sqrt((double)x * x + (double)y * y)), by a shorter route
// with the same result: sqrt(hh) from v_rsq_f64 and two coupled Newton steps (within ~1 ulp of the correctly rounded
// double); (float) of it equals (float) of the IEEE square root unless a float32 rounding boundary - the middle of the 29
// discarded mantissa bits - lies that close, and those lanes (2.4e-7 of them) take the IEEE route.  Checked on the device
// against the IEEE route by sid_pm_debug_hypot_selftest.
__device__ __forceinline__ float hypot_spec(float x, float y)
{
    const double hh = (double)x * (double)x + (double)y * (double)y;
    return (float)sqrt(hh);
}
// (the same value in float32 arithmetic - error-free squares and a rounding guard - measured no faster: tools/patches/hypot_f32.patch)
__device__ __forceinline__ float hypot_fast(float x, float y)
{
    const double hh = (double)x * (double)x + (double)y * (double)y;
    const double y0 = __builtin_amdgcn_rsq(hh);
    double g = hh * y0, h = 0.5 * y0;
    double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g); h = __builtin_fma(h, r, h);
    r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);                                        // sqrt(hh)
    const u32 lo29 = (u32)__double2loint(g) & 0x1fffffffu;
    // not (1e-30 < hh < 1e30): zero, NaN, and results near the float32 denormal range (other rounding boundaries)
    const bool slow = ((lo29 - (0x10000000u - 64u)) <= 128u) || !(hh > 1e-60 && hh < 1e60);
    float out = (float)g;
    if (slow) out = (float)sqrt(hh);
    return out;
}

// Bucket of a Hessian magnitude (>= 0) in the fixed histogram of ph_hessian_fast: 16 binades 2^-15 .. 2 with 128 buckets
// each (the top 7 mantissa bits, 0.5 % wide); monotone in the value, smaller / larger values clamp to the first / last
// bucket.  2048 16-bit counters packed in pairs (a matrix holds fewer than 65536 values).
constexpr int kHesBuckets = 2048;
__device__ __forceinline__ u32 hes_bucket(u32 bits)
{
    const int b = (int)(bits >> 16) - (112 << 7);
    return (u32)(b < 0 ? 0 : (b > kHesBuckets - 1 ? kHesBuckets - 1 : b));
}

// ---------------------------------------------------------------------------------------------
// Phase 5, short form (hes_norm with neither hes_smth nor mcc_norm - the reference's defaults - and G.hist_off set):
// same values as ph_hessian with two barriers instead of eight.  The magnitudes go into a FIXED log-spaced histogram
// (zeroed by the winner's staging) in the pass that computes them, so that no min / max reduction precedes the
// histogram; every wavefront scans the counters itself (no "wavefront 0 scans, barrier, broadcast"); the elements
// of the bucket holding the middle rank (and of the next non-empty one when the second middle value lies there) are
// compacted and ranked by wavefront 0, which also forms the result.  Buckets too full for the list (massive ties, flat
// matrices, magnitudes below 2^-15) fall back to the radix select.
// ---------------------------------------------------------------------------------------------
template <int PRIO = -1, bool BIG = false>
__device__ __noinline__ void ph_hessian_fast(unsigned flags, int iy, int ix, float best_r, float *dbg_ccm, float *dbg_hes,
                                             long long dbg_cap, long long *dbg_cycles)
{
    if (PRIO >= 0) __builtin_amdgcn_s_setprio(PRIO);
    SID_PHASE_LOCALS;
    float *hes = tab_ptr<BIG, float>(G, smem, G.hes_off);
    const float *ccm = tab_ptr<BIG, float>(G, smem, G.ccm_off);
    u32 *hist = reinterpret_cast<u32 *>(smem + G.hist_off);            // 2048 16-bit counters, zero on entry; m->sel_cle = 0
    u32 *list = hist + 1024;                                           // kMedList keys
    if (flags & kSubpixel) ph_subpixel<BIG>(iy, ix);
    const int rh = G.rh, rw = G.rw, npos = G.npos;
    const bool norm = (flags & 1u) != 0;
    double sx = 0.0, sxx = 0.0;
    {
        auto d2 = [&](const float *f, int stride, int k, int n) {
            const int kp = k + 1 < n ? k + 1 : n - 1, km = k > 0 ? k - 1 : 0;
            const int kpp = kp + 1 < n ? kp + 1 : n - 1, kpm = kp > 0 ? kp - 1 : 0;
            const int kmp = km + 1 < n ? km + 1 : n - 1, kmm = km > 0 ? km - 1 : 0;
            const float fa = f[kpp * stride], fb = f[kpm * stride], fc = f[kmp * stride], fd = f[kmm * stride];
            const float gp = (fa - fb) * ((kp > 0 && kp < n - 1) ? 0.5f : 1.0f);
            const float gm = (fc - fd) * ((km > 0 && km < n - 1) ? 0.5f : 1.0f);
            return (gp - gm) * ((k > 0 && k < n - 1) ? 0.5f : 1.0f);
        };
        auto emit = [&](int idx, float hv) {
            hes[idx] = hv;
            sx += (double)hv; sxx += (double)hv * (double)hv;
            if (norm) { const u32 b = hes_bucket(__float_as_uint(hv)); atomicAdd(&hist[b >> 1], 1u << (16 * (b & 1u))); }
        };
        // Interior placements (two or more away from every edge): g(k+1) = (f[k+2] - f[k]) / 2 and g(k-1) = (f[k] - f[k-2]) / 2
        // are central differences themselves, d2 = (g(k+1) - g(k-1)) / 2 - the float32 operations np.gradient performs there.
        // A thread owns one column and a run of rows and slides down it: the rows y-2 .. y+1 of its column stay in registers
        // (one new vertical read per placement + the two horizontal neighbours) and nothing is divided to find a position.
        // Four placements are in flight (their square-root chains interleave); only the stores are predicated.
        const int iw = rw - 4, ih = rh - 4;
        if (iw > 0 && ih > 0) {
            int nseg = kBlockM / iw; nseg = nseg < 1 ? 1 : (nseg > ih ? ih : nseg);
            const int per = (ih + nseg - 1) / nseg;
            constexpr int kB = 4;
            for (int task = tid; task < iw * nseg; task += kBlockM) {  // (one pass unless the matrix is wider than the workgroup)
                const int seg = task / iw, xx = task - seg * iw;
                const int ya = 2 + seg * per, yb = (ya + per < rh - 2) ? ya + per : rh - 2;
                if (ya >= yb) continue;
                const float *col = ccm + xx + 2;                       // column x = xx + 2
                float ra = col[(ya - 2) * rw], rb = col[(ya - 1) * rw], rc = col[ya * rw], rd = col[(ya + 1) * rw];
                for (int y = ya; y < yb; y += kB) {
                    float e[kB], xl[kB], xr[kB], hvv[kB];
#pragma unroll
                    for (int u = 0; u < kB; ++u) {
                        const int yr = (y + u < rh - 3) ? y + u : rh - 3;   // (rows past the run are read where legal and dropped)
                        const float *f = col + yr * rw;
                        e[u] = f[2 * rw]; xl[u] = f[-2]; xr[u] = f[2];
                    }
                    const float cc[kB] = {rc, rd, e[0], e[1]}, uu[kB] = {ra, rb, rc, rd};
#pragma unroll
                    for (int u = 0; u < kB; ++u) {
                        const float d2x = ((xr[u] - cc[u]) * 0.5f - (cc[u] - xl[u]) * 0.5f) * 0.5f;
                        const float d2y = ((e[u] - cc[u]) * 0.5f - (cc[u] - uu[u]) * 0.5f) * 0.5f;
                        hvv[u] = hypot_fast(d2x, d2y);
                    }
#pragma unroll
                    for (int u = 0; u < kB; ++u)
                        if (y + u < yb) emit((y + u) * rw + xx + 2, hvv[u]);
                    ra = e[0]; rb = e[1]; rc = e[2]; rd = e[3];
                }
            }
        }
        const bool has_in = iw > 0 && ih > 0;
        const int nfr = has_in ? 4 * rw + 4 * ih : npos;
        for (int q0 = 0; q0 < nfr; q0 += 2 * kBlockM) {                // two frame placements per thread in flight
            float hv2[2]; int idx2[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int qq = q0 + u * kBlockM + tid, q = qq < nfr ? qq : 0;
                int y, x;
                if (!has_in) { y = q / rw; x = q - y * rw; }
                else if (q < 4 * rw) { const int rr = q / rw; x = q - rr * rw; y = rr < 2 ? rr : rh - 4 + rr; }
                else { const int e = q - 4 * rw; const int yy = e >> 2, cc = e & 3; y = yy + 2; x = cc < 2 ? cc : rw - 4 + cc; }
                idx2[u] = qq < nfr ? y * rw + x : -1;
                hv2[u] = hypot_fast(d2(ccm + y * rw, 1, x, rw), d2(ccm + x, rw, y, rh));
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) if (idx2[u] >= 0) emit(idx2[u], hv2[u]);
        }
    }
    if (norm) {
        const double wsx = wave_sum_dpp_d(sx), wsxx = wave_sum_dpp_d(sxx);
        if (lane == 0) { m->rot[wv][0] = wsx; m->rot[wv][1] = wsxx; }
    }
    if (dbg_cycles && tid == 0) dbg_cycles[19] = (long long)clock64();
    __syncthreads();                                                   // A: magnitudes, histogram, partial sums
    if (dbg_ccm || dbg_hes) {
        for (int idx = tid; idx < npos && idx < dbg_cap; idx += kBlockM) {
            if (dbg_ccm) dbg_ccm[idx] = ccm[idx];
            if (dbg_hes) dbg_hes[idx] = hes[idx];
        }
    }
    if (dbg_cycles && tid == 0) dbg_cycles[14] = (long long)clock64();
    if (!norm) {
        if (tid == 0) { m->red_f[0] = hes[iy * rw + ix]; m->red_f[1] = best_r; }
        return;
    }
    // ---- every wavefront: the bucket of the middle rank.  Lane l sums the counters of buckets 32 l .. 32 l + 31; the lane
    //      whose range holds rank k1 hands its 32 counters to lanes 0..31 through a private LDS slot, and a second
    //      wavefront prefix sum finds the bucket (two short scans instead of a 32-step search in one lane) ----
    u32 c[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 c4 = *reinterpret_cast<const uint4 *>(hist + 16 * lane + 4 * q);
        c[4 * q] = c4.x; c[4 * q + 1] = c4.y; c[4 * q + 2] = c4.z; c[4 * q + 3] = c4.w;
    }
    u32 tot = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) tot += (c[q] & 0xffffu) + (c[q] >> 16);
    const u32 inc = wave_scan_dpp(tot), exc = inc - tot;
    const bool two = !(npos & 1);
    const u32 k1 = two ? (u32)(npos / 2 - 1) : (u32)(npos / 2);
    const bool mine = k1 >= exc && k1 < inc;                           // exactly one lane
    const int L = (int)__builtin_ctzll(__ballot(mine));                // wavefront-uniform
    u32 *xch = reinterpret_cast<u32 *>(m->rTd) + 16 * wv;             // (1 / sqrt(dT) and sum t' per angle are dead: 1 KB of scratch)
    if (mine) {
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<uint4 *>(xch + 4 * q) = make_uint4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
    }
    const u32 base_e = (u32)__builtin_amdgcn_readlane((int)exc, L);    // values below bucket 32 L
    const u32 pk = xch[(lane & 31) >> 1];
    const u32 cq = lane < 32 ? ((lane & 1) ? pk >> 16 : pk & 0xffffu) : 0u;
    const u32 inc2 = wave_scan_dpp(cq) + base_e, exc2 = inc2 - cq;
    const int J = (int)__builtin_ctzll(__ballot(k1 < inc2));           // first bucket whose inclusive count passes k1
    const u32 bin1 = 32u * (u32)L + (u32)J;
    const u32 before = (u32)__builtin_amdgcn_readlane((int)exc2, J), cnt1 = (u32)__builtin_amdgcn_readlane((int)cq, J);
    // the second middle value of an even-sized set lies in the same bucket unless the first is the bucket's last element;
    // then the next three buckets join the list (the next non-empty one is among them unless the matrix is degenerate)
    const bool need2 = two && !(k1 + 1 - before < cnt1);
    const u32 bin_hi = bin1 + (need2 ? 3u : 0u);
    u32 cnt2 = 0;
    if (need2) {
#pragma unroll
        for (u32 d = 1; d <= 3; ++d) { const u32 bb = bin1 + d; if (bb < (u32)kHesBuckets) cnt2 += (hist[bb >> 1] >> (16 * (bb & 1u))) & 0xffffu; }
    }
    const u32 nlist = cnt1 + cnt2;
    if (dbg_cycles && tid == 0) dbg_cycles[22] = (long long)clock64();
    if (nlist > (u32)kMedList || (need2 && cnt2 == 0u)) {              // block-uniform: massive ties, gaps -> radix select
        double tx = 0.0, txx = 0.0;
        for (int q = 0; q < kWavesM; ++q) { tx += m->rot[q][0]; txx += m->rot[q][1]; }
        const float h = hes[iy * rw + ix];
        const float med = block_median(hes, npos, m, hist);
        if (tid == 0) { m->red_f[0] = (h - med) / std_from_sums(tx, txx, npos); m->red_f[1] = best_r; }
        return;
    }
    for (int i = tid; i < npos; i += kBlockM) {
        const u32 bits = __float_as_uint(hes[i]), b = hes_bucket(bits);
        if (b >= bin1 && b <= bin_hi) list[atomicAdd(&m->sel_cle, 1u)] = bits;  // (non-negative floats order like their bits)
    }
    __syncthreads();                                                   // B: the list is complete
    if (dbg_cycles && tid == 0) dbg_cycles[23] = (long long)clock64();
    if (wv != 0) return;
    // wavefront 0: rank the list (both buckets together: bucket order = value order), pick the middle value(s), finish
    double tx = 0.0, txx = 0.0;
    for (int q = 0; q < kWavesM; ++q) { tx += m->rot[q][0]; txx += m->rot[q][1]; }
    const float h = hes[iy * rw + ix];
    const u32 r1 = k1 - before, r2 = r1 + 1;
    u32 key1 = 0, key2 = 0;
    for (u32 base = 0; base < nlist; base += 64) {
        const u32 j = base + (u32)lane;
        const u32 mv = j < nlist ? list[j] : 0xffffffffu;
        u32 rank = 0;
        for (u32 t0 = 0; t0 < nlist; t0 += 4) {                        // (the list region holds kMedList entries: reads past nlist are harmless)
            const uint4 o = *reinterpret_cast<const uint4 *>(list + t0);
            rank += (t0 + 0 < nlist && (o.x < mv || (o.x == mv && t0 + 0 < j))) ? 1u : 0u;
            rank += (t0 + 1 < nlist && (o.y < mv || (o.y == mv && t0 + 1 < j))) ? 1u : 0u;
            rank += (t0 + 2 < nlist && (o.z < mv || (o.z == mv && t0 + 2 < j))) ? 1u : 0u;
            rank += (t0 + 3 < nlist && (o.w < mv || (o.w == mv && t0 + 3 < j))) ? 1u : 0u;
        }
        const unsigned long long h1 = __ballot(j < nlist && rank == r1), h2 = __ballot(j < nlist && rank == r2);
        if (h1) key1 = (u32)__builtin_amdgcn_readlane((int)mv, (int)__builtin_ctzll(h1));
        if (h2) key2 = (u32)__builtin_amdgcn_readlane((int)mv, (int)__builtin_ctzll(h2));
    }
    const float med = two ? (__uint_as_float(key1) + __uint_as_float(key2)) / 2.0f : __uint_as_float(key1);
    if (dbg_cycles && tid == 0) dbg_cycles[24] = (long long)clock64();
    if (tid == 0) { m->red_f[0] = (h - med) / std_from_sums(tx, txx, npos); m->red_f[1] = best_r; }
}

// ---- chained launches (PMArgs::chain, pm_kernel.h): ONE lane per workgroup counts the workgroup's arrival ----
// chain_count issues the add on the workgroup's shard; chain_settle looks at what it returned.  The shard's last arrival adds
// one to the ninth word, and the arrival that completes the non-empty shards is the launch's last: it puts the zeros back
// (nobody else touches the nine words again in this run) and stores the epoch into the release word.  Relaxed: no payload
// travels with the flag.  Agent scope for the counters; the release word lives in host-visible signal memory: system scope.
// A function of uniform arguments that is NOT inlined: the kernels' prologues keep their register allocation (inlined, the
// same lines cost several instantiations of the row-pair kernel up to five spilled VGPRs: profiles/r09_registers.txt).
__device__ __noinline__ void chain_arrive(u32 *count, unsigned long long *release, unsigned long long epoch, int n_launch)
{
    const int shard = (int)(blockIdx.x & (u32)(kChainShards - 1));
    const u32 before = __hip_atomic_fetch_add(count + shard * kChainLineWords, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((int)before + 1 != chain_shard_count(n_launch, shard)) return;
    const u32 shards = __hip_atomic_fetch_add(count + kChainShards * kChainLineWords, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((int)shards + 1 != chain_nonempty_shards(n_launch)) return;
    for (int k = 0; k <= kChainShards; ++k) __hip_atomic_store(count + k * kChainLineWords, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(release, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

}  // namespace sid
