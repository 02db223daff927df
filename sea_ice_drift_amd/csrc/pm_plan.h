// pm_plan.h - the launch planner of the pattern-matching core: every decision where host and device must agree (kernel
// instantiation, window pitch, residency class, band height, block of global memory, free-list policy, launch order), as pure
// host arithmetic.  No HIP call and no handle: pm_capi.hip turns a Plan into device buffers and a Schedule into stream waits and
// launches, tests/cpp/plan_check.cpp and schedule_check.cpp check their invariants with g++ alone, and estimate_points /
// estimate_run_time - the cost model the shards are cut with - read the same functions.
#ifndef SID_PM_PLAN_H
#define SID_PM_PLAN_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/sid_pm.h"
#include "pm_kernel.h"

namespace sid {
namespace plan {

constexpr bool kRecycleAllDefault = true;    // (round 6: -1.0 % on the 15-angle step, HBM traffic 12.7x -> 10.1x the algorithmic bytes: profiles/r06_ab_recycle_all.txt)
constexpr int kMaxPerCu = 3;
constexpr int kW3MaxLds = 40960;   // every window of pitch 104 that fits four times (borders 20 .. 23 at 34 / 35 px; measured per border: tools/archive/r4_w3.sh)

// The environment switches of the PM core, read in ONE place (read_switches) and handed on by reference.  A plan keeps the set
// it was made with (Plan::sw) and the launches follow that; the four marked "per run" are read where the run happens.
// "A/B runs": no test and no caller sets it - it exists to measure one variant against the other.
struct Switches {
    bool no_w3 = false;             // SID_PM_NO_W3=1: no three-wavefront class (four points per CU, 192 threads per point); the round-3 classes.  tests/test_gpu_launch_classes.py
    int w3_max_lds = kW3MaxLds;     // SID_PM_W3_MAX_LDS=bytes: LDS footprint up to which the three-wavefront class is used.  A/B runs
    bool no_occ4 = false;           // SID_PM_NO_OCC4=1: never the 128-VGPR build of the slot-group kernels (four workgroups per CU).  tests/test_gpu_launch_classes.py
    bool no_big = false;            // SID_PM_NO_BIG=1: no big layouts (every per-placement table in global memory); such windows run the large-window pipeline.  A/B runs
    bool always_gs = false;         // SID_PM_ALWAYS_GS=1: sum w'^2 per placement in global memory for every window shape.  tests/test_gpu_launch_classes.py
    bool no_gs = false;             // SID_PM_NO_GS=1: sum w'^2 in LDS wherever an instantiation without gs exists.  tests/test_gpu_launch_classes.py
    bool no_gsi = false;            // SID_PM_NO_GSI=1: the blocks of global memory do not hold sum w' (the winner multiplies the all-ones operand).  tests/test_gpu_launch_classes.py
    bool no_rp = false;             // SID_PM_NO_RP=1: template sides 34 / 35 run the classic kernel.  The tests of the classic kernel at these sizes
    bool no_paired = false;         // SID_PM_NO_PAIRED=1: no paired slots / slot groups for at most 7 angles (classic and row-pair kernel).  A/B runs
    bool no_quad = false;           // SID_PM_NO_QUAD=1: two slot groups also for at most 3 angles.  A/B runs
    int keep_acc = -1;              // SID_PM_KEEP_ACC=1: kept accumulators in every gs launch, =0: never; -1 (unset): the slot-group layouts.  tests/test_gpu_keep_acc.py
    bool no_band8 = false;          // SID_PM_NO_BAND8=1: the two-per-CU class runs 4-row bands.  A/B runs
    bool no_fixed_pitch = false;    // SID_PM_NO_FIXED_PITCH=1: the run-time window pitch everywhere (gs instantiations).  A/B runs
    bool no_xcd_order = false;      // SID_PM_NO_XCD_ORDER=1: every run of points keeps the caller's order.  A/B runs
    bool all_large = false;         // SID_PM_ALL_LARGE=1: every valid point runs the large-window pipeline.  tests/test_gpu_large_window.py
    bool no_recycle = false;        // SID_PM_NO_RECYCLE=1: a block of global memory per launch position, no free lists.  tests/test_gpu_recycle.py
    bool recycle_all = kRecycleAllDefault;   // SID_PM_RECYCLE_ALL=0: only the launches that keep accumulators take recycled blocks.  tests/test_gpu_recycle.py
    bool no_samp_table = false;     // SID_PM_NO_SAMP_TABLE=1: on-the-fly template sampling (set_points, debug_point).  The tests of the general sampler
    bool samp2 = false;             // SID_PM_SAMP2=1: build the sampling table sorted per angle (set_points).  tests/test_gpu_samp2.py
    int side_by_side = -1;          // per run.  SID_PM_SIDE_BY_SIDE=0 / 1: launches never / always side by side; -1 (unset): side_by_side_rule.  A/B runs
    int side_first = -1;            // per run.  SID_PM_SIDE_FIRST=n: only the first n launches of a long run side by side.  A/B runs
    bool no_chain = false;          // per run.  SID_PM_NO_CHAIN=1: the launches of a long run one after the other, never chained (chain_rule).  tests/test_gpu_chained_launches.py
    bool verbose = false;           // per run.  SID_PM_VERBOSE=1: one line per launch on stderr.  tests/test_gpu_launch_classes.py, bench.py
    bool debug_check = false;       // per run.  SID_PM_DEBUG_CHECK=1: debugging builds compare their sums on the device
    double tail_blend = 0.7;        // SID_DIST_TAIL_BLEND=x: share of the other launches' tails a SHORT run pays (sid_pm_estimate_run_time).  A/B runs
};

inline Switches read_switches()
{
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    Switches w;
    const char *e;
    w.no_w3 = on("SID_PM_NO_W3");
    if ((e = getenv("SID_PM_W3_MAX_LDS"))) w.w3_max_lds = atoi(e);
    w.no_occ4 = on("SID_PM_NO_OCC4");
    w.no_big = on("SID_PM_NO_BIG");
    w.always_gs = on("SID_PM_ALWAYS_GS");
    w.no_gs = on("SID_PM_NO_GS");
    w.no_gsi = on("SID_PM_NO_GSI");
    w.no_rp = on("SID_PM_NO_RP");
    w.no_paired = on("SID_PM_NO_PAIRED");
    w.no_quad = on("SID_PM_NO_QUAD");
    if ((e = getenv("SID_PM_KEEP_ACC"))) w.keep_acc = atoi(e) > 0 ? 1 : 0;
    w.no_band8 = on("SID_PM_NO_BAND8");
    w.no_fixed_pitch = on("SID_PM_NO_FIXED_PITCH");
    w.no_xcd_order = on("SID_PM_NO_XCD_ORDER");
    w.all_large = on("SID_PM_ALL_LARGE");
    w.no_recycle = on("SID_PM_NO_RECYCLE");
    if ((e = getenv("SID_PM_RECYCLE_ALL"))) w.recycle_all = atoi(e) != 0;
    w.no_samp_table = on("SID_PM_NO_SAMP_TABLE");
    w.samp2 = on("SID_PM_SAMP2");
    if ((e = getenv("SID_PM_SIDE_BY_SIDE"))) w.side_by_side = atoi(e) > 0 ? 1 : 0;
    if ((e = getenv("SID_PM_SIDE_FIRST"))) w.side_first = std::max(0, atoi(e));
    w.no_chain = on("SID_PM_NO_CHAIN");
    w.verbose = on("SID_PM_VERBOSE");
    w.debug_check = on("SID_PM_DEBUG_CHECK");
    if ((e = getenv("SID_DIST_TAIL_BLEND"))) w.tail_blend = atof(e);
    return w;
}

// Workgroups of `lds` bytes that fit one CU.  gfx950 hands LDS out in 1280-byte granules (160 KB / 128;
// measured with tools/ubench/lds_granule.hip: 53760 B -> 3 per CU, 53761 B -> 2).
// workgroups of four wavefronts a CU takes at the kernels' register budget (3 wavefronts per SIMD): launch classes beyond
// this differ in nothing.  The row-pair kernel's slot-group layouts (<= 7 angles) have a 128-VGPR build as well, for the
// borders whose LDS footprint fits four times.
// four workgroups per CU need the 128-VGPR build of the row-pair kernel (pm_kernel_rp_occ4.hip): the slot-group layouts only.
// (Round 4 measured it for the full operand table as well - with sum w'^2 in global memory borders 20-26 fit four per CU:
// border 20 +1.6 %, border 26 +5 % against three per CU with the sums in LDS; not shipped.)
// Four points per CU with three wavefronts per point (192 threads: 4 x 3 = the 12 wavefronts of 168 VGPRs a CU holds; pitch code
// 1104: pm_kernel.h rp_pitch_is_w3) - the smallest windows only
inline int w3_max_lds(const Switches &sw) { return sw.no_w3 ? 0 : sw.w3_max_lds; }
inline int max_per_cu(const Switches &sw, bool rp, int rpp) { return (rp && (w3_max_lds(sw) > 0 || (rpp > 0 && !sw.no_occ4))) ? 4 : kMaxPerCu; }

inline int blocks_per_cu(int lds)
{
    constexpr int kLdsGranule = 1280;
    const int granules = (lds + kLdsGranule - 1) / kLdsGranule;
    return granules > 0 ? (max_lds_bytes() / kLdsGranule) / granules : 8;
}

// window geometry of one point, the same arithmetic as the kernel (pmlib.py:200-202)
inline bool window_dims(double c2fg, double r2fg, double border, int s, int64_t rows2, int64_t cols2,
                        int &wh, int &ww, bool *clipped = nullptr)
{
    const int hws = (int)((double)s / 2.0);
    const double r0d = r2fg - hws - border, r1d = r2fg + hws + border + 1;
    const double c0d = c2fg - hws - border, c1d = c2fg + hws + border + 1;
    if (!(fabs(r0d) < 1e15 && fabs(r1d) < 1e15 && fabs(c0d) < 1e15 && fabs(c1d) < 1e15)) return false;
    // NumPy slicing (pmlib.py:200-202): an end past the image is clipped to it; a start of -1 or less is not
    // (NumPy would wrap it and the reference raises), nor is a window that leaves fewer than s + 1 rows or columns
    const int64_t r0 = (int64_t)r0d, r1e = std::min((int64_t)r1d, rows2), c0 = (int64_t)c0d, c1e = std::min((int64_t)c1d, cols2);
    if (!(r0 >= 0 && c0 >= 0 && r1e - r0 >= s + 1 && c1e - c0 >= s + 1))
        return false;
    wh = (int)(r1e - r0); ww = (int)(c1e - c0);
    if (clipped) *clipped = (int64_t)r1d > rows2 || (int64_t)c1d > cols2;
    return true;
}

// Launches of a SHORT run go side by side on the handle's side streams (launch_schedule): all launches of the run together are at
// most kSideRounds rounds of workgroups.  ONE rule for the launcher and for the estimate the shard cuts are made with
// (estimate_run_time); each counts its rounds in its own way, see there.
constexpr double kSideRounds = 16.0;
inline bool side_by_side_rule(const Switches &sw, size_t n_launches, double rounds)
{
    if (n_launches < 2) return false;
    return sw.side_by_side >= 0 ? sw.side_by_side > 0 : rounds <= kSideRounds;
}

// Launches of a LONG run are CHAINED (launch_schedule): launch k + 1 is released when the last workgroup of launch k has STARTED
// (the kernels count their arrival: PMArgs::chain), so it fills the CUs launch k drains and never competes with workgroups
// of launch k that still wait to be dispatched - what made whole launches side by side slower.  The release is a stream wait
// on signal memory, a beta interface of the runtime: the device must report it (hipDeviceAttributeCanUseStreamWaitValue)
// and the handle must have got its signal memory.  SID_PM_SIDE_FIRST (experiments) keeps its own order.
enum ChainReason { kChainYes = 0, kChainSingle, kChainShort, kChainSwitch, kChainNoWaitValue, kChainNoSignalMemory };
inline ChainReason chain_reason(const Switches &sw, size_t n_launches, double rounds, bool can_wait_value, bool have_signal_memory)
{
    if (n_launches < 2) return kChainSingle;
    if (side_by_side_rule(sw, n_launches, rounds) || sw.side_first >= 0) return kChainShort;
    if (sw.no_chain) return kChainSwitch;
    if (!can_wait_value) return kChainNoWaitValue;
    if (!have_signal_memory) return kChainNoSignalMemory;
    return kChainYes;
}
inline bool chain_rule(const Switches &sw, size_t n_launches, double rounds, bool can_wait_value, bool have_signal_memory)
{
    return chain_reason(sw, n_launches, rounds, can_wait_value, have_signal_memory) == kChainYes;
}

// paired: the kernel's two-row-phase sweep for angle sets of at most kPairedMaxAngles (pm_kernel.h)
inline bool use_paired(const Switches &sw, int K) { return K <= kPairedMaxAngles && !sw.no_paired; }

// row-pair kernel (pm_kernel_rp.inc): template sides 34 / 35, any number of angles.  (Up to 7 angles the classic kernel
// pairs its slots - 8 output rows per item - and still loses to the row-pair kernel with half of its slots idle: 200x200
// benchmark, 7 angles, mixed borders 4.59 vs 4.35 ms, border 20 3.28 vs 3.05, border 50 16.2 vs 14.8; 3 angles 4.52 vs 4.25.)
// Decided at every set_points / debug_point; the decision is kept with the handle.
inline bool use_rp(const Switches &sw, int s) { return rp_size_supported(s) && !sw.no_rp; }

// row-pair kernel with at most 7 angles: paired slots (8 output rows per item with the 4-row kernel's registers; the LDS
// layout is that of an 8-row band)
inline int rp_paired(const Switches &sw, int K)
{
    if (K > kPairedMaxAngles || sw.no_paired) return 0;
    return (K <= kQuadMaxAngles && !sw.no_quad) ? 2 : 1;
}

// band argument of rp_lds_layout: output rows per sweep work item
inline int rp_rows(int rpp, int band) { return rpp == 2 ? 16 : rpp == 1 ? 8 : band; }

// own_hes of rp_lds_layout: the general Hessian (hes_smth / mcc_norm, several groups of angles) keeps the magnitudes in LDS of
// their own (as the kernel decides: pm_kernel_rp prologue)
inline bool rp_own_hes(int K, uint32_t flags) { return K > kRpGroup || (flags & (SID_PM_HES_SMTH | SID_PM_MCC_NORM)) != 0u; }

// "may this launch use the 8-row band": ONE predicate for the planner and for estimate_points (classic and row-pair kernels alike)
inline bool band8_ok(const Switches &sw, bool rp, int rpp, int s, int K)
{
    return mfma_band8_supported(s) && !sw.no_band8 && (rp ? !rpp : !use_paired(sw, K));
}

// gs: sum w'^2 per placement in global memory (rp_lds_layout; decided per window shape by shape_class, and what the kernel
// instantiation of the launch's window pitch does: rp_pitch_is_gs)
inline int lds_need(const Switches &sw, bool rp, int rpp, int wh, int ww, int s, int K, uint32_t flags, int band = 4, int pitch = 0, bool gs = true)
{
    if (rp) return rp_lds_layout(wh, ww, s, K <= kRpGroup, rp_rows(rpp, band), rp_pitch_bytes(pitch), rp_tab_pitch(rpp), rp_own_hes(K, flags), gs).total;
    return mfma_lds_layout(wh, ww, s, band, use_paired(sw, K) && band == 4).total;
}

// big layouts (rp_lds_layout): every per-placement table in the point's block of global memory; always the full-table 4-row kernel
inline RpLdsLayout big_layout(int wh, int ww, int s, int K, uint32_t flags)
{
    return rp_lds_layout(wh, ww, s, K <= kRpGroup, 4, 0, 512, rp_own_hes(K, flags), true, true);
}

// Kept accumulators (PMArgs::gs_keep_acc, round 5): the gs launches of a run with ONE group of angles store the sweep's exact
// S_IT' of every slot and placement in the point's block of global memory, and the winner's NCC matrix is a normalisation of
// stored sums.  Default: the slot-group layouts (at most 7 angles - 16 / 32 bytes per placement; the reference's default is 3
// angles); Switches::keep_acc = 1: also the full table (64 bytes per placement), = 0: never.
inline bool keep_acc_policy(const Switches &sw, bool rp, int rpp, int K)
{
    if (!rp || K > kRpGroup) return false;
    if (rpp == 0) return false;                                   // (the full-table kernels do not carry the code: tools/patches/keep_acc_full.patch)
    return sw.keep_acc >= 0 ? sw.keep_acc > 0 : rpp > 0;
}
// ... per launch: four slot groups (at most 3 angles, 16 B per placement) everywhere; two groups (at most 7 angles, 32 B) only
// in the four-per-CU class of the smallest windows - at larger borders the stores cost more than the winner's matrix
// instructions they replace (7 angles, mixed borders: +1.5 % with, -2 % at border 20; Switches::keep_acc = 1 keeps them everywhere)
inline bool keep_acc_launch(const Switches &sw, bool policy, int rpp, bool gs, bool big, int cls)
{
    if (!policy || !gs || big) return false;
    if (rpp == 1 && cls != 4) return sw.keep_acc > 0;
    return true;
}
// u32 entries of the block of a point of that shape in a gs launch.  keep_si: full-table row-pair launches with the sums in
// global memory also keep sum w' there (the winner then multiplies no all-ones operand): rp && !Switches::no_gsi
inline uint32_t block_entries(int rpp, int s, bool keep_si, int wh, int ww, int band, bool keep)
{
    return rp_block_entries(wh - s + 1, ww - s + 1, rp_rows(rpp, band), 16 >> rpp, keep_si, keep);
}

// Class of one window shape: band height of its sweep items, workgroups per CU, LDS bytes (natural window pitch) and - row-pair
// kernel - whether sum w'^2 per placement lives in global memory (gs).  gs costs ~5 % where it changes nothing and buys
// -10 .. -17 % where its smaller footprint lifts the shape into the next residency class, so it is chosen exactly there;
// and wherever only a gs instantiation exists (window pitch above 112, the 8-row-band kernel, the run-time pitch).
struct ShapeClass {
    bool gs;
    int band, cls, lds, nat_pitch;
    bool big = false;               // cls 0, a launch of its own (one workgroup per CU)
    int w3_pitch = 0;               // pitch code of the three-wavefront class (0: not in it)
};
inline ShapeClass shape_class(const Switches &sw, bool rp, int rpp, int wh, int ww, int s, int K, uint32_t flags, bool band8, bool force_gs)
{
    auto eval = [&](bool gs) {
        ShapeClass c{gs, 4, 0, lds_need(sw, rp, rpp, wh, ww, s, K, flags, 4, 0, gs), 0};
        // the two-per-CU class runs the 8-row-band kernel (two wavefronts per SIMD leave it 256 VGPRs); its
        // window carries a few more zero rows, and a point that then no longer fits twice joins the one-per-CU
        // class (a launch of their own for the few points in between costs more than it saves)
        if (band8 && blocks_per_cu(c.lds) == 2) {
            const int need8 = lds_need(sw, rp, rpp, wh, ww, s, K, flags, 8, 0, gs);
            if (blocks_per_cu(need8) >= 2) { c.lds = need8; c.band = 8; c.cls = 2; }
            else c.cls = 1;
        } else c.cls = std::max(1, std::min(max_per_cu(sw, rp, rpp), blocks_per_cu(c.lds)));
        if (rp) c.nat_pitch = rp_lds_layout(wh, ww, s, K <= kRpGroup, rp_rows(rpp, c.band), 0, rp_tab_pitch(rpp), rp_own_hes(K, flags), gs).wpitch;
        return c;
    };
    if (!rp) return eval(false);
    ShapeClass g = eval(true);
    // (no four-per-CU build with gs - except the three-wavefront class of the full table, for the smallest windows)
    // The three-wavefront class: window pitch 104 (borders 20 .. 23), sums in global memory, a footprint that fits four times.
    // (Pitch 112 - borders 24 .. 28 - measured: full table +-0 / +0.5 / +4 %, three angles +1.5 / +-0 %, seven angles +1 %: not
    // instantiated.  Sums in LDS - pitch code 2104, slot groups at borders 20 / 21 - won until the blocks of global memory held
    // sum w' as well; since then the gs form is 1.5 % ahead there too and the code 2104 is no longer instantiated.)
    if (K <= kRpGroup && g.band == 4 && g.nat_pitch <= 104 && !force_gs) {
        const int code = 1000 + rp_class_pitch(g.nat_pitch), need = lds_need(sw, rp, rpp, wh, ww, s, K, flags, 4, code, true);
        if (need <= std::min(w3_max_lds(sw), 32 * 1280) && rp_pitch_instantiated(4, rpp, code)) {
            ShapeClass c = g; c.gs = true; c.cls = 4; c.lds = need; c.w3_pitch = code; return c;
        }
    }
    g.cls = std::min(g.cls, 3);
    if (g.lds > max_lds_bytes() && !sw.no_big) {   // beyond the LDS even so: the tables go to global memory
        const RpLdsLayout B = big_layout(wh, ww, s, K, flags);
        if (B.total <= max_lds_bytes()) return ShapeClass{true, 4, 0, B.total, B.wpitch, true};
    }
    if (force_gs || sw.always_gs) return g;
    // slot groups: since their gs launches keep sum w' for the winner as well, the gs form is ahead at every border (3 / 7 angles,
    // mixed: -0.9 %; borders 25 / 26: -0.8 %; tools/archive/r4_env_ab.sh) - unless the round-3 classes were asked for (no_w3)
    if (rpp > 0 && w3_max_lds(sw) > 0 && !sw.no_gs && !sw.no_gsi) return g;
    ShapeClass l = eval(false);
    if (rpp == 0) l.cls = std::min(l.cls, 3);   // (the full table has no four-per-CU build: more than kRpGroup angles at borders below 16 reach here)
    if (l.band == 8 || l.nat_pitch > 112 || l.lds > max_lds_bytes()) return g;   // (no instantiation without gs)
    // a class the gs footprint reaches only pays where a kernel build exists for it: the four-per-CU build (128 VGPRs) is
    // instantiated for the pitches without gs alone, so gs never buys the step from three to four
    if (!sw.no_gs && g.cls > l.cls) return g;
    return l;
}

// One launch: `count` positions of Plan::order from `offset` on.
struct Bucket {
    int offset;
    int count;
    int lds;                        // largest LDS footprint of its points, bytes
    int band;                       // output rows per sweep work item of this launch (4 or 8)
    int pitch;                      // compile-time window pitch of the row-pair kernel (0: run-time)
    int occ;                        // wavefronts per SIMD of the kernel build (3; 4: the four-per-CU class of the slot-group layouts)
    uint32_t gs_stride = 0;         // largest sum w'^2 block of the launch's points, in u32 entries (gs launches; 0 otherwise)
    bool big = false;               // big layout: every per-placement table in global memory, a launch of its own
    bool keep = false;              // the launch keeps the sweep's accumulators (PMArgs::gs_keep_acc) and takes recycled blocks
    bool pooled = false;            // the launch takes its blocks of global memory from the free lists (PMArgs::ring)
};

// Workgroups per CU and threads per point of a launch, for the launch loop of sid_pm_run and the round count of launch_schedule.
// per_cu: the workgroups a CU holds - what the LDS footprint allows, capped by the kernel build (two wavefronts per SIMD for the
// 8-row band; 3, or 4 for the 128-VGPR build and for the three-wavefront class): the class the cost model reports.
// round_slots: per_cu WITHOUT the cap of the build (4 wherever the LDS fits four times): the round count of side_by_side_rule
// was fitted with this number and keeps it; it exceeds per_cu for classic-kernel and occ-3 launches of small windows.
// threads: 256 per point; 768 when the LDS footprint leaves room for one point per CU only, so that
// the CU still carries 12 wavefronts (3 per SIMD = the register budget).  (Measured for the
// two-per-CU class, border 28: 256 threads 5.8 ms, 384: 9.1, 512: 7.8, 768: 7.8 - six wavefronts per group
// land 2/2/1/1 on the SIMDs, a second group of 168-VGPR wavefronts then no longer fits.)  192: the three-wavefront class.
// (The thread count was decided with a cap of 8 before; it only asks whether one point fits, where every cap agrees.)
struct LaunchShape { int per_cu, round_slots, nthreads; };
inline LaunchShape launch_shape(const Bucket &b, bool rp)
{
    const bool w3 = rp && rp_pitch_is_w3(b.pitch);
    const int fit = std::max(1, blocks_per_cu(b.lds));
    const int per_cu = std::min(b.band == 8 ? 2 : (b.occ == 4 || w3) ? 4 : kMaxPerCu, fit);
    return LaunchShape{per_cu, std::min(b.band == 8 ? 2 : 4, fit), b.band == 8 ? 256 : (fit == 1 ? 768 : w3 ? 192 : 256)};
}

// The order in which a run puts its launches onto streams, decided here and only executed by sid_pm_run.
//
// Launches side by side for SHORT runs.  A full grid is dozens of rounds of workgroups per launch and its launches run one
// after the other (side by side they measured 1-6 % slower: a CU that took a workgroup of a large-window class is lost to
// several small ones, rounds 2-4).  A rank's shard of an 8-GPU run is two or three launches of one to seven rounds each,
// and every launch ends with a half-empty round - a quarter of such a run; side by side the next launch's workgroups fill
// the CUs the previous one drains.  Rule: all launches of a run together are at most kSideRounds rounds of workgroups
// (side_by_side_rule).  The launches keep their order (largest footprint first): launch 0 on the handle's stream, launch k on
// side[(k - 1) % 3], and the handle's stream continues when every side stream is done (the join).
// (Switches::side_first, experiments: only the first n launches of a long run side by side - the large-window classes, a
// round or two of workgroups each - then the join and the rest in sequence.  The order is still reported as a sequence.)
//
// LONG runs are CHAINED (chain_rule): every launch ends with a drain - its last workgroups on a GPU that is otherwise
// emptying - and the next launch of the same stream cannot start before the previous one has COMPLETED.  The starvation
// above needs workgroups of the earlier launch still waiting to be dispatched, so launch k + 1 is released at the moment the
// LAST workgroup of launch k has started (the kernels count their arrival, PMArgs::chain): it fills the drain slot by slot
// and competes with nothing.  The launches alternate between side[0] and side[1]; launch k >= 1 is preceded on its stream
// by a wait for the release word of the launch before it to reach this run's epoch, and stream order adds "launch k - 2 has
// completed": at most two launches in flight.  The last launch counts nothing: nobody waits for its release word.  The
// handle's stream only forks and joins, as side by side - the caller's stream, which may be the legacy default stream, never
// carries a wait.  (A launch without points - the planner makes none - is a plain step on the handle's stream.)
struct LaunchStep {
    int stream = -1;                // -1: the handle's stream; 0..2: side[k]
    bool join_before = false;       // the handle's stream first waits for the side streams used so far
    bool wait_fork = false;         // first use of that side stream in this run: it waits for the fork event
    int wait_release = -1;          // chained: launch index whose release word this launch waits for (-1: none)
    bool counts_arrival = false;    // chained: PMArgs::chain is set - the launch's last-arriving workgroup stores its release word
};
struct Schedule {
    enum Order { kSequence = 0, kSideBySide, kChained };
    Order order = kSequence;
    ChainReason why = kChainSingle;
    bool record_fork = false;       // some step waits for the fork event
    // rounds of workgroups of the run, each launch at the slots its LDS footprint allows (LaunchShape::round_slots, not capped by the
    // kernel build): kSideRounds was fitted with this count, while estimate_run_time counts at the capped per_cu its tails were fitted with
    double rounds = 0;
    std::vector<LaunchStep> steps;  // one per bucket, in bucket order
};
inline Schedule launch_schedule(const Switches &run_sw, const std::vector<Bucket> &buckets, bool rp, bool can_wait_value, bool have_signal_memory)
{
    Schedule S;
    const size_t n = buckets.size();
    for (const Bucket &b : buckets) S.rounds += (double)b.count / (256.0 * launch_shape(b, rp).round_slots);
    const bool side_by_side = side_by_side_rule(run_sw, n, S.rounds);
    S.why = chain_reason(run_sw, n, S.rounds, can_wait_value, have_signal_memory);
    const bool chained = S.why == kChainYes;
    S.order = chained ? Schedule::kChained : side_by_side ? Schedule::kSideBySide : Schedule::kSequence;
    const size_t n_side = side_by_side ? n : run_sw.side_first >= 0 ? std::min(n, (size_t)run_sw.side_first) : 0;
    int last = -1, counting = -1;                                     // chained: the last launch with points; the latest launch so far that counts its arrivals
    if (chained) for (size_t k = 0; k < n; ++k) if (buckets[k].count > 0) last = (int)k;
    unsigned used = 0;
    S.steps.resize(n);
    for (size_t k = 0; k < n; ++k) {
        LaunchStep &st = S.steps[k];
        st.join_before = k == n_side && n_side > 1;
        int side = (k > 0 && k < n_side) ? (int)((k - 1) % 3) : -1;
        if (chained && buckets[k].count > 0) {
            side = (int)(k & 1);
            st.wait_release = counting;
            st.counts_arrival = (int)k != last;
            if (st.counts_arrival) counting = (int)k;
        }
        if (side >= 0) { st.stream = side; st.wait_fork = !(used & (1u << side)); used |= 1u << side; }
    }
    S.record_fork = used != 0;                                        // (= more than one launch side by side, or chained - with a launch that has points)
    return S;
}
// A failure at step k (its wait or its launch) must leave no stream waiting: the release words 0 .. this index get the epoch from
// the host - every word a wait was enqueued on up to and including step k (the launch that would have stored it may be the one
// that failed).  -1: none.
inline int release_upto(const Schedule &S, size_t k)
{
    int upto = -1;
    for (size_t j = 0; j <= k && j < S.steps.size(); ++j) upto = std::max(upto, S.steps[j].wait_release);
    return upto;
}

// What a plan is made from: the resident points (host copies), the sweep, the shape of the current pair, and the kernel
// family decided at set_points (use_rp / rp_paired).
struct PlanInput {
    int64_t n = 0;
    const double *c1 = nullptr, *r1 = nullptr, *c2fg = nullptr, *r2fg = nullptr, *border = nullptr;
    int s = 0, K = 0;
    uint32_t flags = 0;
    int64_t rows1 = 0, cols1 = 0, rows2 = 0, cols2 = 0;
    bool rp = false;
    int rpp = 0;
};

struct Plan {
    Switches sw;                        // the switches it was made with: the launches follow these, not the environment
    std::vector<Bucket> buckets;        // the launches, in launch order
    std::vector<int32_t> order;         // point index of every launch position
    std::vector<uint32_t> goff;         // row-pair kernel: offset of every launch position's block of global memory, in granules of 256 B
    std::vector<PointRec> recs;         // row-pair kernel: one record per launch position (index, block offset, the five inputs)
    // points beyond the launch classes of the one-workgroup-per-point kernels (search window too large for the LDS, clipped by the
    // edge of image 2, template side above 64): each runs the large-window pipeline (pm_large.hip) after the launches of the others
    std::vector<int32_t> large_idx;
    std::vector<int32_t> nan_idx;       // ... and, when NO other kernel of the run exists (template side above 64), the points without a valid window
    uint32_t pool_stride = 0;           // u32 entries per recycled block: the largest block of any launch that takes them (0: no such launch)
    uint64_t gsii_granules = 0;         // granules of 256 B of all blocks of the launch positions together
    bool gs_keep_si = true;             // the blocks of global memory are sized for sum w' as well (row-pair kernel; Switches::no_gsi: not)
    bool gs_keep_acc = false;           // ... or for the sweep's accumulators (PMArgs::gs_keep_acc: keep_acc_policy)
    double info[5] = {0, 0, 0, 0, 0};   // sid_pm_work_info: launches, valid points, multiply-adds, bytes, largest LDS footprint
};

namespace detail {

// Everything the launch needs to know about a point follows from the SHAPE of its search window, and a run has a few
// dozen shapes (one per border): the LDS layouts are evaluated per shape, the points are only binned.
struct Shape {
    int wh = 0, ww = 0;
    int lds = 0, band = 4, cls = 0, nat_pitch = 0, pitch = 0;
    double work = 0.0;                  // placements
    std::vector<int32_t> idx;           // its points, in the caller's order
    bool gs = false, big = false;
    int w3p = 0;
    bool keep = false, large = false, pooled = false;
};

struct Work {
    const PlanInput &in;
    const Switches &sw;
    Plan &out;
    std::vector<Shape> shapes;
    std::vector<int32_t> shape_of;      // shape of every point (0: its window does not lie inside image 2)
    std::vector<int> ord;               // launch order of the shapes
    int lds_max = 0;
    bool keep_si() const { return in.rp && out.gs_keep_si; }
    uint32_t block(const Shape &sh) const
    {
        return sh.big ? (uint32_t)(big_layout(sh.wh, sh.ww, in.s, in.K, in.flags).big_bytes / 4)
                      : block_entries(in.rpp, in.s, keep_si(), sh.wh, sh.ww, sh.band, sh.keep);
    }
};

// step 1: bin the points by the shape of their window; the class of every new shape
inline int bin_points(Work &W, std::string &err)
{
    const PlanInput &in = W.in;
    const Switches &sw = W.sw;
    const int s = in.s, K = in.K;
    const bool rp = in.rp;
    const int rpp = in.rpp;
    const bool band8 = band8_ok(sw, rp, rpp, s, K);
    std::vector<Shape> &shapes = W.shapes;
    std::vector<int32_t> slot_of((size_t)1 << 16, -1);                // (wh, ww) -> shape, direct-mapped on a hash of the pair
    auto find_shape = [&](int wh, int ww) -> int {
        uint32_t h = ((uint32_t)wh * 2654435761u ^ (uint32_t)ww * 40503u) & 0xffffu;
        for (;; h = (h + 1) & 0xffffu) {
            const int k = slot_of[h];
            if (k < 0) { slot_of[h] = (int32_t)shapes.size(); return -1 - (int)h; }
            if (shapes[(size_t)k].wh == wh && shapes[(size_t)k].ww == ww) return k;
        }
    };
    // template sides the one-point kernels do not take: every point with a valid window runs the large-window pipeline
    const bool small_ok = mfma_img_size_supported(s);
    const int lds_min = small_ok ? lds_need(sw, rp, rpp, s + 1, s + 1, s, K, in.flags, 4, 0, false) : 0;
    {   // shape 0: points whose window does not lie inside image 2 (they write NaN at once; minimal footprint)
        Shape z;
        z.lds = lds_min;
        z.cls = std::min(kMaxPerCu, blocks_per_cu(lds_min));          // (NaN writers: any class)
        shapes.push_back(z);
    }
    double macs = 0, bytes = 0, valid = 0;
    W.lds_max = lds_min;
    std::map<std::pair<int, int>, int> clipped_shape;                // windows clipped by the edge of image 2: (wh, ww) -> shape
    W.shape_of = std::vector<int32_t>((size_t)in.n, 0);
    for (int64_t i = 0; i < in.n; ++i) {
        int wh = 0, ww = 0;
        bool clipped = false;
        if (!window_dims(in.c2fg[i], in.r2fg[i], in.border[i], s, in.rows2, in.cols2, wh, ww, &clipped)) { shapes[0].idx.push_back((int32_t)i); continue; }
        if (wh > 65535 || ww > 4000000) {
            char buf[160];
            snprintf(buf, sizeof buf, "point %lld: search window %dx%d too large (65535 rows: a launch dimension of the large-window pipeline)", (long long)i, wh, ww);
            err = buf;
            return SID_PM_ERR_UNSUPPORTED;
        }
        // a window clipped by the bottom / right edge of image 2 (NumPy slicing) has a shape the one-point kernels' layouts were
        // not validated for (as few as two placement rows or columns next to a full-width other axis): such points run the
        // large-window pipeline, whose kernels take any rectangle byte by byte (the benchmark grid never reaches an edge)
        // (one shape per clipped wh x ww, kept apart from the one-point kernels' shapes of the same size; the pipeline itself runs
        // all of its points as one batch of launches - run_large_points)
        int k = -1;
        if (clipped) {
            const auto it = clipped_shape.find(std::make_pair(wh, ww));
            if (it != clipped_shape.end()) k = it->second;
        } else {
            k = find_shape(wh, ww);
        }
        if (k < 0) {
            Shape sh;
            sh.wh = wh; sh.ww = ww;
            sh.work = (double)(wh - s + 1) * (double)(ww - s + 1);
            sh.large = true;
            if (!clipped && small_ok && !sw.all_large) {
                const ShapeClass sc = shape_class(sw, rp, rpp, wh, ww, s, K, in.flags, band8, sw.no_fixed_pitch);
                // a window whose tables do not fit the LDS of one workgroup: the placement space is tiled over the device instead
                if (sc.lds <= max_lds_bytes()) {
                    sh.large = false;
                    sh.lds = sc.lds; sh.band = sc.band; sh.cls = sc.cls; sh.gs = sc.gs; sh.nat_pitch = sc.nat_pitch; sh.big = sc.big; sh.w3p = sc.w3_pitch;
                }
            }
            if (sh.large && !clipped) sh.cls = 1;
            k = (int)shapes.size();
            if (clipped) clipped_shape.emplace(std::make_pair(wh, ww), k);
            shapes.push_back(sh);
        }
        Shape &sh = shapes[(size_t)k];
        if (sh.large) W.out.large_idx.push_back((int32_t)i);
        else sh.idx.push_back((int32_t)i);
        W.shape_of[(size_t)i] = (int32_t)k;
        macs += (double)K * sh.work * s * s;
        // window + bounding box of the rotated template + 5 inputs + outputs
        bytes += (double)wh * ww + 51.0 * 51.0 + 40.0 + 52.0;
        valid += 1;
    }
    if (!small_ok) W.out.nan_idx.swap(shapes[0].idx);                 // no one-point kernel of this template side: the NaN rows are written by lw_write_nan
    const double img_bytes = (double)in.rows1 * in.cols1 + (double)in.rows2 * in.cols2;
    W.out.info[1] = valid;
    W.out.info[2] = macs;
    W.out.info[3] = std::min(bytes, img_bytes + 92.0 * valid);
    return SID_PM_OK;
}

// step 2: launch order of the shapes: biggest footprints (fewest workgroups per CU) first, one launch per (class, band), longest first
inline void sort_shapes(Work &W)
{
    const std::vector<Shape> &shapes = W.shapes;
    for (size_t k = 0; k < shapes.size(); ++k) if (!shapes[k].idx.empty()) W.ord.push_back((int)k);
    std::sort(W.ord.begin(), W.ord.end(), [&](int a, int b) {
        const Shape &x = shapes[(size_t)a], &y = shapes[(size_t)b];
        if (x.cls != y.cls) return x.cls < y.cls;
        if (x.band != y.band) return x.band < y.band;
        if (x.gs != y.gs) return x.gs;                                // (gs first: the larger windows of a class)
        if (x.w3p != y.w3p) return x.w3p > y.w3p;                     // (three-wavefront class: one launch per window pitch)
        if (x.work != y.work) return x.work > y.work;
        return x.idx[0] < y.idx[0];
    });
}

// step 3.  Row-pair kernel: one window pitch per launch, a compile-time constant of the kernel instantiation (every LDS offset of
// the sweep's and the winner's fragment loops is then an immediate).  The pitch of a launch = the smallest instantiated
// pitch that holds the natural pitch of all of its points; if a footprint with that pitch no longer fits its residency
// class, the whole launch keeps the run-time pitch (Switches::no_fixed_pitch: always).
// gs groups take a pitch of 136 or more (or the run-time pitch): those instantiations keep sum w'^2 in global memory.
inline void assign_pitches(Work &W)
{
    const PlanInput &in = W.in;
    const Switches &sw = W.sw;
    if (!in.rp) return;
    std::vector<Shape> &shapes = W.shapes;
    const std::vector<int> &ord = W.ord;
    for (size_t a = 0; a < ord.size();) {
        size_t b = a + 1;
        const Shape &first = shapes[(size_t)ord[a]];
        while (b < ord.size() && shapes[(size_t)ord[b]].cls == first.cls && shapes[(size_t)ord[b]].band == first.band &&
               shapes[(size_t)ord[b]].gs == first.gs && shapes[(size_t)ord[b]].w3p == first.w3p) ++b;
        const bool gs = first.gs;
        int nat = gs ? 136 : 0;
        for (size_t i = a; i < b; ++i) nat = std::max(nat, shapes[(size_t)ord[i]].nat_pitch);
        int pitch = (nat > 0 && !sw.no_fixed_pitch && !first.big) ? rp_class_pitch(nat) : 0;
        if (first.w3p) pitch = first.w3p;                                  // (the three-wavefront class: its own instantiations)
        if (pitch && !rp_pitch_instantiated(first.band, in.rpp, pitch)) pitch = 0;
        for (size_t i = a; i < b && pitch; ++i) {
            const Shape &sh = shapes[(size_t)ord[i]];
            if (sh.wh > 0 && std::min(max_per_cu(sw, in.rp, in.rpp), blocks_per_cu(lds_need(sw, in.rp, in.rpp, sh.wh, sh.ww, in.s, in.K, in.flags, sh.band, pitch, gs))) < first.cls) pitch = 0;
        }
        // (a group without gs that lost its compile-time pitch - it does not happen with the instantiated pitches - runs the
        // run-time-pitch kernel, which is a gs one)
        const bool gs_now = gs || pitch == 0;
        for (size_t i = a; i < b; ++i) {
            Shape &sh = shapes[(size_t)ord[i]];
            sh.pitch = pitch; sh.gs = gs_now;
            if (sh.wh > 0 && !sh.big) sh.lds = lds_need(sw, in.rp, in.rpp, sh.wh, sh.ww, in.s, in.K, in.flags, sh.band, pitch, gs_now);
        }
        a = b;
    }
}

// step 4: kept accumulators per launch class (final here), and recycled blocks (PMArgs::ring): the launches that keep accumulators
// always (their blocks are 3 - 5x larger); the others that keep per-placement tables in global memory with Switches::recycle_all
// (Switches::no_recycle: a block per launch position everywhere)
inline void decide_keep_pooled(Work &W)
{
    const bool rp = W.in.rp;
    for (Shape &sh : W.shapes) {
        sh.keep = rp && sh.wh > 0 && keep_acc_launch(W.sw, W.out.gs_keep_acc, W.in.rpp, sh.gs, sh.big, sh.cls);
        sh.pooled = rp && sh.wh > 0 && sh.gs && !sh.big && !W.sw.no_recycle && (sh.keep || W.sw.recycle_all);
    }
}

// step 5: the launches and the XCD-aware launch order.  Workgroup j of a launch runs on XCD j mod 8 and every XCD has its own L2, so
// within a run of points of equal class and work (= equal border: the order there is the caller's, i.e.
// spatial for a grid) the run is cut into 8 contiguous chunks and chunk c goes to the XCD of slot
// (start + c) mod 8: neighbouring points - whose search windows overlap - meet in the same L2.
// Runs keep their place in the launch (long first), so the load balance across XCDs is unchanged.
inline void build_launches(Work &W)
{
    const PlanInput &in = W.in;
    const std::vector<Shape> &shapes = W.shapes;
    const std::vector<int> &ord = W.ord;
    std::vector<int32_t> &order = W.out.order;
    std::vector<Bucket> &buckets = W.out.buckets;
    order.reserve((size_t)in.n);
    std::vector<int32_t> run;
    int cls_now = -1;                                                 // class of the bucket being filled
    for (size_t a = 0; a < ord.size();) {
        // a run = the shapes of equal (class, band, work): their points in the caller's order
        size_t b = a + 1;
        const Shape &first = shapes[(size_t)ord[a]];
        while (b < ord.size() && shapes[(size_t)ord[b]].cls == first.cls && shapes[(size_t)ord[b]].band == first.band &&
               shapes[(size_t)ord[b]].pitch == first.pitch && shapes[(size_t)ord[b]].work == first.work) ++b;
        const std::vector<int32_t> *src = &first.idx;
        if (b - a > 1) {
            run.clear();
            for (size_t i = a; i < b; ++i) run.insert(run.end(), shapes[(size_t)ord[i]].idx.begin(), shapes[(size_t)ord[i]].idx.end());
            std::sort(run.begin(), run.end());
            src = &run;
        }
        int lds_run = 0;
        for (size_t i = a; i < b; ++i) lds_run = std::max(lds_run, shapes[(size_t)ord[i]].lds);
        W.lds_max = std::max(W.lds_max, lds_run);
        if (buckets.empty() || buckets.back().band != first.band || buckets.back().pitch != first.pitch || cls_now != first.cls)
            buckets.push_back(Bucket{(int)order.size(), 0, 0, first.band, first.pitch,
                                     (in.rp && first.cls >= 4 && rp_pitch_instantiated(first.band, in.rpp, first.pitch, 4)) ? 4 : 3});
        cls_now = first.cls;
        Bucket &bk = buckets.back();
        // (the points without a window - the last run of their class - take no block and leave the launch they join as it is)
        if (first.wh > 0 || bk.count == 0) { bk.big = first.big; bk.keep = first.keep; bk.pooled = first.pooled; }
        bk.count += (int)src->size();
        bk.lds = std::max(bk.lds, lds_run);
        if (in.rp && first.gs)                                        // (launches that keep sum w'^2 in global memory: the largest block)
            for (size_t i = a; i < b; ++i) {
                const Shape &sh = shapes[(size_t)ord[i]];
                if (sh.wh > 0) bk.gs_stride = std::max<uint32_t>(bk.gs_stride, W.block(sh));
            }
        constexpr int64_t kXcd = 8;
        const int64_t L = (int64_t)src->size(), m = (L + kXcd - 1) / kXcd;
        if (!W.sw.no_xcd_order && L >= 4 * kXcd) {
            for (int64_t p = 0; p < m; ++p)                           // slot t = p * 8 + c takes element c * m + p
                for (int64_t c = 0; c < kXcd; ++c) {
                    const int64_t e = c * m + p;
                    if (e < L) order.push_back((*src)[(size_t)e]);
                }
        } else order.insert(order.end(), src->begin(), src->end());
        a = b;
    }
}

// step 6.  Row-pair kernel: every launch position of a launch that keeps per-placement tables in global memory (gs and big launches)
// gets a block of its own there, in 256-byte granules: sum w'^2, then sum w' or the sweep's accumulators (block_entries);
// big layouts: every table of the point.  Points whose launch keeps its sums in LDS get none.  Scratch per run =
// the sum over those points: 14 KB per point at border 20 with sum w', 48 KB with the accumulators of four slot groups,
// 0.6 MB at border 111 (sid_pm.h).
// Pooled launches take their blocks from the per-XCD free lists (PMArgs::ring) instead: kPoolBlocks blocks (1024 per
// XCD) of the largest such block (Plan::pool_stride), whatever the number of points.
inline int assign_blocks(Work &W, std::string &err)
{
    if (!W.in.rp) return SID_PM_OK;
    const std::vector<Shape> &shapes = W.shapes;
    Plan &out = W.out;
    std::vector<uint32_t> gran_shape(shapes.size(), 0u);
    for (size_t k = 1; k < shapes.size(); ++k) {
        const Shape &sh = shapes[k];
        if (sh.big) gran_shape[k] = W.block(sh) / 64u;
        else if (sh.pooled) out.pool_stride = std::max(out.pool_stride, W.block(sh));
        else if (sh.gs) gran_shape[k] = W.block(sh) / 64u;
    }
    out.goff = std::vector<uint32_t>(out.order.size());
    out.recs = std::vector<PointRec>(out.order.size());
    for (size_t p = 0; p < out.order.size(); ++p) {
        const int32_t i = out.order[p];
        out.goff[p] = (uint32_t)out.gsii_granules;
        out.gsii_granules += gran_shape[(size_t)W.shape_of[(size_t)i]];
        out.recs[p] = PointRec{i, out.goff[p], W.in.c1[i], W.in.r1[i], W.in.c2fg[i], W.in.r2fg[i], W.in.border[i]};
    }
    if (out.gsii_granules >= 0xffffffffull) { err = "per-placement tables in global memory beyond 1 TB"; return SID_PM_ERR_UNSUPPORTED; }
    return SID_PM_OK;
}

}  // namespace detail

// Launch classes of the points for a pair whose image 2 has in.rows2 x in.cols2 pixels: LDS footprint -> residency class
// (workgroups per CU) -> one launch per (class, band), XCD-aware order inside.  The footprint depends on the shape
// of image 2 (a window outside the image is a NaN point and gets the minimal footprint), so a pair of another shape needs
// a plan of its own.  Returns SID_PM_OK, or an error code with its text in `err`.
inline int plan_points(const PlanInput &in, const Switches &sw, Plan &out, std::string &err)
{
    out = Plan();
    out.sw = sw;
    out.gs_keep_si = !sw.no_gsi;
    out.gs_keep_acc = keep_acc_policy(sw, in.rp, in.rpp, in.K);
    detail::Work W{in, sw, out, {}, {}, {}};
    if (int rc = detail::bin_points(W, err)) return rc;
    detail::sort_shapes(W);
    detail::assign_pitches(W);
    detail::decide_keep_pooled(W);
    detail::build_launches(W);
    if (int rc = detail::assign_blocks(W, err)) return rc;
    out.info[0] = (double)out.buckets.size();
    out.info[4] = (double)W.lds_max;
    return SID_PM_OK;
}

// Estimated cost of a grid point in nanoseconds of one MI355X, for cutting a set of points into shards of equal cost
// (sea_ice_drift_amd/dist.py).  Not a table per border: the cost follows what the kernel executes for the point - the
// matrix instructions of the sweep (bands x placement tiles x template row pairs, per group of angles), those of the
// winner's NCC matrix, the placements themselves - times a factor for the residency class of its LDS footprint (fewer
// co-resident workgroups hide less latency).  The six constants were fitted to tools/border_cost.py (template side 34, 15
// angles, borders 20..50: within 4 % everywhere); what matters to the sharding are the ratios between points.
// per_cu_out: the launch class (include/sid_pm.h: sid_pm_estimate_residency).  It must describe plan_points exactly
// (square windows inside image 2): the same use_rp / rp_paired / band8_ok / shape_class, from the same switches.
inline void estimate_points(const Switches &sw, const double *border, int64_t n, int s, int K, uint32_t flags, double *cost_ns, int32_t *per_cu_out)
{
    const bool small_ok = mfma_img_size_supported(s);
    // a point of the large-window pipeline (pm_large.hip: batches of up to 64 points, each tiled over the device): the matrix
    // instructions of lw_corr and the per-placement passes, fitted to profiles/r06_large_window_bench_batched.jsonl (11 / 19 / 46 us
    // at borders 112 / 160 / 250 with 15 angles, 9 us at 100 px, 6 us at 65 px: within 40 %); the ~25 launches of a batch
    // (0.15 ms) are priced per batch by sid_pm_estimate_run_time
    auto large_cost = [&](int wn) {
        const double r = (double)(wn - s + 1);
        const double tiles = ceil(r / 64.0) * ceil(r / 16.0) * (double)((K + 15) / 16);
        return 3000.0 + 4.5 * tiles * (double)(s + 3) * (double)((s + 63) / 64);
    };
    const bool rp = use_rp(sw, s);
    const int rpp = rp ? rp_paired(sw, K) : 0;
    const bool band8 = band8_ok(sw, rp, rpp, s, K);
    const int hws = (int)((double)s / 2.0);
    const int groups = (K + kRpGroup - 1) / kRpGroup;
    // round 4 (transposed strip columns, sum w'^2 in global memory where it lifts the residency class): refitted to
    // tools/border_cost.py on the shipped library, one set per kernel family - full table / two / four slot groups - within
    // 2.3 / 4.3 / 7 % of the measured staircase (profiles/r04_border_cost.json)
    struct Fit { double sweep, winner, pos, fixed, two, one, gs, four; };
    static const Fit kFit[3] = {{3.4646e-3, 2.2848e-2, 7.6082e-3, 29.955, 1.1228, 1.2800, 1.06500, 0.88700},
                                {3.9853e-3, 1.7996e-2, 7.6297e-3, 25.686, 1.2348, 1.3287, 0.99236, 0.91000},
                                {2.5923e-3, 1.8513e-2, 6.4734e-3, 24.173, 1.2518, 1.3574, 1.00890, 0.86000}};   // (last column: the three-wavefront class, refitted to tools/archive/r4_w3.sh / r4_w3p.sh)
    const Fit &F = kFit[rpp];
    constexpr double kBigFactor = 1.25;   // every per-placement table through L2 / HBM (measured at borders 70 .. 100: tools/border_cost.py)
    const double kSweep = F.sweep, kWinner = F.winner, kPos = F.pos, kFixed = F.fixed, kTwoPerCu = F.two, kOnePerCu = F.one, kFourPerCu = F.four;
    for (int64_t i = 0; i < n; ++i) {
        const double b = border[i];
        if (per_cu_out) per_cu_out[i] = kMaxPerCu;
        if (!(b >= 0.0 && b < 4096.0)) { if (cost_ns) cost_ns[i] = kFixed; continue; }      // NaN / absurd: a point that writes NaN at once
        const int wn = 2 * hws + 2 * (int)b + 1, r = wn - s + 1;
        if (r < 2) { if (cost_ns) cost_ns[i] = kFixed; continue; }
        double sweep, winner, cls_factor;
        int cls = kMaxPerCu;
        if (!small_ok) {
            if (cost_ns) cost_ns[i] = large_cost(wn);
            if (per_cu_out) per_cu_out[i] = 1 + SID_PM_CLASS_LARGE;
            continue;
        }
        if (rp) {
            const ShapeClass sc = shape_class(sw, rp, rpp, wn, wn, s, K, flags, band8, sw.no_fixed_pitch);   // (the flags decide the Hessian's LDS: rp_own_hes)
            if (sc.lds > max_lds_bytes()) {                               // beyond the LDS of one workgroup: the large-window pipeline
                if (cost_ns) cost_ns[i] = large_cost(wn);
                if (per_cu_out) per_cu_out[i] = 1 + SID_PM_CLASS_LARGE;
                continue;
            }
            const RpLdsLayout L4 = rp_lds_layout(wn, wn, s, K <= kRpGroup, rp_rows(rpp, 4), 0, rp_tab_pitch(rpp), rp_own_hes(K, flags), sc.gs);
            const int per_cu = std::max(1, sc.cls), band = sc.band;            // (big layouts - class 0 - run one workgroup per CU, full table)
            const int rows = sc.big ? 4 : rp_rows(rpp, band), tiles = 2 * L4.npair + L4.nsingle;
            const double per_row_tile = (double)((s + 1) / 2 + s / 2 + 1) / 2.0 + (double)(((s - 32 + 1) / 2) * 2);
            // work items are dealt to the wavefronts of the workgroup: the busiest wavefront sets the pace
            const int nwaves = per_cu == 1 ? 12 : 4;
            // (the sweep's items: rp_sweep_items - ragged single items where the full-table kernels pack the leftover columns of all bands)
            const int sw_units = rp_sweep_items(r, r, rows, rp_sweep_ragged_ok(sc.big ? 0 : rpp)).units;
            const int units = ((sw_units + nwaves - 1) / nwaves) * nwaves, wunits = ((((r + 15) / 16) * tiles + nwaves - 1) / nwaves) * nwaves;
            sweep = groups * (sc.big ? 1.0 : rpp == 2 ? 0.33 : rpp == 1 ? 0.55 : 1.0) * units * (rows * per_row_tile + 2.0);
            winner = wunits * 76.0;
            cls_factor = ((per_cu >= 4 && max_per_cu(sw, rp, rpp) == 4) ? kFourPerCu : per_cu >= 3 ? 1.0 : per_cu == 2 ? kTwoPerCu : kOnePerCu) * (sc.gs ? F.gs : 1.0) * (sc.big ? kBigFactor : 1.0);
            cls = std::max(1, std::min(per_cu, max_per_cu(sw, rp, rpp))) + (sc.gs ? 16 : 0) + (sc.big ? 32 : 0) + (sc.w3_pitch > 1104 ? 64 : 0);   // (+ 64: the second launch of the three-wavefront class)   // (+ 16: the launches that keep sum w'^2 in global memory are launches of their own)
        } else {
            const MfmaLdsLayout L = mfma_lds_layout(wn, wn, s, 4, use_paired(sw, K));
            if (L.total > max_lds_bytes()) {
                if (cost_ns) cost_ns[i] = large_cost(wn);
                if (per_cu_out) per_cu_out[i] = 1 + SID_PM_CLASS_LARGE;
                continue;
            }
            const int per_cu = blocks_per_cu(L.total), ntx = (r + 15) / 16;
            sweep = groups * (double)r * ntx * s * (use_paired(sw, K) ? 0.55 : 1.0) * 1.3;    // one template row per MFMA
            winner = (double)((r + 15) / 16) * ntx * (16 + s - 1) * 2.0;
            cls_factor = per_cu >= 3 ? 1.0 : per_cu == 2 ? kTwoPerCu : kOnePerCu;
            cls = std::max(1, std::min(per_cu, kMaxPerCu));
        }
        if (cost_ns) cost_ns[i] = (kSweep * sweep + kWinner * winner + kPos * (double)r * r + kFixed) * cls_factor;
        if (per_cu_out) per_cu_out[i] = cls;
    }
}

// Estimated kernel time of ONE run over these points (nanoseconds): per launch class the sum of the point costs plus the tail of
// the launch - with 256 x (workgroups per CU) points in flight the last round is half empty on average; the classes with few
// slots run the large borders, whose run times differ by up to 1.5x inside one launch, and end less evenly (fitted to the
// shards tools/shard_sim.py measures: 1.0 / 0.7 / 0.5 / 0.5 rounds for 1 / 2 / 3 / 4 workgroups per CU) - a launch shorter than
// one round still takes a full one; a SHORT run (side_by_side_rule, the launcher's own) ends with ONE tail, the longest, and
// Switches::tail_blend (0.7) of the others; the points of the large-window pipeline run one after the other behind the launches.
// LONG runs are priced as a sequence, although the launcher chains them (chain_rule: the next launch fills the previous one's
// drain): only shards long enough not to be short are affected, rebalance_with_feedback measures those anyway, and the tail
// constants are refitted once tails under chaining have been measured.
inline double estimate_run_time(const Switches &sw, const double *border, int64_t n, int s, int K, uint32_t flags)
{
    if (n <= 0) return 0.0;
    std::vector<double> cost((size_t)n);
    std::vector<int32_t> cls((size_t)n);
    estimate_points(sw, border, n, s, K, flags, cost.data(), cls.data());
    struct Part { double sum = 0, count = 0; };
    Part parts[256];
    for (int64_t i = 0; i < n; ++i) { Part &p = parts[cls[(size_t)i] & 255]; p.sum += cost[(size_t)i]; p.count += 1; }
    static const double kTail[5] = {0.5, 1.0, 0.7, 0.5, 0.5};
    const double blend = sw.tail_blend;
    double large = 0, sum_all = 0, rounds = 0, tail_max = 0, tail_sum = 0, lat_max = 0, seq = 0;
    size_t nparts = 0;
    for (int c = 0; c < 256; ++c) {
        const Part &p = parts[c];
        if (p.count == 0) continue;
        if (c & SID_PM_CLASS_LARGE) { large += p.sum + 150000.0 * ceil(p.count / 64.0); continue; }   // (+ the launches of every batch of 64)
        const int per_cu = std::max(1, c & SID_PM_CLASS_PER_CU);
        const double latency = 256.0 * per_cu * (p.sum / p.count), tail = kTail[std::min(per_cu, 4)] * latency;
        // rounds of workgroups at the workgroups per CU the class REPORTS (capped by the kernel build); launch_schedule counts the slots
        // the LDS footprint allows (LaunchShape::round_slots, up to 4): the tail constants above were fitted with this count, the launcher's rule with that
        ++nparts; sum_all += p.sum; rounds += p.count / (256.0 * per_cu);
        tail_max = std::max(tail_max, tail); tail_sum += tail; lat_max = std::max(lat_max, latency);
        seq += std::max(p.sum + tail, latency);
    }
    double t = seq;
    if (side_by_side_rule(sw, nparts, rounds)) t = std::max(sum_all + tail_max + blend * (tail_sum - tail_max), lat_max);
    return t + large;
}

}  // namespace plan
}  // namespace sid

#endif  // SID_PM_PLAN_H
