// pm_instances.h - every instantiation of the two PM kernels, once; and what the host asks about them.
//
// Plain C++17 without HIP: the planner (pm_plan.h), both kernel translation units and the host checks under tests/cpp include
// the same rows.  The translation units generate their kernel-pointer lookups from them (pm_kernel_classic.h classic_kernel,
// pm_kernel_rp.inc rp_kernel): the numbers of a row are written once and form both the condition and the template arguments.
//
// The ORDER of the rows is the order in which a translation unit emits its kernels; it is kept as it is so that the gfx950
// code objects do not change with an edit that is meant to leave them alone (profiles/kernel_split_code_objects.txt).
#pragma once

namespace sid {

// ---- classic kernel: pm_kernel_mfma<S, BAND, PAIRED> (pm_kernel_classic.h; three wavefronts per SIMD) ----
// S: template side known at compile time, 0: run-time side (2..64).  BAND: output rows per sweep item.  PAIRED: at most
// kPairedMaxAngles angles, slots 8..15 repeat them for the rows four further down.
#define SID_PM_CLASSIC_INSTANCES(X) \
    X(35, 4, true)                  \
    X(0, 4, true)                   \
    X(34, 4, true)                  \
    X(34, 8, false)                 \
    X(35, 8, false)                 \
    X(35, 4, false)                 \
    X(0, 4, false)                  \
    X(34, 4, false)

// ---- row-pair kernel: pm_kernel_rp<S, BAND, PAIRED, PITCH, BIG> (pm_kernel_rp.inc) ----
// PAIRED: 0 = one group of 16 slots, 1 = two groups, 2 = four.  PITCH: compile-time window pitch code (pm_kernel.h rp_pitch_*;
// 0 = run-time pitch).  occ: wavefronts per SIMD of the translation unit that carries the row - 3 pm_kernel_mfma.hip, 4
// pm_kernel_rp_occ4.hip.  BIG: per-placement tables in global memory.  The rows of one side S, then all of them:
#define SID_PM_RP_SIDE_INSTANCES(X, S) \
    X(S, 4, 2, 0, 3, false)            \
    X(S, 4, 2, 168, 3, false)          \
    X(S, 4, 2, 136, 3, false)          \
    X(S, 4, 2, 112, 3, false)          \
    X(S, 4, 2, 104, 3, false)          \
    X(S, 4, 2, 1104, 3, false)         \
    X(S, 4, 1, 0, 3, false)            \
    X(S, 4, 1, 168, 3, false)          \
    X(S, 4, 1, 136, 3, false)          \
    X(S, 4, 1, 112, 3, false)          \
    X(S, 4, 1, 104, 3, false)          \
    X(S, 4, 1, 1104, 3, false)         \
    X(S, 8, 0, 0, 3, false)            \
    X(S, 8, 0, 168, 3, false)          \
    X(S, 8, 0, 136, 3, false)          \
    X(S, 4, 0, 0, 3, false)            \
    X(S, 4, 0, 168, 3, false)          \
    X(S, 4, 0, 1104, 3, false)         \
    X(S, 4, 0, 136, 3, false)          \
    X(S, 4, 0, 112, 3, false)          \
    X(S, 4, 0, 104, 3, false)          \
    X(S, 4, 2, 104, 4, false)          \
    X(S, 4, 2, 112, 4, false)          \
    X(S, 4, 1, 104, 4, false)          \
    X(S, 4, 1, 112, 4, false)
#define SID_PM_RP_INSTANCES(X)       \
    SID_PM_RP_SIDE_INSTANCES(X, 34)  \
    X(34, 4, 0, 0, 3, true)          \
    X(35, 4, 0, 0, 3, true)          \
    SID_PM_RP_SIDE_INSTANCES(X, 35)

// ---- what the host asks ----
constexpr int max_lds_bytes() { return 160 * 1024; }

constexpr bool mfma_img_size_supported(int s) { return s >= 2 && s <= 64; }   // K = 64 template columns per matrix instruction

// template argument S of the classic kernel that serves side s: s where rows name it, else 0 (the run-time side)
constexpr int mfma_side_arg(int s)
{
#define SID_ROW(S, BAND, PAIRED) if (S != 0 && S == s) return S;
    SID_PM_CLASSIC_INSTANCES(SID_ROW)
#undef SID_ROW
    return 0;
}
constexpr bool mfma_instantiated(int side_arg, int band, bool paired)
{
#define SID_ROW(S, BAND, PAIRED) if (S == side_arg && BAND == band && PAIRED == paired) return true;
    SID_PM_CLASSIC_INSTANCES(SID_ROW)
#undef SID_ROW
    return false;
}
constexpr bool mfma_band8_supported(int s) { return mfma_instantiated(s, 8, false); }

constexpr bool rp_instantiated(int s, int band, int paired, int pitch, int occ, bool big)
{
#define SID_ROW(S, BAND, PAIRED, PITCH, OCC, BIG) \
    if (S == s && BAND == band && PAIRED == paired && PITCH == pitch && OCC == occ && BIG == big) return true;
    SID_PM_RP_INSTANCES(SID_ROW)
#undef SID_ROW
    return false;
}
// true when launch_pm_rp carries an instantiation with this compile-time window pitch (0 = run-time pitch: always) and
// register budget (occ = 3 wavefronts per SIMD, or 4).  Both sides carry the same rows.  Slot groups (paired != 0) have
// four-row bands only, and with three wavefronts per SIMD the band asked for is not looked at for them - the planner never
// pairs them with another, and launch_pm_rp refuses it.
constexpr bool rp_pitch_instantiated(int band, int paired, int pitch, int occ = 3)
{
    return rp_instantiated(34, (occ == 3 && paired != 0) ? 4 : band, paired, pitch, occ, false);
}

}  // namespace sid
