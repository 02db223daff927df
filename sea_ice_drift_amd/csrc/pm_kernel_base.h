// pm_kernel_base.h - what every phase of the PM kernels (pm_kernel_mfma.hip, pm_kernel_rp_occ4.hip) stands on.
//
// Holds: the LDS header of a workgroup (MiscM at offset 0, the per-point geometry Geo at kGeoOff) and SID_PHASE_LOCALS, which
// gives a non-inlined phase its view of them; tab_ptr; the wavefront reductions on DPP and the block reductions; the medians
// (radix select, ranged and fast forms); the NCC normalisation wrappers (exact_from_sums*, ncc_*: ncc_norm.h with the device's
// seed) and Score / take_better.
// Needs: SID_PM_OCC, set by the translation unit before its first include - the wavefronts per SIMD its kernels' register
// allocation must allow: 3 (168 VGPRs, up to 768 threads) or 4 (128 VGPRs, 256 threads).  A translation unit per budget because
// the register budget of a kernel is handed down to the non-inlined phase functions it calls: instantiated side by side, the
// 128-VGPR kernels slowed the 168-VGPR ones by 0.9 %.
// Everything here is in an anonymous namespace: each translation unit compiles its own copy.  Compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>
#include "pm_kernel.h"
#include "ncc_norm.h"

#if !defined(SID_PM_OCC) || (SID_PM_OCC != 3 && SID_PM_OCC != 4)
#error "define SID_PM_OCC as 3 or 4 before including the PM kernel headers"
#endif

namespace sid {

namespace {

typedef uint32_t u32;
typedef int v4i __attribute__((ext_vector_type(4)));
typedef void (*PmKernel)(const PMArgs);   // either PM kernel

// Threads per grid point are chosen at launch: 256, or 768 for the LDS-footprint class that fits one
// point per CU only (12 wavefronts = 3 per SIMD, the register budget).
constexpr int kOccM = SID_PM_OCC;     // wavefronts per SIMD the register allocation must allow
constexpr int kMaxBlockM = kOccM == 4 ? 256 : 768;
#define kBlockM ((int)blockDim.x)
#define kWavesM ((int)(blockDim.x >> 6))
constexpr int kSlots = 16;           // MFMA M: 15 angles + ones
constexpr int kAnglesPerGroup = kRpGroup;
constexpr float kMargin = 1e-5f;     // pre-filter margin (see the top of pm_kernel_mfma.hip)

struct MiscM {                       // LDS offset 0, kMiscMfmaBytes reserved
    float red_f[16];
    int red_i[16];
    u32 sel_key, sel_cle;
    int zero_flag;
    int best_key; float best_val;
    u32 gmax_key;                    // block-wide running max of the float32 estimates (ordered key)
    u32 qcount;                      // candidate queue fill
    int pad_;
    double gw[5];                    // hes_smth: Gaussian taps (PMArgs::gauss_w)
    int isT[kSlots], isTT[kSlots];   // integer template sums of the current group
    double rot[kSlots][4];           // cos, sin, tcT0, tcT1 of the current group's angles
    double rTd[kMaxAngles];          // 1/sqrt(dT) per angle
    double sTd[kMaxAngles];          // sum t' per angle
    int constT[kMaxAngles];
    // row-pair kernel: float32 pre-filter terms of the current group's slots (pm_kernel_rp.inc), 16-byte aligned:
    // a lane fetches the terms of its four slots with one ds_read_b128 each
    __attribute__((aligned(16))) int nmTi[kSlots];      // -round(S_T' / N)
    __attribute__((aligned(16))) float ncTf[kSlots];    // -(S_T' - N round(S_T' / N)) / N
    __attribute__((aligned(16))) float aTf[kSlots];     // N / sqrt(dT); NaN: constant template; 0: dead slot
    __attribute__((aligned(16))) float biasf[kSlots];   // 0, or -inf for a dead slot
    float maxA;
    int any_const;
    double sub[2];                   // SID_PM_SUBPIXEL: dx, dy of the peak, from the raw NCC matrix of the winning angle (ph_subpixel)
};

// Per-point geometry, written once by thread 0 and read by every phase (the phases are separate
// non-inlined functions so that each gets its own register allocation; their shared state is here).
struct Geo {
    int wh, ww, rh, rw, npos, wpitch, arow, s, K;
    int gpitch, arow0, tab_rows, ones_slot;   // operand-table geometry (mfma_lds_layout) and the all-ones slot: 15, or 7 paired
    int win_off, sii_off, u_off, patch_off, ppitch, pdim, pradius, queue_off, trow_bytes;
    int pr0, pc0;                    // patch origin on image 1
    u32 win_magic;                   // floor(2^32 / dwr) + 1, dwr = (ww + 3) / 4 the pixel dwords of a window row: idx / dwr == umulhi(idx, win_magic) for idx < 2^16 and dwr > 1
    u32 patch_magic, rw_magic;       // same for ppitch/4 and for rw
    int band;                        // output rows per sweep work item (kernel template parameter)
    int wp_off, wp_pitch, wp_rows, strip_off, wrows, npair, nsingle;   // row-pair kernel (RpLdsLayout)
    int sw_npair, sw_rem, sw_nsing;  // row-pair kernel, the SWEEP's work items (rp_sweep_items): pair items per band, leftover columns per band of the ragged tiling (0: today's), single items of the point
    int queue_cap;                   // row-pair kernel: entries of the candidate queue (RpLdsLayout::queue_cap)
    int hes_off, ccm_off;            // Hessian magnitudes and NCC matrix of the winning angle (f32 per placement)
    int si_off;                      // row-pair kernel: sum w' per placement kept from the sweep for the winner (0: none)
    int gsi;                         // ... the same in the point's block of global memory, behind sum w'^2: offset in u32 entries (0: none)
    int hist_off;                    // 5 KB behind the NCC matrix of the winning angle for ph_hessian_fast (0: none - the general ph_hessian runs)
    int gsa, gsa_rw;                 // kept accumulators (PMArgs::gs_keep_acc): offset of the table in the point's block (u32 entries; 0: none) and its row pitch in placements
    int blk, blk_xcd;                // recycled block of this point and its home word of the free lists (PMArgs::ring; blk -1: none)
    int lin;                         // rot_order = 1 (SID_PM_ROT_ORDER1, pmlib.py:89): templates sampled bilinearly, every sample through sample_exact
    long long r0, c0;                // window origin on image 2
    double c1, r1, nd;
    unsigned long long big;          // row-pair kernel, big layouts (rp_lds_layout): the point's block of global memory
    unsigned long long pre;          // rot_order 2..5: this point's K templates in global memory [K][s][s], sampled from the spline coefficients
                                     // of image 1 by lw_presample (pm_large.hip); lin is then 2 and sample_exact loads them (0: none)
};
// per-placement table at `off`: LDS, or - big layouts of the row-pair kernel - the point's block of global memory
template <bool BIG, typename T>
__device__ __forceinline__ T *tab_ptr(const Geo &G, unsigned char *smem, int off)
{
    if constexpr (BIG) return reinterpret_cast<T *>(reinterpret_cast<unsigned char *>(G.big) + (unsigned)off);
    else return reinterpret_cast<T *>(smem + off);
}
constexpr int kGeoOff = 2432;
static_assert(sizeof(MiscM) <= kGeoOff, "misc header too large");
static_assert(kGeoOff + sizeof(Geo) <= kMiscMfmaBytes, "geometry block does not fit the LDS header");

#define SID_PHASE_LOCALS                                                                        \
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];                         \
    [[maybe_unused]] MiscM *m = reinterpret_cast<MiscM *>(smem);                                 \
    [[maybe_unused]] const Geo &G = *reinterpret_cast<const Geo *>(smem + kGeoOff);              \
    [[maybe_unused]] const int tid = threadIdx.x, lane = tid & 63;                               \
    /* wavefront index as a scalar: loops over work items become uniform (SALU counters, scalar branches) */ \
    [[maybe_unused]] const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);                    \
    [[maybe_unused]] const int n_l = lane & 15, q_l = lane >> 4


// ---- wavefront reductions on the VALU (DPP row shifts + row broadcasts, gfx9 encoding): the
// __shfl_* forms go through the LDS crossbar (~100 cycles per step) and were the slowest part of
// the epilogues.  Result is returned in every lane. ----
template <typename Op>
__device__ __forceinline__ int wave_reduce_i32(int v, int ident, Op op) {
    v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1,3
    v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2,3
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int wave_sum_dpp(int v) { return wave_reduce_i32(v, 0, [](int a, int b) { return a + b; }); }
__device__ __forceinline__ float wave_max_dpp(float v) {
    // NaN-free inputs expected (callers map NaN away); float max on the bit patterns via fmaxf
    const int r = wave_reduce_i32(__float_as_int(v), __float_as_int(-INFINITY),
                                  [](int a, int b) { return __float_as_int(fmaxf(__int_as_float(a), __int_as_float(b))); });
    return __int_as_float(r);
}

__device__ __forceinline__ int wave_min_dpp(int v) { return wave_reduce_i32(v, 0x7fffffff, [](int a, int b) { return a < b ? a : b; }); }
__device__ __forceinline__ u32 wave_umin_dpp(u32 v) {
    return (u32)wave_reduce_i32((int)(v ^ 0x80000000u), 0x7fffffff, [](int a, int b) { return a < b ? a : b; }) ^ 0x80000000u;
}
// inclusive prefix sum across the wavefront (same DPP sequence, result per lane)
__device__ __forceinline__ u32 wave_scan_dpp(u32 x) {
    int v = (int)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return (u32)v;
}
template <int CTRL, int RMASK>
__device__ __forceinline__ double dpp_add_step_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, RMASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, RMASK, 0xf, false);
    return v + __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);       // + 0.0 where no source lane
}
__device__ __forceinline__ double wave_sum_dpp_d(double v) {
    v = dpp_add_step_d<0x111, 0xf>(v); v = dpp_add_step_d<0x112, 0xf>(v); v = dpp_add_step_d<0x114, 0xf>(v);
    v = dpp_add_step_d<0x118, 0xf>(v); v = dpp_add_step_d<0x142, 0xa>(v); v = dpp_add_step_d<0x143, 0xc>(v);
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// ---- small block utilities ----

__device__ __forceinline__ u32 block_min(u32 v, MiscM *m) {
    v = wave_umin_dpp(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) m->red_i[threadIdx.x >> 6] = (int)v;
    __syncthreads();
    u32 a = (u32)m->red_i[0];
    for (int w = 1; w < kWavesM; ++w) { const u32 b = (u32)m->red_i[w]; a = a < b ? a : b; }
    return a;
}
__device__ __forceinline__ u32 f2key(float f) { u32 b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float key2f(u32 k) { u32 b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; return __uint_as_float(b); }

// k-th smallest (0-based) of v[0..n) by 4 x 8-bit radix select.  The four histograms are zeroed
// up front (hist4: 4 x 256 counters, 16-byte aligned scratch); per pass: all threads bin their elements (LDS atomics), barrier, wavefront 0 scans the
// 256 bins (4 per lane + a wavefront prefix sum) and publishes the digit, barrier.
__device__ __forceinline__ u32 block_select(const float *v, int n, u32 k, MiscM *m, u32 *hist4, u32 *count_le) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    for (int i = threadIdx.x; i < 1024; i += kBlockM) hist4[i] = 0;
    if (threadIdx.x == 0) { m->sel_key = 0; m->sel_cle = 0; }
    __syncthreads();
    u32 prefix = 0, mask = 0, kk = k, less_total = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        u32 *hist = hist4 + 256 * pass;
        for (int i = threadIdx.x; i < n; i += kBlockM) {
            const u32 key = f2key(v[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (w == 0) {
            const uint4 c4 = *reinterpret_cast<const uint4 *>(hist + 4 * lane);
            const u32 tot = c4.x + c4.y + c4.z + c4.w;
            const u32 inc = wave_scan_dpp(tot);
            const u32 exc = inc - tot;
            if (kk >= exc && kk < inc) {                       // exactly one lane
                u32 e = exc, bin = 4 * lane, cnt = c4.x;
                if (kk >= e + c4.x) { e += c4.x; bin += 1; cnt = c4.y;
                    if (kk >= e + c4.y) { e += c4.y; bin += 1; cnt = c4.z;
                        if (kk >= e + c4.z) { e += c4.z; bin += 1; cnt = c4.w; } } }
                m->sel_key = bin; m->sel_cle = e; m->red_i[0] = (int)cnt;
            }
        }
        __syncthreads();
        const u32 bin = m->sel_key, less = m->sel_cle, cnt = (u32)m->red_i[0];
        prefix |= bin << shift;
        mask |= 255u << shift;
        kk -= less;
        less_total += less;
        if (pass == 3) *count_le = less_total + cnt;
    }
    return prefix;
}

// np.median of a float32 LDS array (mean of the two middle values for even n, float32).
__device__ __forceinline__ float block_median(const float *v, int n, MiscM *m, u32 *hist4) {
    u32 cle;
    if (n & 1) return key2f(block_select(v, n, (u32)(n / 2), m, hist4, &cle));
    const u32 k1 = (u32)(n / 2 - 1);
    const u32 key1 = block_select(v, n, k1, m, hist4, &cle);
    u32 key2 = key1;
    if (cle < k1 + 2) {                                        // next order statistic is a larger value
        u32 mn = 0xffffffffu;
        for (int i = threadIdx.x; i < n; i += kBlockM) { const u32 key = f2key(v[i]); if (key > key1 && key < mn) mn = key; }
        key2 = block_min(mn, m);
    }
    return (key2f(key1) + key2f(key2)) / 2.0f;
}

constexpr int kMedList = 256;
// The part after the key range [kmin, kmax] is known to every thread.  Expects hist[0..1023] = 0 and m->sel_cle = 0, made
// visible by a barrier.
__device__ __forceinline__ float block_median_ranged(const float *v, int n, MiscM *m, u32 *hist, u32 *list, u32 kmin, u32 kmax,
                                                     long long *dbg = nullptr)
{
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u32 range = kmax - kmin;
    const int shift = range < 1024u ? 0 : 22 - __clz(range);           // (range >> shift) < 1024
    for (int i = tid; i < n; i += kBlockM) atomicAdd(&hist[(f2key(v[i]) - kmin) >> shift], 1u);
    __syncthreads();
    if (dbg && tid == 0) dbg[21] = (long long)clock64();
    const bool two = !(n & 1);
    const u32 k1 = two ? (u32)(n / 2 - 1) : (u32)(n / 2);
    if (w == 0) {                                                      // 16 buckets per lane + a wavefront prefix sum
        u32 c[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 c4 = *reinterpret_cast<const uint4 *>(hist + 16 * lane + 4 * q);
            c[4 * q] = c4.x; c[4 * q + 1] = c4.y; c[4 * q + 2] = c4.z; c[4 * q + 3] = c4.w;
        }
        u32 tot = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) tot += c[q];
        const u32 inc = wave_scan_dpp(tot), exc = inc - tot;
        if (k1 >= exc && k1 < inc) {                                   // exactly one lane
            u32 e = exc, bin = 16 * lane, cnt = 0;
            bool found = false;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (!found) { if (k1 < e + c[q]) { found = true; bin = 16 * lane + q; cnt = c[q]; } else e += c[q]; }
            }
            m->sel_key = bin; m->red_i[14] = (int)e; m->red_i[15] = (int)cnt;
        }
    }
    __syncthreads();
    if (dbg && tid == 0) dbg[22] = (long long)clock64();
    const u32 bin = m->sel_key, before = (u32)m->red_i[14], cnt = (u32)m->red_i[15];
    if (cnt > (u32)kMedList) return block_median(v, n, m, hist);       // block-uniform
    // the second middle value of an even-sized set lies in the same bucket unless the first is the bucket's last
    // element (block-uniform): only then is the smallest key beyond the bucket needed
    const bool need_above = two && !(k1 + 1 - before < cnt);
    u32 above = 0xffffffffu;
    for (int i = tid; i < n; i += kBlockM) {
        const u32 key = f2key(v[i]), b = (key - kmin) >> shift;
        if (b == bin) list[atomicAdd(&m->sel_cle, 1u)] = key;
        else if (need_above && b > bin && key < above) above = key;
    }
    if (need_above) above = block_min(above, m);                       // (barriers inside: the list is complete)
    else __syncthreads();
    if (dbg && tid == 0) dbg[23] = (long long)clock64();
    if ((u32)tid < cnt) {
        const u32 mine = list[tid];
        u32 rank = 0;
        for (u32 j = 0; j < cnt; ++j) { const u32 o = list[j]; rank += (o < mine || (o == mine && j < (u32)tid)) ? 1u : 0u; }
        if (rank == k1 - before) m->sel_key = mine;
        if (rank == k1 + 1 - before) m->best_key = (int)mine;
    }
    __syncthreads();
    if (dbg && tid == 0) dbg[24] = (long long)clock64();
    const u32 key1 = m->sel_key;
    if (!two) return key2f(key1);
    const u32 key2 = need_above ? above : (u32)m->best_key;
    return (key2f(key1) + key2f(key2)) / 2.0f;
}

// np.median, fast path: one log-spaced histogram over [min, max] of the keys (1024 buckets: the float bit
// patterns are spread evenly, no hot bins), the bucket holding the middle rank is compacted into a list and
// ranked by brute force.  Two passes over the data instead of the radix select's five; falls back to the
// radix select when the bucket holds more than kMedList elements (massive ties).
// hist: 1024 counters, list: kMedList keys (LDS scratch); tmin / tmax: this thread's min / max key of v.
__device__ __forceinline__ float block_median_fast(const float *v, int n, MiscM *m, u32 *hist, u32 *list, u32 tmin, u32 tmax)
{
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    u32 *red_max = reinterpret_cast<u32 *>(m->red_f);
    tmin = wave_umin_dpp(tmin);
    tmax = ~wave_umin_dpp(~tmax);
    __syncthreads();
    if (lane == 0) { m->red_i[w] = (int)tmin; red_max[w] = tmax; }
    for (int i = tid; i < 1024; i += kBlockM) hist[i] = 0;
    if (tid == 0) m->sel_cle = 0;
    __syncthreads();
    u32 kmin = (u32)m->red_i[0], kmax = red_max[0];
    for (int q = 1; q < kWavesM; ++q) { const u32 a = (u32)m->red_i[q], b = red_max[q]; kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax; }
    return block_median_ranged(v, n, m, hist, list, kmin, kmax);
}

// two block sums with one pair of barriers (scratch: the rotation table of the template phase, dead by now)
__device__ __forceinline__ void block_sum2(double &a, double &b, MiscM *m) {
    a = wave_sum_dpp_d(a); b = wave_sum_dpp_d(b);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { m->rot[threadIdx.x >> 6][0] = a; m->rot[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    double ta = 0.0, tb = 0.0;
    for (int w = 0; w < kWavesM; ++w) { ta += m->rot[w][0]; tb += m->rot[w][1]; }
    a = ta; b = tb;
}

// np.std of a float32 LDS array from its double sums: sqrt(E[x^2] - E[x]^2) evaluated in double
// (NumPy works in float32; the difference is ~1e-7 relative, inside the 1e-5 bar on h).
__device__ __forceinline__ float std_from_sums(double sx, double sxx, int n) {
    const double mean = sx / (double)n;
    double var = sxx / (double)n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    return sqrtf((float)var);
}


// The spec's normalisation in IEEE double -> float32 (shared by candidates and the winner's matrix): ncc_norm.h, which the
// host check (tests/cpp/ncc_norm_check.cpp) compiles as well.
__device__ __forceinline__ float exact_from_sums(int p, int swp, u32 siiv, double nd, double sT, double rTd, bool cT)
{
    return ncc_norm::spec_from_sums(p, swp, siiv, nd, sT, rTd, cT);
}

// The same value by a shorter route (the winner's matrix evaluates thousands of these per point).  1 / sqrt(dI) comes
// from v_rsq_f64 and two coupled Newton steps - no IEEE square root, no IEEE division - so the product q' differs from
// the spec's q (whose own 1 / sqrt carries two roundings) by less than 2^-49 |q|.  (float)q' = (float)q unless q' lies
// that close to a rounding boundary of float32 (the middle of the 29 discarded mantissa bits) or to one of the clamp
// thresholds 1 and 1.125: those lanes - about 1e-7 of them, plus the perfect matches - take the spec's route; lanes beyond
// a threshold take the clamp.  The arithmetic is ncc_norm.h's; this is its seed.
struct RsqSeed { __device__ __forceinline__ double operator()(double x) const { return __builtin_amdgcn_rsq(x); } };

// one value start to end; spec_route: whether the specification's route decided it (the selftest counts those)
__device__ __forceinline__ float exact_from_sums_fast(int p, int swp, u32 siiv, double nd, double sT, double rTd, bool cT, bool &spec_route)
{
    return ncc_norm::from_sums_fast(p, swp, siiv, nd, sT, rTd, cT, RsqSeed(), spec_route);
}

// Branch-free part of it (ncc_norm::lean): the value by the short route and whether the lane needs a second look
// (ncc_flagged).  Callers evaluate a batch of these back to back (independent dependency chains interleave) and handle the
// rare flagged ones afterwards - a branch around every single value serialises the ~20-deep double-precision chains.  The
// caller hoists `c` (ncc_norm::Hoisted) and handles a constant template on its own.
__device__ __forceinline__ float ncc_fast_nobranch(int p, int swp, u32 siiv, const ncc_norm::Hoisted &c, bool &flagged)
{
    double q;
    return ncc_norm::lean(p, swp, siiv, c, RsqSeed(), flagged, q);
}
// A flagged value, behind the batch: q' is computed again from sums the compiler cannot relate to the batch's (it would
// otherwise keep every q' and 1 / sqrt(dI) of the batch in registers for a block that almost never runs: 51 spilled VGPRs
// instead of 24 in the 128-register build)
__device__ __forceinline__ float ncc_flagged(int p, int swp, u32 siiv, const ncc_norm::Hoisted &c, double rTd)
{
    asm volatile("" : "+v"(p), "+v"(swp));
    bool fl, spec_route; double q;
    (void)ncc_norm::lean(p, swp, siiv, c, RsqSeed(), fl, q);
    return ncc_norm::flagged_value(p, swp, siiv, c, rTd, q, spec_route);
}

struct Score { float lmax, bestv; int bestkey; };

__device__ __forceinline__ void take_better(Score &sc, float rv, int key)
{
    if (rv > sc.bestv || (rv == sc.bestv && key < sc.bestkey)) { sc.bestv = rv; sc.bestkey = key; }
}

}  // namespace

}  // namespace sid
