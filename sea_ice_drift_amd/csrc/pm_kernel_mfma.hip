// pm_kernel_mfma.hip - the pattern-matching kernel on the gfx950 matrix cores.
//
// Operator: reference pmlib.py:117-212, :36-59; NCC specification in DESIGN.md section 3.  The 34x34 uint8
// correlation runs on v_mfma_i32_16x16x64_i8 as an implicit correlation - no im2col is materialised:
//
//   bytes are re-centred (w' = w ^ 0x80, t' = t ^ 0x80 as int8); numer, dI and dT are covariances
//   and do not change under the shift, so the integer sums stay exact and the spec is untouched.
//
//   sweep ("angle-major"):  D[slot][x] += A[slot][c] * B[c][x]
//       M = 16 template slots: up to 15 trial angles + one all-ones template (gives sum w' = S_I')
//       N = 16 adjacent placements x0..x0+15 of one output row y
//       K = 64 window columns c of window row rho = y + i ; A[slot][c] = T'_slot[i][c] (0 for c >= s)
//     B[c][x] = W'[rho][x0 + x + c] is the same for every (y, i) with y + i = rho, so a wavefront
//     keeps a band of BAND output rows in accumulators and a ring of BAND template-row fragments in
//     registers: one window fragment built from LDS (5 ds_read_b32 + 4 v_alignbyte_b32) feeds BAND
//     MFMAs.  BAND = 4 with three wavefronts per SIMD (168 VGPRs), BAND = 8 in the instantiation for the
//     LDS class that fits two workgroups per CU (256 VGPRs): the sweep is LDS-bandwidth-bound, and the
//     taller band halves the LDS bytes per MFMA.
//
//   winner ("row-major"):   the NCC matrix of the best angle is recomputed with M = 16 output rows
//     (A[m][c] = T'_best[rho - y0 - m][c]) and a second all-ones operand for S_I'.
//
//   S_II' = sum w'^2 comes from two running-sum passes over LDS (columns, then rows).
//   The double-precision normalisation of the spec is evaluated only for arg-max candidates picked
//   by a float32 pre-filter (|r~ - r| <= 4e-7 << margin 1e-5) and for the winner's matrix.
//
//   templates: for an integral template centre (what the reference's driver always passes) the rotated
//   nearest-neighbour sample positions depend only on the angle; the host precomputes them once per
//   set_points as LDS patch offsets (pm_capi.hip make_samp) and the kernel gathers through that table;
//   any other centre, and templates at the image border, are sampled on the fly.
//
// One workgroup per grid point; 256 or 768 threads by LDS-footprint class (see kMaxBlockM).  The phases
// other than the sweep are separate non-inlined functions sharing a geometry block in LDS, so each has its
// own register allocation; throughput is set by the latency of a workgroup's phase chain.
// Compile with -ffp-contract=off.
//
// The device code lives in headers by content: pm_kernel_base.h (LDS header, reductions, medians, normalisation),
// pm_kernel_phases.h (the phases both kernels share), pm_kernel_classic.h (the kernel described above) and pm_kernel_rp.inc
// (the row-pair kernel for sides 34 and 35).  This translation unit instantiates both kernels for three wavefronts per SIMD
// (168 VGPRs); pm_kernel_rp_occ4.hip instantiates the row-pair kernel once more for four (128 VGPRs).  Here as well: three
// diagnostic kernels and the host launchers.
#define SID_PM_OCC 3
#include <mutex>
#include <set>
#include <utility>
#include "pm_kernel_classic.h"
#include "pm_kernel_rp.inc"

namespace sid {

namespace {

// exact_from_sums_fast against exact_from_sums on pseudo-random sums of plausible windows (diagnostic):
// out[0] = evaluations, out[1] = results that differ, out[2] = evaluations that took the spec's route
__global__ void ncc_selftest_kernel(unsigned long long seed, int per_thread, int s, unsigned long long *out)
{
    unsigned long long st = seed ^ (0x9e3779b97f4a7c15ull * (unsigned long long)(blockIdx.x * blockDim.x + threadIdx.x + 1));
    auto next = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    const double nd = (double)(s * s);
    unsigned long long bad = 0, slow = 0;
    for (int it = 0; it < per_thread; ++it) {
        // template: sum sT (re-centred), denominator dT = N S_TT - S_T^2 > 0
        const int sT = (int)(next() % (unsigned)(2 * 128 * s * s + 1)) - 128 * s * s;
        const double dTmin = 1.0, dT = dTmin + (double)(next() % (1ull << (20 + (int)(next() % 28))));
        const double rTd = 1.0 / sqrt(dT);
        const int swp = (int)(next() % (unsigned)(2 * 128 * s * s + 1)) - 128 * s * s;
        const unsigned long long sw2 = (unsigned long long)((long long)swp * swp);
        const u32 sii_min = (u32)((sw2 + (unsigned long long)(s * s) - 1) / (unsigned long long)(s * s));
        const u32 room = (u32)(s * s) * 16384u - sii_min;                 // S_I'I' <= N 128^2
        const u32 siiv = sii_min + (u32)(next() % (unsigned long long)(room + 1u)) % (1u << (1 + (int)(next() % 27)));
        const double dI = nd * (double)siiv - (double)swp * (double)swp;
        // numerator within (and sometimes just beyond) the Cauchy-Schwarz bound: nd p - swp sT = f sqrt(dI dT)
        const double f = ((double)(long long)(next() % 2400001ull) - 1200000.0) / 1000000.0;
        const double target = f * sqrt(dI > 0 ? dI : 0.0) * sqrt(dT);
        const int p = (int)llrint((target + (double)swp * (double)sT) / nd);
        const float a = exact_from_sums(p, swp, siiv, nd, (double)sT, rTd, false);
        bool spec_route;
        const float b = exact_from_sums_fast(p, swp, siiv, nd, (double)sT, rTd, false, spec_route);
        bad += __float_as_uint(a) != __float_as_uint(b) ? 1ull : 0ull;
        slow += spec_route ? 1ull : 0ull;
    }
    atomicAdd(&out[0], (unsigned long long)per_thread);
    if (bad) atomicAdd(&out[1], bad);
    if (slow) atomicAdd(&out[2], slow);
}

// hypot_fast against hypot_spec on pseudo-random float32 pairs of the magnitudes second differences of NCC values take
// (and, every fourth sample, pairs constructed to land next to a float32 rounding boundary): out = evaluations, mismatches
__global__ void hypot_selftest_kernel(unsigned long long seed, int per_thread, unsigned long long *out)
{
    unsigned long long st = seed ^ (0x9e3779b97f4a7c15ull * (unsigned long long)(blockIdx.x * blockDim.x + threadIdx.x + 1));
    auto next = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    unsigned long long bad = 0;
    for (int it = 0; it < per_thread; ++it) {
        const unsigned long long a = next(), b = next();
        // mantissas uniform, exponents 2^-40 .. 2^1 (and occasionally zero / denormal / huge)
        const int ea = 127 - (int)(a % 41) + 1, eb = 127 - (int)((a >> 8) % 41) + 1;
        float x = __uint_as_float(((u32)ea << 23) | (u32)(b & 0x7fffffu)), y = __uint_as_float(((u32)eb << 23) | (u32)((b >> 23) & 0x7fffffu));
        const u32 kind = (u32)(a >> 60);
        if (kind == 0) y = 0.0f;                                       // perfect squares: sqrt lands on a float exactly
        if (kind == 1) { x = 0.0f; y = 0.0f; }
        if (kind == 2) x = __uint_as_float((u32)(b & 0x7fffffu));      // denormal
        if (kind == 3) { x = __uint_as_float(0x7e000000u | (u32)(b & 0x7fffffu)); }
        if (a & (1ull << 40)) x = -x;
        if (a & (1ull << 41)) y = -y;
        bad += __float_as_uint(hypot_fast(x, y)) != __float_as_uint(hypot_spec(x, y)) ? 1ull : 0ull;
    }
    atomicAdd(&out[0], (unsigned long long)per_thread);
    if (bad) atomicAdd(&out[1], bad);
}

__global__ void rsqrt_kernel(const double *x, double *y, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = 1.0 / sqrt(x[i]);
}

}  // namespace

PmKernel rp_occ4_kernel(int img_size, int paired, int pitch);   // pm_kernel_rp_occ4.hip

int launch_rsqrt(const double *x, double *y, int64_t n, void *stream)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (n <= 0) return (int)hipSuccess;
    hipLaunchKernelGGL(rsqrt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, n);
    return (int)hipGetLastError();
}

int launch_ncc_selftest(unsigned long long seed, int blocks, int per_thread, int s, unsigned long long *out, void *stream)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ncc_selftest_kernel, dim3((unsigned)blocks), dim3(256), 0, st, seed, per_thread, s, out);
    return (int)hipGetLastError();
}

int launch_hypot_selftest(unsigned long long seed, int blocks, int per_thread, unsigned long long *out, void *stream)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(hypot_selftest_kernel, dim3((unsigned)blocks), dim3(256), 0, st, seed, per_thread, out);
    return (int)hipGetLastError();
}

// The dynamic-LDS limit belongs to the function and the device, not to the stream: it is raised to the maximum once per
// (kernel, device) - always the maximum, so that launches of different footprints from different host threads cannot
// undercut each other - instead of on every launch.
static hipError_t allow_max_lds(PmKernel kern)
{
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const std::pair<const void *, int> key(reinterpret_cast<const void *>(kern), dev);
    std::lock_guard<std::mutex> lock(mu);
    if (done.count(key)) return hipSuccess;
    e = hipFuncSetAttribute(key.first, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds_bytes());
    if (e == hipSuccess) done.insert(key);
    return e;
}

int launch_pm_mfma(const PMArgs &args, int lds_bytes, int nthreads, int band, bool paired, void *stream)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (args.n_launch <= 0) return (int)hipSuccess;
    if (paired) {                                                      // at most 7 angles: one group, paired slots
        if (band != 4 || args.n_angles > kPairedMaxAngles) return (int)hipErrorInvalidValue;
    } else if (band == 8) {
        if (!mfma_band8_supported(args.img_size) || nthreads != 256) return (int)hipErrorInvalidValue;
    } else if (band != 4) return (int)hipErrorInvalidValue;
    const PmKernel kern = classic_kernel(mfma_side_arg(args.img_size), band, paired);
    if (!kern) return (int)hipErrorInvalidValue;
    const hipError_t e = allow_max_lds(kern);
    if (e != hipSuccess) return (int)e;
    if (lds_bytes > max_lds_bytes() || (nthreads != 256 && nthreads != 768)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3(args.n_launch), dim3(nthreads), lds_bytes, st, args);
    return (int)hipGetLastError();
}

int launch_pm_rp(const PMArgs &args, int lds_bytes, int nthreads, int band, int paired, int pitch, int occ, void *stream, bool big)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (args.n_launch <= 0) return (int)hipSuccess;
    if (!rp_size_supported(args.img_size)) return (int)hipErrorInvalidValue;
    if ((band != 4 && band != 8) || (band == 8 && nthreads != 256)) return (int)hipErrorInvalidValue;
    if ((occ != 3 && occ != 4) || (occ == 4 && (nthreads != 256 || band != 4))) return (int)hipErrorInvalidValue;
    if (paired && (band != 4 || args.n_angles > (paired == 2 ? kQuadMaxAngles : kPairedMaxAngles))) return (int)hipErrorInvalidValue;
    if (big && (band != 4 || paired || pitch || occ != 3)) return (int)hipErrorInvalidValue;
    const PmKernel kern = occ == 4 ? rp_occ4_kernel(args.img_size, paired, pitch) : rp_kernel<3>(args.img_size, band, paired, pitch, big);
    if (!kern) return (int)hipErrorInvalidValue;
    const hipError_t e = allow_max_lds(kern);
    if (e != hipSuccess) return (int)e;
    if (lds_bytes > max_lds_bytes() || nthreads < 192 || nthreads > 768 || (nthreads & 63)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3(args.n_launch), dim3(nthreads), lds_bytes, st, args);
    return (int)hipGetLastError();
}

}  // namespace sid
