// pm_capi.hip - host side of the C ABI declared in include/sid_pm.h.
//
// Replaces the reference's process pool (pmlib.py:430-448): the "shared_args" of the
// workers become device-resident buffers owned by a handle, the Pool.map over point
// indices becomes a few kernel launches (one per LDS-footprint class), and the pickled
// 5-tuples coming back become one device array copied to the host.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "../../include/sid_pm.h"
#include "pm_kernel.h"
#include "pm_large.h"
#include "pm_plan.h"
#include "pm_host.h"

using namespace sid::plan;   // the launch planner: Switches, Plan, Bucket and the decision functions

static_assert(SID_PM_SUBPIXEL == sid::kSubpixel, "the kernels test the bit of include/sid_pm.h");

#define SID_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? SID_PM_ERR_NOMEM : SID_PM_ERR_HIP,         \
                        "%s failed: %s", #expr, hipGetErrorString(e_));                        \
    } while (0)

struct Image {
    const uint8_t *ptr = nullptr;       // device
    int64_t rows = 0, cols = 0, stride = 0;
};

// device memory that frees itself where it leaves its scope (pm_host.h), on the device that is current there: the entry points
// declare their buffers after their Guard
struct HipAlloc {
    static int alloc(void **p, size_t bytes) { HIP_TRY(hipMalloc(p, bytes)); return SID_PM_OK; }
    static void free(void *p) { (void)hipFree(p); }
};
template <typename T> using DevBuf = ScopedBuf<T, HipAlloc>;

}  // namespace

struct sid_pm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // image pairs: two owned slots + one borrowed binding
    DevBuf<uint8_t> own[2][2];
    Image slot_img[2][2];
    Image cur[2];
    bool have_pair = false;
    int cur_slot = -1;                  // -1: borrowed binding (or none)
    // pair streaming: uploads run on their own stream; slot_ready[s] = upload of slot s complete,
    // slot_done[s] = last kernels reading slot s complete (an upload into s waits for it)
    hipStream_t copy_stream = nullptr;
    // short runs (a rank's shard of an N-GPU run: two or three launches of a few rounds of workgroups each) put their launches
    // side by side on these streams, so that one launch's half-empty last round is filled by the next (pm_plan.h launch_schedule)
    hipStream_t side[3] = {nullptr, nullptr, nullptr};
    hipEvent_t fork_ev = nullptr, join_ev[3] = {nullptr, nullptr, nullptr};
    // long runs CHAIN their launches on side[0] / side[1] (pm_plan.h launch_schedule): launch k + 1 waits - a stream wait on signal
    // memory - for the word launch k's last-arriving workgroup stores the run's epoch into.  Allocated at the first run that
    // wants them: the arrival counters of every launch index (zero between runs: the kernels restore them) and one release
    // word per launch index (an allocation of signal memory is one 64-bit word)
    bool can_wait_value = false;        // hipDeviceAttributeCanUseStreamWaitValue
    bool chain_alloc_failed = false;    // the signal memory was refused once: not asked for again
    uint32_t *chain_count = nullptr;    // [kChainMaxLaunches][kChainWords]
    unsigned long long *chain_release[sid::kChainMaxLaunches] = {};
    int n_chain_release = 0;
    unsigned long long chain_epoch = 1; // chained runs of this handle so far, + 1 (a fresh release word never holds a value a run waits for)
    hipEvent_t slot_ready[2] = {nullptr, nullptr}, slot_done[2] = {nullptr, nullptr};
    bool ready_rec[2] = {false, false}, done_rec[2] = {false, false};
    // resident points: one device arena (a single upload per set_points) carved into the vectors below
    DevBuf<uint8_t> arena;
    double *d_vec = nullptr;            // 5 * n
    int32_t *d_order = nullptr;
    double *d_angles = nullptr, *d_rot = nullptr;
    uint16_t *d_samp = nullptr;         // sampling table of the kernel (make_samp)
    uint32_t *d_samp2 = nullptr;        // ... sorted per angle for the row-pair kernel (make_samp2; SID_PM_SAMP2=1: built)
    bool rp = false;                    // the resident points run the row-pair kernel (decided at set_points: use_rp) ...
    int rp_paired = 0;                  // ... with slot groups: 0 none, 1 two groups (<= 7 angles), 2 four groups (<= 3 angles)
    bool have_samp = false;             // SID_PM_NO_SAMP_TABLE=1 keeps the on-the-fly sampling (tests of the general sampler)
    int samp_nflag = 0;
    // host copies of what the classification needs: the launch classes depend on the shape of image 2, so a
    // pair of another shape (select_pair / bind_pair / upload_pair after set_points) is re-classified at run()
    std::vector<double> h_c2fg, h_r2fg, h_border, h_c1, h_r1;
    int64_t cls_rows2 = -1, cls_cols2 = -1;
    DevBuf<double> out;
    DevBuf<int32_t> out_ij;
    DevBuf<int32_t> dbg_err;            // debugging builds only (SID_PM_DEBUG_CHECK=1)
    DevBuf<uint32_t> gsii;              // row-pair kernel: sum w'^2 per placement of every resident point (PMArgs::gsii) ...
    DevBuf<uint32_t> d_goff;            // ... and the offset of every launch position's block in it (units of 64 entries)
    DevBuf<sid::PointRec> d_rec;        // row-pair kernel: one record per launch position (index, block offset, the five inputs)
    DevBuf<uint32_t> ring, pool;        // recycled blocks of the launches that keep accumulators (PMArgs::ring / pool; SID_PM_NO_RECYCLE=1: none)
    int32_t *h_refused = nullptr;       // pinned, device-visible: valid points a launch could not hold (PMArgs::refused)
    double *user_out = nullptr;         // caller-owned result arrays (bind_results)
    int32_t *user_ij = nullptr;
    // the launches of the resident points for the current pair, the points of the large-window pipeline and the switches they
    // were decided with (pm_plan.h; made by classify_points).  sid_pm_run launches from this and reads no switch of a plan again
    Plan plan;
    DevBuf<int32_t> d_nan_idx;          // Plan::nan_idx on the device
    sid::LwWorkspace lw;
    // rot_order 2..5: image 1 through scipy's spline prefilter (coef[1]; coef[0] = scratch), valid for (pair_serial, order); and the
    // templates of the resident points sampled from it (pre), valid for (pair_serial, points_serial)
    DevBuf<double> coef[2];
    uint64_t pair_serial = 1, points_serial = 1, coef_pair = 0, pre_pair = 0, pre_points = 0;
    int coef_order = 0;
    DevBuf<uint8_t> pre;
    DevBuf<double> lw_small;            // rotate_and_match as a call of its own: angles, rotation terms, the five results
    int64_t n = 0;
    int img_size = 0, n_angles = 0;
    uint32_t flags = 0;
    bool have_points = false;
};

namespace {

struct Guard {
    int prev = -1;
    explicit Guard(int dev) { (void)hipGetDevice(&prev); if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~Guard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// rotation terms [K][4] = cos, sin, tcT0, tcT1 of angle - alpha0 (pmlib.py:105-110), as the CALLER's NumPy computed them:
// required (include/sid_pm.h) - libm's cos / sin may differ from NumPy's in the last bit, which can tip a sample at a rounding tie
int make_rot(int n_angles, const double *rot_in, std::vector<double> &rot)
{
    if (!rot_in) return fail(SID_PM_ERR_ARG, "rot is required: [n_angles][4] = cos, sin, tcT0, tcT1 as the caller's NumPy computed them (pmlib.py:105-110; include/sid_pm.h)");
    rot.assign(rot_in, rot_in + 4 * (size_t)n_angles);
    for (const double v : rot) if (!(fabs(v) < 1e6)) return fail(SID_PM_ERR_ARG, "rot holds a non-finite or absurd value");
    return SID_PM_OK;
}

// Sampling table of the MFMA kernel.  The reference rounds the template centres to integers before the
// dispatch (pmlib.py:401), and for an integral centre (R, C) the nearest-neighbour sample positions of
// get_template (pmlib.py:105-113; scipy order 0: floor(x + 0.5)) are those of the centre (0, 0) shifted by
// (R, C) - unless a coordinate lies so close to k + 1/2 that the float64 roundings at the magnitude of R
// could tip it.  Those entries (|frac - boundary| < kSampGuard; expected: none or a handful per table) carry
// a flag and are recomputed per point in the kernel (ph_tpl_fix) with the reference's operation order.
// Entry = (row + pradius) * ppitch + (col + pradius): the byte offset inside the kernel's LDS patch.
int make_samp(const std::vector<double> &rot, int K, int s, std::vector<uint16_t> &tab)
{
    int nflag = 0;
    const sid::MfmaLdsLayout L = sid::mfma_lds_layout(s + 1, s + 1, s);
    const int sp = sid::samp_pitch(s);
    tab.assign((size_t)K * s * sp, 0);
    for (int k = 0; k < K; ++k) {
        const double cosa = rot[4 * k + 0], sina = rot[4 * k + 1];
        const double off0 = 0.0 - rot[4 * k + 2], off1 = 0.0 - rot[4 * k + 3];
        for (int i = 0; i < s; ++i)
            for (int j = 0; j < s; ++j) {
                double rr = 0.0 + (double)i * cosa;                    // NI_GeometricTransform order (matrix = transform.T)
                rr = rr + (double)j * sina;
                rr = rr + off0;
                double cc = 0.0 + (double)i * (-sina);
                cc = cc + (double)j * cosa;
                cc = cc + off1;
                const double fr = floor(rr + 0.5), fc = floor(cc + 0.5);
                const double dr = (rr + 0.5) - fr, dc = (cc + 0.5) - fc;
                bool doubt = !(dr >= sid::kSampGuard && dr <= 1.0 - sid::kSampGuard && dc >= sid::kSampGuard && dc <= 1.0 - sid::kSampGuard);
                int pr = (int)fr + L.pradius, pc = (int)fc + L.pradius;
                if (!(pr >= 0 && pr < L.pdim && pc >= 0 && pc < L.pdim)) doubt = true;
                // flagged: gather the spare byte behind the patch (128), the kernel's fix pass supplies the sample
                tab[((size_t)k * s + i) * sp + j] = doubt ? (uint16_t)((L.pdim * L.ppitch) | 0x8000) : (uint16_t)(pr * L.ppitch + pc);
                nflag += doubt ? 1 : 0;
            }
    }
    return nflag;
}

// The sampling table sorted per angle for the row-pair kernel (PMArgs::samp2): run records first, gather records after.
// A quad (row i, columns 4 jq .. 4 jq + 3, all inside the 32 main columns) is a RUN when none of its entries is flagged and
// its four patch offsets are consecutive.
void make_samp2(const std::vector<uint16_t> &tab, int K, int s, std::vector<uint32_t> &out)
{
    const int sp = sid::samp_pitch(s), nq = sp >> 2;
    out.assign((size_t)K * sid::kSamp2Words, 0u);
    for (int k = 0; k < K; ++k) {
        uint32_t *blk = out.data() + (size_t)k * sid::kSamp2Words;
        uint32_t nrun = 0, ngat = 0;
        uint16_t *ids = reinterpret_cast<uint16_t *>(blk + sid::kSamp2Id);
        for (int i = 0; i < s; ++i)
            for (int jq = 0; jq < nq; ++jq) {
                const uint16_t *e = tab.data() + ((size_t)k * s + i) * sp + 4 * jq;
                const bool full = 4 * jq + 3 < s && jq < 8;
                const bool run = full && !((e[0] | e[1] | e[2] | e[3]) & 0x8000u) && e[1] == e[0] + 1 && e[2] == e[0] + 2 && e[3] == e[0] + 3;
                if (run) blk[sid::kSamp2Run + nrun++] = (uint32_t)(e[0] & ~3u) | ((uint32_t)(e[0] & 3u) << 15) | ((uint32_t)i << 17) | ((uint32_t)jq << 23);
                else {
                    blk[sid::kSamp2Gat + 2 * ngat] = (uint32_t)e[0] | ((uint32_t)e[1] << 16);
                    blk[sid::kSamp2Gat + 2 * ngat + 1] = (uint32_t)e[2] | ((uint32_t)e[3] << 16);
                    ids[ngat++] = (uint16_t)(i * nq + jq);
                }
            }
        blk[0] = nrun; blk[1] = ngat;
    }
}

int check_images(const Image &a, const Image &b)
{
    if (!a.ptr || !b.ptr) return fail(SID_PM_ERR_ARG, "null image pointer");
    if (a.rows < 1 || a.cols < 1 || a.stride < a.cols || b.rows < 1 || b.cols < 1 || b.stride < b.cols)
        return fail(SID_PM_ERR_ARG, "bad image shape/stride");
    return SID_PM_OK;
}

int check_sweep(int img_size, const double *angles, int n_angles, uint32_t flags)
{
    if (!angles || n_angles < 1)
        return fail(SID_PM_ERR_ARG, "angles must hold at least one angle (the reference's loop, pmlib.py:150, "
                                    "leaves best_result undefined for an empty list)");
    if (n_angles > sid::kMaxAngles) return fail(SID_PM_ERR_UNSUPPORTED, "more than %d angles", sid::kMaxAngles);
    if (img_size < 2 || img_size > sid::kLargeMaxSide)
        return fail(SID_PM_ERR_UNSUPPORTED, "img_size=%d: the kernels support 2..%d", img_size, sid::kLargeMaxSide);
    if (flags & ~(SID_PM_HES_NORM | SID_PM_HES_SMTH | SID_PM_MCC_NORM | SID_PM_ROT_ORDER(7) | SID_PM_SUBPIXEL)) return fail(SID_PM_ERR_ARG, "unknown flag bits");
    if (((flags >> 3) & 7u) > 5u) return fail(SID_PM_ERR_UNSUPPORTED, "rot_order %u: scipy's spline orders are 0..5", (flags >> 3) & 7u);
    return SID_PM_OK;
}

// scipy.ndimage.gaussian_filter(ccm, 1) taps (pmlib.py:46-47): exp(-k^2 / 2), k = -4..4, divided by their sum in
// NumPy's pairwise order for nine terms; host libm, as in the oracle
void gauss_taps(double w5[5])
{
    double w[9];
    for (int k = -4; k <= 4; ++k) w[k + 4] = exp(-0.5 * (double)(k * k));
    const double sum = (((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]))) + w[8];
    for (int k = 0; k < 5; ++k) w5[k] = w[k] / sum;
}

// the current pair as the kernels take it (the resident points' launches and debug_point)
void set_images(const sid_pm_ctx *ctx, sid::PMArgs &A)
{
    A.img1 = ctx->cur[0].ptr; A.rows1 = ctx->cur[0].rows; A.cols1 = ctx->cur[0].cols; A.stride1 = ctx->cur[0].stride;
    A.img2 = ctx->cur[1].ptr; A.rows2 = ctx->cur[1].rows; A.cols2 = ctx->cur[1].cols; A.stride2 = ctx->cur[1].stride;
}

int fill_args(sid_pm_ctx *ctx, const Switches &run_sw, sid::PMArgs &A)
{
    memset(&A, 0, sizeof A);
    gauss_taps(A.gauss_w);
    set_images(ctx, A);
    const int64_t n = ctx->n;
    A.c1 = ctx->d_vec; A.r1 = ctx->d_vec + n; A.c2fg = ctx->d_vec + 2 * n; A.r2fg = ctx->d_vec + 3 * n;
    A.border = ctx->d_vec + 4 * n;
    A.img_size = ctx->img_size; A.n_angles = ctx->n_angles; A.flags = ctx->flags;
    A.angles = ctx->d_angles; A.rot = ctx->d_rot; A.samp = ctx->have_samp ? ctx->d_samp : nullptr; A.samp_nflag = ctx->samp_nflag; A.samp2 = ctx->have_samp ? ctx->d_samp2 : nullptr;
    A.out = ctx->user_out ? ctx->user_out : ctx->out.p;
    A.out_ij = ctx->user_out ? ctx->user_ij : ctx->out_ij.p;
    A.refused = ctx->h_refused;
    A.gsii = ctx->gsii.p; A.gsii_off = ctx->d_goff.p; A.rec = ctx->d_rec.p;
    A.gs_keep_si = (ctx->rp && ctx->plan.gs_keep_si) ? 1u : 0u;
    A.gs_keep_acc = 0u; A.ring = nullptr; A.pool = ctx->pool.p; A.pool_stride = ctx->plan.pool_stride;   // (per launch: sid_pm_run)
    if (run_sw.debug_check) {
        if (!ctx->dbg_err.p && ctx->dbg_err.reserve(320) == SID_PM_OK) (void)hipMemset(ctx->dbg_err.p, 0, 320 * sizeof(int32_t));
        A.dbg_err = ctx->dbg_err.p;
    }
    return SID_PM_OK;
}

// The handle's memory for chained launches (sid_pm_ctx::chain_count / chain_release), for runs of up to n launches.  False -
// and never asked for again - when the runtime refuses it: the run then keeps its launches in sequence.
bool ensure_chain_memory(sid_pm_ctx *ctx, size_t n)
{
    if (ctx->chain_alloc_failed || n > (size_t)sid::kChainMaxLaunches) return false;
    if (!ctx->chain_count) {
        const size_t bytes = sizeof(uint32_t) * (size_t)sid::kChainMaxLaunches * sid::kChainWords;
        if (hipMalloc(reinterpret_cast<void **>(&ctx->chain_count), bytes) != hipSuccess) { ctx->chain_count = nullptr; ctx->chain_alloc_failed = true; }
        else if (hipMemset(ctx->chain_count, 0, bytes) != hipSuccess) { (void)hipFree(ctx->chain_count); ctx->chain_count = nullptr; ctx->chain_alloc_failed = true; }
    }
    while (!ctx->chain_alloc_failed && (size_t)ctx->n_chain_release < n) {
        void *p = nullptr;
        if (hipExtMallocWithFlags(&p, sizeof(unsigned long long), hipMallocSignalMemory) != hipSuccess || !p) { ctx->chain_alloc_failed = true; break; }
        // (host-visible; whatever the runtime initialised the word with, it starts below every epoch: chain_epoch starts at 1
        // and a run increments it first)
        __atomic_store_n(static_cast<unsigned long long *>(p), 0ull, __ATOMIC_RELEASE);
        ctx->chain_release[ctx->n_chain_release++] = static_cast<unsigned long long *>(p);
    }
    if (ctx->chain_alloc_failed) (void)hipGetLastError();           // (the refusal is handled here: not the next call's error)
    return !ctx->chain_alloc_failed;
}

// The plan of the resident points for the pair that is current now (pm_plan.h: plan_points, with the switches as the
// environment holds them at this call) and its device side: buffers, free lists, the uploads of `order`, `goff` and the
// point records.  The plan depends on the shape of image 2, so this runs in set_points and again in run() whenever the
// current pair's image 2 has another shape.  The handle takes the plan only when all of it succeeded.
int classify_points(sid_pm_ctx *ctx)
{
    const Switches sw = read_switches();
    PlanInput in;
    in.n = ctx->n;
    in.c1 = ctx->h_c1.data(); in.r1 = ctx->h_r1.data(); in.c2fg = ctx->h_c2fg.data(); in.r2fg = ctx->h_r2fg.data(); in.border = ctx->h_border.data();
    in.s = ctx->img_size; in.K = ctx->n_angles; in.flags = ctx->flags;
    in.rows1 = ctx->cur[0].rows; in.cols1 = ctx->cur[0].cols; in.rows2 = ctx->cur[1].rows; in.cols2 = ctx->cur[1].cols;
    in.rp = ctx->rp; in.rpp = ctx->rp_paired;
    Plan plan;
    std::string err;
    if (int rc = plan_points(in, sw, plan, err)) return fail(rc, "%s", err.c_str());
    const size_t n_order = plan.order.size();
    if (int rc = ctx->d_nan_idx.reserve(std::max<size_t>(plan.nan_idx.size(), 1))) return rc;
    if (!plan.nan_idx.empty()) HIP_TRY(hipMemcpy(ctx->d_nan_idx.p, plan.nan_idx.data(), sizeof(int32_t) * plan.nan_idx.size(), hipMemcpyHostToDevice));
    if (ctx->rp) {
        if (plan.pool_stride) {
            if (int rc = ctx->pool.reserve((size_t)sid::kPoolBlocks * plan.pool_stride)) return rc;
            if (int rc = ctx->ring.reserve((size_t)sid::kRingU64 * 2)) return rc;
            // every block free (all bits set).  Rewritten at every classification - no launch of this handle is in flight here -
            // so that an aborted run cannot leave a list short of blocks
            std::vector<uint32_t> init((size_t)sid::kRingU64 * 2, 0u);
            for (int w = 0; w < 8 * sid::kRingWordsPerXcd; ++w) { init[(size_t)w * sid::kRingStride * 2] = 0xffffffffu; init[(size_t)w * sid::kRingStride * 2 + 1] = 0xffffffffu; }
            HIP_TRY(hipMemcpyAsync(ctx->ring.p, init.data(), init.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
        {   // fail with the numbers before hipMalloc does
            size_t free_b = 0, total_b = 0;
            if (plan.gsii_granules * 256ull > ctx->gsii.cap * sizeof(uint32_t) && hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
                plan.gsii_granules * 256ull > (uint64_t)free_b + ctx->gsii.cap * sizeof(uint32_t))
                return fail(SID_PM_ERR_NOMEM, "per-placement tables of %lld points need %.1f GB of device memory, %.1f GB are free (smaller batches, or borders below 69 px)",
                            (long long)ctx->n, (double)plan.gsii_granules * 256e-9, (double)free_b * 1e-9);
        }
        if (int rc = ctx->gsii.reserve((size_t)std::max<uint64_t>(plan.gsii_granules, 1) * 64)) return rc;
        if (int rc = ctx->d_goff.reserve((size_t)std::max<int64_t>(ctx->n, 1))) return rc;
        if (int rc = ctx->d_rec.reserve((size_t)std::max<int64_t>(ctx->n, 1))) return rc;
    }
    if (n_order) {                                                    // (the points of the large-window pipeline are in no launch)
        HIP_TRY(hipMemcpyAsync(ctx->d_order, plan.order.data(), sizeof(int32_t) * n_order, hipMemcpyHostToDevice, ctx->stream));
        if (ctx->rp) HIP_TRY(hipMemcpyAsync(ctx->d_goff.p, plan.goff.data(), sizeof(uint32_t) * n_order, hipMemcpyHostToDevice, ctx->stream));
        if (ctx->rp) HIP_TRY(hipMemcpyAsync(ctx->d_rec.p, plan.recs.data(), sizeof(sid::PointRec) * n_order, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));               // (the host vectors are pageable)
    }
    if (sw.verbose) {                                                 // the launches of a step, one line each
        for (const Bucket &b : plan.buckets)
            fprintf(stderr, "sid_pm: launch of %d points, %d B of LDS (%d per CU), band %d, window pitch %d, %d wavefronts per SIMD\n",
                    b.count, b.lds, std::min(b.occ, blocks_per_cu(b.lds)), b.band, b.pitch, b.occ);
        if (!plan.large_idx.empty())
            fprintf(stderr, "sid_pm: %zu points through the large-window pipeline (one point at a time, tiled over the device)\n", plan.large_idx.size());
    }
    ctx->plan = std::move(plan);
    ctx->plan.recs = std::vector<sid::PointRec>();                    // (on the device now; the largest of the host vectors)
    ctx->cls_rows2 = in.rows2; ctx->cls_cols2 = in.cols2;
    return SID_PM_OK;
}

// rot_order 2..5 (pmlib.py:112-113): image 1 of the current pair through scipy's whole-image spline prefilter, once per pair and
// order (8 B per pixel x 2 buffers, kept with the handle); enqueued on the handle's stream behind the upload of the pair
int ensure_coef(sid_pm_ctx *ctx, int order)
{
    if (order < 2) return SID_PM_OK;
    if (ctx->coef_pair == ctx->pair_serial && ctx->coef_order == order && ctx->coef[1].p) return SID_PM_OK;
    const size_t px = (size_t)ctx->cur[0].rows * (size_t)ctx->cur[0].cols;
    if (ctx->cur[0].rows < 2 && ctx->cur[0].cols < 2) return fail(SID_PM_ERR_UNSUPPORTED, "rot_order %d on a 1 x 1 image", order);
    {
        size_t free_b = 0, total_b = 0;
        const size_t need = (ctx->coef[0].cap < px ? px * 8 : 0) + (ctx->coef[1].cap < px ? px * 8 : 0);
        if (need && hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b)
            return fail(SID_PM_ERR_NOMEM, "rot_order %d: the spline coefficients of image 1 need %.1f GB of device memory, %.1f GB are free", order, (double)need * 1e-9, (double)free_b * 1e-9);
    }
    if (int rc = ctx->coef[0].reserve(px)) return rc;
    if (int rc = ctx->coef[1].reserve(px)) return rc;
    if (ctx->cur_slot >= 0 && ctx->ready_rec[ctx->cur_slot]) HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->slot_ready[ctx->cur_slot], 0));
    const int e = sid::lw_spline_prefilter(ctx->cur[0].ptr, ctx->cur[0].rows, ctx->cur[0].cols, ctx->cur[0].stride, order, ctx->coef[0].p, ctx->coef[1].p, ctx->stream);
    if (e) return fail(SID_PM_ERR_HIP, "spline prefilter: %s", hipGetErrorString((hipError_t)e));
    ctx->coef_pair = ctx->pair_serial; ctx->coef_order = order;
    ctx->pre_pair = 0;                                                // (templates sampled from the old coefficients are stale)
    return SID_PM_OK;
}

// ... and the K templates of every resident point sampled from them (the one-workgroup-per-point kernels load these: PMArgs::pre)
int ensure_presampled(sid_pm_ctx *ctx, int order)
{
    if (order < 2 || ctx->n == 0) return SID_PM_OK;
    if (ctx->pre_pair == ctx->pair_serial && ctx->pre_points == ctx->points_serial && ctx->pre.p) return SID_PM_OK;
    const size_t bytes = (size_t)ctx->n * (size_t)ctx->n_angles * (size_t)ctx->img_size * (size_t)ctx->img_size;
    {
        size_t free_b = 0, total_b = 0;
        if (bytes > ctx->pre.cap && hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes > free_b)
            return fail(SID_PM_ERR_NOMEM, "rot_order %d: the pre-sampled templates of %lld points need %.1f GB of device memory, %.1f GB are free (smaller batches)",
                        order, (long long)ctx->n, (double)bytes * 1e-9, (double)free_b * 1e-9);
    }
    if (int rc = ctx->pre.reserve(bytes)) return rc;
    const int e = sid::lw_presample(ctx->coef[1].p, ctx->cur[0].rows, ctx->cur[0].cols, ctx->d_vec, ctx->d_vec + ctx->n, ctx->n, ctx->d_rot, ctx->n_angles,
                                    ctx->img_size, order, ctx->pre.p, ctx->stream);
    if (e) return fail(SID_PM_ERR_HIP, "template pre-sampling: %s", hipGetErrorString((hipError_t)e));
    ctx->pre_pair = ctx->pair_serial; ctx->pre_points = ctx->points_serial;
    return SID_PM_OK;
}

// The points of the resident set that are beyond the one-point kernels, one after the other through the large-window pipeline
// (pm_large.hip): a stream of launches, nothing read back; results straight into the rows of the run's result arrays.
int run_large_points(sid_pm_ctx *ctx, const sid::PMArgs &A)
{
    if (!ctx->plan.nan_idx.empty()) {
        const int e = sid::lw_write_nan(ctx->d_nan_idx.p, (int)ctx->plan.nan_idx.size(), A.out, A.out_ij, ctx->stream);
        if (e) return fail(SID_PM_ERR_HIP, "large-window pipeline: %s", hipGetErrorString((hipError_t)e));
    }
    std::vector<sid::LargeCall> calls;
    calls.reserve(ctx->plan.large_idx.size());
    size_t worst = 0;
    for (const int32_t i : ctx->plan.large_idx) {
        int wh = 0, ww = 0;
        const double c2 = ctx->h_c2fg[(size_t)i], r2 = ctx->h_r2fg[(size_t)i], b = ctx->h_border[(size_t)i];
        if (!window_dims(c2, r2, b, ctx->img_size, ctx->cur[1].rows, ctx->cur[1].cols, wh, ww)) continue;   // (cannot happen: classified with this pair)
        const int hws = (int)((double)ctx->img_size / 2.0);
        sid::LargeCall c;
        c.img1 = A.img1; c.rows1 = A.rows1; c.cols1 = A.cols1; c.stride1 = A.stride1;
        c.img2 = A.img2; c.stride2 = A.stride2;
        c.win_r0 = (int64_t)(r2 - hws - b); c.win_c0 = (int64_t)(c2 - hws - b); c.wh = wh; c.ww = ww;
        c.c1 = ctx->h_c1[(size_t)i]; c.r1 = ctx->h_r1[(size_t)i];
        c.s = ctx->img_size; c.K = ctx->n_angles; c.flags = ctx->flags;
        c.d_rot = ctx->d_rot; c.d_angles = ctx->d_angles;
        c.d_coef = ((ctx->flags >> 3) & 7u) >= 2u ? ctx->coef[1].p : nullptr;
        c.add_c = c2; c.add_r = r2;
        memcpy(c.gauss_w, A.gauss_w, sizeof c.gauss_w);
        c.out5 = A.out + 5 * (size_t)i; c.ij3 = A.out_ij ? A.out_ij + 3 * (size_t)i : nullptr;
        worst = std::max(worst, sid::lw_scratch_bytes(wh, ww, c.s, c.K, c.flags));
        calls.push_back(c);
    }
    if (!calls.empty()) {
        const int e = sid::lw_run_batch(calls.data(), (int)calls.size(), ctx->lw, ctx->stream);
        if (e == -1) return fail(SID_PM_ERR_NOMEM, "the large-window pipeline could not allocate its device scratch (%.2f GB for the largest of %zu points, batches of up to 3 GB)",
                                 (double)worst * 1e-9, calls.size());
        if (e) return fail(SID_PM_ERR_HIP, "large-window pipeline: %s", hipGetErrorString((hipError_t)e));
    }
    return SID_PM_OK;
}

}  // namespace

// ------------------------------------------------------------------------------- API
SID_EXPORT int sid_pm_abi_version(void) { return SID_PM_ABI_VERSION; }

SID_EXPORT const char *sid_pm_strerror(int code)
{
    switch (code) {
    case SID_PM_OK: return "ok";
    case SID_PM_ERR_ARG: return "bad argument";
    case SID_PM_ERR_HIP: return "HIP runtime error";
    case SID_PM_ERR_NOMEM: return "out of memory";
    case SID_PM_ERR_UNSUPPORTED: return "unsupported option or size";
    case SID_PM_ERR_NODEVICE: return "no gfx950 device";
    case SID_PM_ERR_STATE: return "call order violated";
    default: return "unknown error";
    }
}

SID_EXPORT const char *sid_pm_last_error(void) { return g_err.c_str(); }

SID_EXPORT int sid_pm_device_count(int *count)
{
    if (!count) return fail(SID_PM_ERR_ARG, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(SID_PM_ERR_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_create(int device, sid_pm_ctx **out)
{
    if (!out) return fail(SID_PM_ERR_ARG, "null ctx pointer");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(SID_PM_ERR_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(SID_PM_ERR_ARG, "device %d out of range (0..%d)", device, n - 1);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SID_PM_ERR_NODEVICE, "device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
    sid_pm_ctx *ctx = new (std::nothrow) sid_pm_ctx();
    if (!ctx) return fail(SID_PM_ERR_NOMEM, "host allocation failed");
    ctx->device = device;
    {
        Guard g(device);
        hipError_t e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
        for (int k = 0; k < 2 && e == hipSuccess; ++k) {
            e = hipEventCreateWithFlags(&ctx->slot_ready[k], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->slot_done[k], hipEventDisableTiming);
        }
        for (int k = 0; k < 3 && e == hipSuccess; ++k) {
            e = hipStreamCreateWithFlags(&ctx->side[k], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->join_ev[k], hipEventDisableTiming);
        }
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&ctx->h_refused), 4 * sizeof(int32_t), hipHostMallocMapped);
        if (e != hipSuccess) { sid_pm_destroy(ctx); return fail(SID_PM_ERR_HIP, "stream/event creation failed: %s", hipGetErrorString(e)); }
        ctx->h_refused[0] = ctx->h_refused[1] = ctx->h_refused[2] = ctx->h_refused[3] = 0;
        int wait_value = 0;
        ctx->can_wait_value = hipDeviceGetAttribute(&wait_value, hipDeviceAttributeCanUseStreamWaitValue, device) == hipSuccess && wait_value != 0;
    }
    *out = ctx;
    return SID_PM_OK;
}

SID_EXPORT void sid_pm_destroy(sid_pm_ctx *ctx)
{
    if (!ctx) return;
    Guard g(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->copy_stream) { (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamDestroy(ctx->copy_stream); }
    for (int k = 0; k < 2; ++k) {
        if (ctx->slot_ready[k]) (void)hipEventDestroy(ctx->slot_ready[k]);
        if (ctx->slot_done[k]) (void)hipEventDestroy(ctx->slot_done[k]);
    }
    for (int k = 0; k < 3; ++k) {
        if (ctx->side[k]) { (void)hipStreamSynchronize(ctx->side[k]); (void)hipStreamDestroy(ctx->side[k]); }
        if (ctx->join_ev[k]) (void)hipEventDestroy(ctx->join_ev[k]);
    }
    if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
    for (int k = 0; k < ctx->n_chain_release; ++k) (void)hipFree(ctx->chain_release[k]);
    if (ctx->chain_count) (void)hipFree(ctx->chain_count);
    sid::lw_workspace_release(ctx->lw);
    if (ctx->h_refused) (void)hipHostFree(ctx->h_refused);
    delete ctx;                                                       // (the DevBuf members free themselves, on the handle's device: `g` is still in scope)
}

SID_EXPORT int sid_pm_set_stream(sid_pm_ctx *ctx, void *hip_stream)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_upload_pair(sid_pm_ctx *ctx, int slot,
                                  const uint8_t *img1, int64_t rows1, int64_t cols1, int64_t stride1,
                                  const uint8_t *img2, int64_t rows2, int64_t cols2, int64_t stride2)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    if (slot < 0 || slot > 1) return fail(SID_PM_ERR_ARG, "slot must be 0 or 1");
    Image h[2] = {{img1, rows1, cols1, stride1}, {img2, rows2, cols2, stride2}};
    if (int rc = check_images(h[0], h[1])) return rc;
    Guard g(ctx->device);
    // The copy runs on the context's copy stream, so that the upload of the next pair overlaps the kernels
    // of the current one (asynchronous when the host buffers are pinned, e.g. hipHostRegister /
    // torch pin_memory; staged synchronously otherwise).  It waits for the kernels that still read this slot.
    if (ctx->done_rec[slot]) HIP_TRY(hipStreamWaitEvent(ctx->copy_stream, ctx->slot_done[slot], 0));
    for (int k = 0; k < 2; ++k) {
        // device copy is packed to a 256-byte multiple pitch (coalesced, dword-aligned rows)
        const int64_t pitch = (h[k].cols + 255) / 256 * 256;
        const size_t need = (size_t)(pitch * h[k].rows);
        if (ctx->own[slot][k].cap < need) {                // growing frees the old buffer: nothing may still read it
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
        }
        if (int rc = ctx->own[slot][k].reserve(need)) return rc;
        HIP_TRY(hipMemcpy2DAsync(ctx->own[slot][k].p, (size_t)pitch, h[k].ptr, (size_t)h[k].stride,
                                 (size_t)h[k].cols, (size_t)h[k].rows, hipMemcpyHostToDevice, ctx->copy_stream));
        ctx->slot_img[slot][k] = Image{ctx->own[slot][k].p, h[k].rows, h[k].cols, pitch};
    }
    HIP_TRY(hipEventRecord(ctx->slot_ready[slot], ctx->copy_stream));
    ctx->ready_rec[slot] = true;
    ++ctx->pair_serial;
    // first pair, refresh of the selected slot, or a borrowed binding is current (an upload replaces it: the
    // caller who streams through both slots switches with select_pair)
    if (!ctx->have_pair || ctx->cur_slot == slot || ctx->cur_slot < 0) {
        ctx->cur[0] = ctx->slot_img[slot][0]; ctx->cur[1] = ctx->slot_img[slot][1];
        ctx->have_pair = true; ctx->cur_slot = slot;
    }
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_select_pair(sid_pm_ctx *ctx, int slot)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    if (slot < 0 || slot > 1 || !ctx->slot_img[slot][0].ptr) return fail(SID_PM_ERR_STATE, "slot %d holds no pair", slot);
    ctx->cur[0] = ctx->slot_img[slot][0]; ctx->cur[1] = ctx->slot_img[slot][1];
    ctx->have_pair = true; ctx->cur_slot = slot;
    ++ctx->pair_serial;
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_bind_pair(sid_pm_ctx *ctx,
                                const uint8_t *d_img1, int64_t rows1, int64_t cols1, int64_t stride1,
                                const uint8_t *d_img2, int64_t rows2, int64_t cols2, int64_t stride2)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    Image d[2] = {{d_img1, rows1, cols1, stride1}, {d_img2, rows2, cols2, stride2}};
    if (int rc = check_images(d[0], d[1])) return rc;
    ctx->cur[0] = d[0]; ctx->cur[1] = d[1];
    ctx->have_pair = true; ctx->cur_slot = -1;
    ++ctx->pair_serial;
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_set_points(sid_pm_ctx *ctx, const double *c1, const double *r1, const double *c2fg,
                                 const double *r2fg, const double *border, int64_t n, int img_size,
                                 double alpha0, const double *angles, const double *rot, int n_angles,
                                 uint32_t flags)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    if (n < 0 || n > 0x7fffffff / 8) return fail(SID_PM_ERR_ARG, "bad point count");
    if (n > 0 && (!c1 || !r1 || !c2fg || !r2fg || !border)) return fail(SID_PM_ERR_ARG, "null point vector");
    if (int rc = check_sweep(img_size, angles, n_angles, flags)) return rc;
    if (!ctx->have_pair) return fail(SID_PM_ERR_STATE, "set_points needs an image pair (upload_pair/bind_pair first)");
    Guard g(ctx->device);
    const int s = img_size, K = n_angles;
    const Switches sw = read_switches();

    (void)alpha0;
    std::vector<double> rotv;
    if (int rc = make_rot(K, rot, rotv)) return rc;
    std::vector<uint16_t> sampv;
    int nflag = 0;
    // (rot_order = 1: no offset table - every template sample is interpolated in float64 by the general sampler)
    if (!sw.no_samp_table && ((flags >> 3) & 7u) == 0u && sid::mfma_img_size_supported(s)) nflag = make_samp(rotv, K, s, sampv);
    std::vector<uint32_t> samp2v;
    // (measured +2 % on the 15-angle step - fifteen table loads per angle instead of five, a uniform branch per chunk - although
    // it executes a third fewer VALU instructions in the template phase: built on request only, SID_PM_SAMP2=1)
    if (!sampv.empty() && use_rp(sw, s) && sw.samp2) make_samp2(sampv, K, s, samp2v);

    // one arena, one upload: the layout of pm_host.h measures it, carves the host image and carves the device block
    auto layout = [&](Carver &c) { return point_arena(c, (size_t)n, (size_t)K, sampv.size(), samp2v.size()); };
    Carver measure;
    layout(measure);
    const size_t total = measure.off;
    HIP_TRY(hipStreamSynchronize(ctx->stream));               // nothing may still read the old arena
    if (int rc = ctx->arena.reserve(total)) return rc;
    if (int rc = ctx->out.reserve((size_t)(5 * n))) return rc;
    if (int rc = ctx->out_ij.reserve((size_t)(3 * n))) return rc;
    std::vector<uint8_t> host(total, 0);
    Carver on_host(host.data()), on_device(ctx->arena.p);
    const PointArena h = layout(on_host), d = layout(on_device);
    const double *src[5] = {c1, r1, c2fg, r2fg, border};
    for (int k = 0; k < 5 && n > 0; ++k) memcpy(h.vec + (size_t)(k * n), src[k], sizeof(double) * (size_t)n);
    memcpy(h.angles, angles, sizeof(double) * (size_t)K);
    memcpy(h.rot, rotv.data(), sizeof(double) * rotv.size());
    if (!sampv.empty()) memcpy(h.samp, sampv.data(), sizeof(uint16_t) * sampv.size());
    if (!samp2v.empty()) memcpy(h.samp2, samp2v.data(), sizeof(uint32_t) * samp2v.size());
    // synchronous: the host vectors are caller-owned and not retained
    HIP_TRY(hipMemcpy(ctx->arena.p, host.data(), total, hipMemcpyHostToDevice));
    ctx->d_vec = d.vec; ctx->d_angles = d.angles; ctx->d_rot = d.rot; ctx->d_order = d.order; ctx->d_samp = d.samp; ctx->d_samp2 = d.samp2;
    ctx->have_samp = !sampv.empty(); ctx->samp_nflag = nflag;
    ctx->h_c2fg.assign(c2fg, c2fg + n); ctx->h_r2fg.assign(r2fg, r2fg + n); ctx->h_border.assign(border, border + n);
    ctx->h_c1.assign(c1, c1 + n); ctx->h_r1.assign(r1, r1 + n);

    ctx->user_out = nullptr; ctx->user_ij = nullptr;
    ctx->n = n; ctx->img_size = s; ctx->n_angles = K; ctx->flags = flags; ctx->rp = use_rp(sw, s); ctx->rp_paired = ctx->rp ? rp_paired(sw, K) : 0;
    ctx->have_points = false;
    ++ctx->points_serial;
    if (int rc = classify_points(ctx)) return rc;
    ctx->have_points = true;
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_bind_results(sid_pm_ctx *ctx, double *d_out, int32_t *d_out_ij)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    if (!ctx->have_points) return fail(SID_PM_ERR_STATE, "bind_results before set_points");
    if (!d_out && d_out_ij) return fail(SID_PM_ERR_ARG, "d_out_ij without d_out");
    ctx->user_out = d_out; ctx->user_ij = d_out_ij;
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_run(sid_pm_ctx *ctx)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    if (!ctx->have_points || !ctx->have_pair) return fail(SID_PM_ERR_STATE, "run needs set_points and an image pair");
    Guard g(ctx->device);
    // the launch classes were sized for the image-2 shape current at set_points; a pair of another shape
    // (select_pair / bind_pair / upload_pair since then) gets its own classification before anything is launched
    if (ctx->cur[1].rows != ctx->cls_rows2 || ctx->cur[1].cols != ctx->cls_cols2) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (int rc = classify_points(ctx)) return rc;
    }
    const Switches run_sw = read_switches();                          // (the five switches of a run: side_by_side, side_first, no_chain, verbose, debug_check)
    const std::vector<Bucket> &buckets = ctx->plan.buckets;
    sid::PMArgs A;
    fill_args(ctx, run_sw, A);
    if (ctx->cur_slot >= 0 && ctx->ready_rec[ctx->cur_slot])
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->slot_ready[ctx->cur_slot], 0));
    {   // rot_order 2..5: spline coefficients of image 1 (once per pair), templates of the points sampled from them (once per pair and point set)
        const int order = (int)((ctx->flags >> 3) & 7u);
        if (int rc = ensure_coef(ctx, order)) return rc;
        if (!buckets.empty()) { if (int rc = ensure_presampled(ctx, order)) return rc; }
        A.pre = (order >= 2 && !buckets.empty()) ? ctx->pre.p : nullptr;
    }
    // the order of the launches: decided by pm_plan.h launch_schedule (why short runs go side by side and long ones are chained
    // is told there); the signal memory of a chained run is asked for only when everything else says "chained"
    Schedule S = launch_schedule(run_sw, buckets, ctx->rp, ctx->can_wait_value, true);
    if (S.order == Schedule::kChained && !ensure_chain_memory(ctx, buckets.size())) S = launch_schedule(run_sw, buckets, ctx->rp, ctx->can_wait_value, false);
    if (run_sw.verbose) {
        static const char *const kOrder[] = {"sequence", "side by side", "chained"};
        static const char *const kWhy[] = {"", "", "", "", " (not chained: the device lacks stream wait-value support)", " (not chained: no signal memory)"};
        fprintf(stderr, "sid_pm: launch order %s, %zu launches%s\n", kOrder[S.order], buckets.size(), kWhy[S.why]);
    }
    if (S.record_fork) HIP_TRY(hipEventRecord(ctx->fork_ev, ctx->stream));
    const unsigned long long epoch = S.order == Schedule::kChained ? ++ctx->chain_epoch : 0ull;
    unsigned used = 0;                                               // side streams that carry work the handle's stream has not joined yet
    auto join = [&]() -> int {
        for (int k = 0; k < 3; ++k)                                  // the handle's stream continues when every side launch is done
            if (used & (1u << k)) {
                HIP_TRY(hipEventRecord(ctx->join_ev[k], ctx->side[k]));
                HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->join_ev[k], 0));
            }
        used = 0;
        return SID_PM_OK;
    };
    // a failure midway: no stream of the handle is left waiting (release_upto), and what the side streams already hold still
    // orders before the handle's stream
    auto abandon = [&](size_t k, const char *what, hipError_t e) {
        for (int j = 0; j <= release_upto(S, k); ++j) __atomic_store_n(ctx->chain_release[j], epoch, __ATOMIC_RELEASE);
        (void)join();
        return fail(SID_PM_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    };
    for (size_t k = 0; k < buckets.size(); ++k) {
        const Bucket &b = buckets[k];
        const LaunchStep &step = S.steps[k];
        if (step.join_before) { if (int rc = join()) return rc; }
        const hipStream_t st = step.stream < 0 ? ctx->stream : ctx->side[step.stream];
        if (step.stream >= 0) used |= 1u << step.stream;
        hipError_t we = hipSuccess;
        if (step.wait_fork) we = hipStreamWaitEvent(st, ctx->fork_ev, 0);
        if (we == hipSuccess && step.wait_release >= 0) we = hipStreamWaitValue64(st, ctx->chain_release[step.wait_release], epoch, hipStreamWaitValueGte);
        if (we != hipSuccess) return abandon(k, S.order == Schedule::kChained ? "chained launch: stream wait" : "stream wait", we);
        A.chain.count = step.counts_arrival ? ctx->chain_count + k * sid::kChainWords : nullptr;
        A.chain.release = step.counts_arrival ? ctx->chain_release[k] : nullptr;
        A.chain.epoch = step.counts_arrival ? epoch : 0;
        A.order = ctx->d_order + b.offset;
        A.gsii_off = ctx->d_goff.p ? ctx->d_goff.p + b.offset : nullptr;
        A.rec = ctx->d_rec.p ? ctx->d_rec.p + b.offset : nullptr;
        A.n_launch = b.count;
        A.gs_keep_acc = b.keep ? 1u : 0u;
        A.ring = (b.pooled && ctx->plan.pool_stride) ? ctx->ring.p : nullptr;
        const int lds_launch = std::min(b.lds, sid::max_lds_bytes());
        A.lds_bytes = lds_launch;
        const int nthreads = launch_shape(b, ctx->rp).nthreads;
        const int e = ctx->rp
                          ? sid::launch_pm_rp(A, lds_launch, nthreads, b.band, b.big ? 0 : ctx->rp_paired, b.pitch, b.occ, st, b.big)
                          : sid::launch_pm_mfma(A, lds_launch, nthreads, b.band, use_paired(ctx->plan.sw, ctx->n_angles), st);
        if (e != 0) return abandon(k, "kernel launch", (hipError_t)e);
    }
    if (int rc = join()) return rc;
    if (int rc = run_large_points(ctx, A)) return rc;
    if (ctx->cur_slot >= 0) {
        HIP_TRY(hipEventRecord(ctx->slot_done[ctx->cur_slot], ctx->stream));
        ctx->done_rec[ctx->cur_slot] = true;
    }
    return SID_PM_OK;
}

// Valid points the kernels refused since the last check (the launch their classification put them in could not hold
// their LDS layout: host and device disagree - a bug, reported as an error instead of the NaN row the point received).
// Reads a pinned host word: call it once the launch stream is synchronised, by whatever means.
SID_EXPORT int sid_pm_check(sid_pm_ctx *ctx)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    if (!ctx->h_refused) return SID_PM_OK;
    const int32_t n = __atomic_exchange_n(ctx->h_refused, 0, __ATOMIC_ACQ_REL);
    const int32_t polls = __atomic_exchange_n(ctx->h_refused + 1, 0, __ATOMIC_ACQ_REL);
    if (polls > 0 && read_switches().verbose) fprintf(stderr, "sid_pm: %d workgroup(s) found the home words of their XCD's free list empty and took a block of its reserve words\n", (int)polls);
    if (n != 0)
        return fail(SID_PM_ERR_STATE, "%d grid point(s) with a valid search window were refused by their launch (LDS layout of the "
                                      "kernel and classification of the host disagree, or all %d recycled blocks of global memory of an XCD "
                                      "were taken - %d pops went to the reserve words); their rows hold NaN", (int)n, sid::kRingWordsPerXcd * 64, (int)polls);
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_sync(sid_pm_ctx *ctx)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    Guard g(ctx->device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return sid_pm_check(ctx);
}

SID_EXPORT int sid_pm_fetch(sid_pm_ctx *ctx, double *out, int32_t *out_ij)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    if (!ctx->have_points) return fail(SID_PM_ERR_STATE, "fetch before set_points");
    if (ctx->n > 0 && !out) return fail(SID_PM_ERR_ARG, "null out");
    Guard g(ctx->device);
    if (ctx->n > 0) {
        const double *src = ctx->user_out ? ctx->user_out : ctx->out.p;
        const int32_t *src_ij = ctx->user_out ? ctx->user_ij : ctx->out_ij.p;
        HIP_TRY(hipMemcpyAsync(out, src, sizeof(double) * 5 * (size_t)ctx->n, hipMemcpyDeviceToHost, ctx->stream));
        if (out_ij && src_ij)
            HIP_TRY(hipMemcpyAsync(out_ij, src_ij, sizeof(int32_t) * 3 * (size_t)ctx->n, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->dbg_err.p) {
        int32_t e[320];
        if (hipMemcpy(e, ctx->dbg_err.p, sizeof e, hipMemcpyDeviceToHost) == hipSuccess && (e[0] || e[1] || e[2] || e[3])) {
            if (e[4] > 0) {
                fprintf(stderr, "first event, (i,j got want):");
                for (int k = 0; k < e[4] && k < 200; ++k) fprintf(stderr, " (%d,%d %d %d)", (e[64 + k] >> 24) & 255, (e[64 + k] >> 16) & 255, (e[64 + k] >> 8) & 255, e[64 + k] & 255);
                fprintf(stderr, "\n");
            }
            fprintf(stderr, "SID_PM_DEBUG_CHECK: sum mismatches after sampling %d, after sweep %d; table bytes != exact resampling %d (pt %d slot %d n %d); patch bytes != image %d;", e[0], e[1], e[2], e[40], e[41], e[42], e[3]);
            for (int t = 0; t < 2; ++t) for (int k = 0; k < 4 && k < e[t]; ++k)
                fprintf(stderr, " [tag %d pt %d slot %d dST %d dSTT %d]", t, e[8 + 16 * t + 4 * k], e[9 + 16 * t + 4 * k], e[10 + 16 * t + 4 * k], e[11 + 16 * t + 4 * k]);
            fprintf(stderr, "\n");
            (void)hipMemset(ctx->dbg_err.p, 0, sizeof e);
        }
    }
    return sid_pm_check(ctx);
}

// ---- exchange step of the N-GPU path: the gathered per-rank blocks -> original point order, in ONE pass ----
// stack: `world` blocks of m rows [m x 5 float64 | m x 3 int32] (what every rank's kernels wrote, gathered by RCCL);
// perm[i] = row of point i in the stacked blocks.  One thread per (point, field): eight threads move the 52 bytes of a
// point, so the writes of a wavefront are 8 x 40 + 8 x 12 contiguous bytes.  `out` / `out_ij` may be pinned host memory:
// the results then reach the host without a copy after the kernel (posted PCIe writes).
namespace {
__global__ void unpermute_rows_kernel(const uint8_t *stack, int64_t m, const int32_t *perm, int64_t n, double *out, int32_t *out_ij)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = t >> 3;
    const int f = (int)(t & 7);
    if (i >= n) return;
    const int64_t row = perm[i], blk = row / m, r = row - blk * m;
    const uint8_t *base = stack + blk * m * 52;
    if (f < 5) out[i * 5 + f] = reinterpret_cast<const double *>(base)[r * 5 + f];
    else if (out_ij) out_ij[i * 3 + (f - 5)] = reinterpret_cast<const int32_t *>(base + m * 40)[r * 3 + (f - 5)];
}
}  // namespace

SID_EXPORT int sid_pm_unpermute(const void *d_stack, int64_t world, int64_t m, const int32_t *d_perm, int64_t n,
                                double *out, int32_t *out_ij, void *hip_stream)
{
    if (n < 0 || world < 1 || m < 1 || (m & 1) || (n > 0 && (!d_stack || !d_perm || !out)))
        return fail(SID_PM_ERR_ARG, "unpermute: bad argument (rows per block must be even: the blocks then keep their doubles aligned)");
    if (n == 0) return SID_PM_OK;
    const int64_t threads = n * 8;
    hipLaunchKernelGGL(unpermute_rows_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream),
                       static_cast<const uint8_t *>(d_stack), m, d_perm, n, out, out_ij);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SID_PM_ERR_HIP, "unpermute: %s", hipGetErrorString(e));
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_device_results(sid_pm_ctx *ctx, double **d_out, int32_t **d_out_ij)
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    if (!ctx->have_points) return fail(SID_PM_ERR_STATE, "device_results before set_points");
    if (d_out) *d_out = ctx->user_out ? ctx->user_out : ctx->out.p;
    if (d_out_ij) *d_out_ij = ctx->user_out ? ctx->user_ij : ctx->out_ij.p;
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_work_info(sid_pm_ctx *ctx, double info[6])
{
    if (!ctx || !info) return fail(SID_PM_ERR_ARG, "null argument");
    if (!ctx->have_points) return fail(SID_PM_ERR_STATE, "work_info before set_points");
    memcpy(info, ctx->plan.info, sizeof ctx->plan.info);
    info[5] = 0;
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_batch(const uint8_t *img1, int64_t rows1, int64_t cols1, int64_t stride1,
                            const uint8_t *img2, int64_t rows2, int64_t cols2, int64_t stride2,
                            const double *c1, const double *r1, const double *c2fg, const double *r2fg,
                            const double *border, int64_t n, int img_size, double alpha0,
                            const double *angles, const double *rot, int n_angles, uint32_t flags,
                            double *out, int32_t *out_ij)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(SID_PM_ERR_NODEVICE, "no current HIP device");
    sid_pm_ctx *ctx = nullptr;
    int rc = sid_pm_create(dev, &ctx);
    if (rc) return rc;
    rc = sid_pm_upload_pair(ctx, 0, img1, rows1, cols1, stride1, img2, rows2, cols2, stride2);
    if (!rc) rc = sid_pm_set_points(ctx, c1, r1, c2fg, r2fg, border, n, img_size, alpha0, angles, rot, n_angles, flags);
    if (!rc) rc = sid_pm_run(ctx);
    if (!rc) rc = sid_pm_fetch(ctx, out, out_ij);
    const std::string keep = g_err;
    sid_pm_destroy(ctx);
    if (rc) g_err = keep;
    return rc;
}

// ---- rotate_and_match / get_template / get_hessian as calls of their own (reference pmlib.py:117-174, :89-115, :36-59) ----
SID_EXPORT int sid_pm_rotate_and_match(sid_pm_ctx *ctx, double c1, double r1, int img_size,
                                       int64_t win_row0, int64_t win_col0, int64_t win_rows, int64_t win_cols,
                                       double alpha0, const double *angles, const double *rot, int n_angles, uint32_t flags,
                                       double out5[5], int32_t ij3[3], float *ccm, int64_t ccm_cap, uint8_t *best_template)
{
    (void)alpha0;
    if (!ctx || !out5) return fail(SID_PM_ERR_ARG, "null argument");
    if (!ctx->have_pair) return fail(SID_PM_ERR_STATE, "rotate_and_match needs an image pair (upload_pair / bind_pair first)");
    if (int rc = check_sweep(img_size, angles, n_angles, flags)) return rc;
    if (!rot) return fail(SID_PM_ERR_ARG, "rot is required: the rotation terms as the caller's NumPy computed them (pmlib.py:105-110)");
    const int s = img_size, K = n_angles;
    if (win_row0 < 0 || win_col0 < 0 || win_rows < 1 || win_cols < 1 || win_row0 + win_rows > ctx->cur[1].rows || win_col0 + win_cols > ctx->cur[1].cols)
        return fail(SID_PM_ERR_ARG, "the window does not lie inside image 2");
    // cv2.matchTemplate needs a window at least as large as the template, np.gradient two values along each axis (pmlib.py:156, :51)
    if (win_rows - s + 1 < 2 || win_cols - s + 1 < 2)
        return fail(SID_PM_ERR_ARG, "window %lldx%lld: fewer than two placements of a %d px template along an axis", (long long)win_rows, (long long)win_cols, s);
    if (win_rows > 65535 || win_cols > 4000000)
        return fail(SID_PM_ERR_UNSUPPORTED, "window %lldx%lld too large (at most 65535 rows: a launch dimension of the large-window pipeline)", (long long)win_rows, (long long)win_cols);
    const int64_t np = (win_rows - s + 1) * (win_cols - s + 1);
    if (np >= 0xffffffffll) return fail(SID_PM_ERR_UNSUPPORTED, "more than 2^32 placements");
    if (ccm && ccm_cap < np) return fail(SID_PM_ERR_ARG, "ccm capacity %lld < %lld placements", (long long)ccm_cap, (long long)np);
    Guard g(ctx->device);
    // small device block: [K angles | 4K rotation terms | 5 results | 3 int32]
    if (int rc = ctx->lw_small.reserve((size_t)K * 5 + 8)) return rc;
    std::vector<double> host((size_t)K * 5);
    memcpy(host.data(), angles, sizeof(double) * (size_t)K);
    memcpy(host.data() + K, rot, sizeof(double) * 4 * (size_t)K);
    HIP_TRY(hipMemcpyAsync(ctx->lw_small.p, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (`host` is a local)
    if (ctx->cur_slot >= 0 && ctx->ready_rec[ctx->cur_slot]) HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->slot_ready[ctx->cur_slot], 0));
    sid::LargeCall c;
    c.img1 = ctx->cur[0].ptr; c.rows1 = ctx->cur[0].rows; c.cols1 = ctx->cur[0].cols; c.stride1 = ctx->cur[0].stride;
    c.img2 = ctx->cur[1].ptr; c.stride2 = ctx->cur[1].stride;
    c.win_r0 = win_row0; c.win_c0 = win_col0; c.wh = (int)win_rows; c.ww = (int)win_cols;
    c.c1 = c1; c.r1 = r1; c.s = s; c.K = K; c.flags = flags;
    if (int rc = ensure_coef(ctx, (int)((flags >> 3) & 7u))) return rc;
    c.d_coef = ((flags >> 3) & 7u) >= 2u ? ctx->coef[1].p : nullptr;
    c.d_angles = ctx->lw_small.p; c.d_rot = ctx->lw_small.p + K;
    c.add_c = 0.0; c.add_r = 0.0;
    gauss_taps(c.gauss_w);
    c.out5 = ctx->lw_small.p + 5 * (size_t)K;
    c.ij3 = reinterpret_cast<int32_t *>(ctx->lw_small.p + 5 * (size_t)K + 5);
    const int e = sid::lw_run(c, ctx->lw, ctx->stream);
    if (e == -1) return fail(SID_PM_ERR_NOMEM, "rotate_and_match needs %.2f GB of device scratch for a %dx%d window and %d angles",
                             (double)sid::lw_scratch_bytes(c.wh, c.ww, s, K, flags) * 1e-9, c.wh, c.ww, K);
    if (e) return fail(SID_PM_ERR_HIP, "large-window pipeline: %s", hipGetErrorString((hipError_t)e));
    if (ctx->cur_slot >= 0) { HIP_TRY(hipEventRecord(ctx->slot_done[ctx->cur_slot], ctx->stream)); ctx->done_rec[ctx->cur_slot] = true; }
    int32_t ij[3] = {-1, -1, -1};
    HIP_TRY(hipMemcpyAsync(out5, c.out5, sizeof(double) * 5, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ij, c.ij3, sizeof ij, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ij3) memcpy(ij3, ij, sizeof ij);
    if (ij[2] >= 0) {                                                 // (a NaN point has no matrix and no template: pmlib.py:152-154)
        if (ccm) HIP_TRY(hipMemcpy(ccm, sid::lw_ncc_matrix(ctx->lw, c.wh, c.ww, s, ij[2]), sizeof(float) * (size_t)np, hipMemcpyDeviceToHost));
        if (best_template) HIP_TRY(hipMemcpy(best_template, sid::lw_template(ctx->lw, s, ij[2]), (size_t)s * s, hipMemcpyDeviceToHost));
    }
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_get_template(int device, const uint8_t *img, int64_t rows, int64_t cols, int64_t stride, double c, double r,
                                   const double rot4[4], int img_size, int rot_order, uint8_t *out)
{
    if (!img || !rot4 || !out || rows < 1 || cols < 1 || stride < cols) return fail(SID_PM_ERR_ARG, "bad argument");
    if (img_size < 1 || img_size > 4096) return fail(SID_PM_ERR_UNSUPPORTED, "img_size=%d", img_size);
    if (rot_order < 0 || rot_order > 5) return fail(SID_PM_ERR_UNSUPPORTED, "rot_order=%d: scipy's spline orders are 0..5", rot_order);
    if (!(fabs(c) < 1e15 && fabs(r) < 1e15)) return fail(SID_PM_ERR_ARG, "non-finite centre");
    // (make_rot's rule, before any device call: `reach` below goes through floor() and a cast)
    for (int k = 0; k < 4; ++k) if (!(fabs(rot4[k]) < 1e6)) return fail(SID_PM_ERR_ARG, "rot4 holds a non-finite or absurd value");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(SID_PM_ERR_NODEVICE, "no such device");
    Guard g(device);
    const int s = img_size;
    // only the part of the image the samples can touch travels to the device: the samples lie within hypot(s, s) + |tcT| of (r, c)
    const double reach = 1.5 * (double)s + fabs(rot4[2]) + fabs(rot4[3]) + 4.0;
    // (orders 2..5: scipy prefilters the WHOLE image - pmlib.py:112-113 - so the whole image travels)
    const bool whole = rot_order >= 2;
    const int64_t row0 = whole ? 0 : std::max<int64_t>(0, (int64_t)floor(r - reach)), row1 = whole ? rows : std::min<int64_t>(rows, (int64_t)ceil(r + reach) + 1);
    const int64_t col0 = whole ? 0 : std::max<int64_t>(0, (int64_t)floor(c - reach)), col1 = whole ? cols : std::min<int64_t>(cols, (int64_t)ceil(c + reach) + 1);
    DevBuf<uint8_t> dimg, dout;
    DevBuf<double> drot, dcoef0, dcoef1;
    int rc = SID_PM_OK;
    const int64_t nr = std::max<int64_t>(row1 - row0, 0), nc = std::max<int64_t>(col1 - col0, 0);
    if ((rc = dimg.reserve((size_t)std::max<int64_t>(nr * nc, 1))) || (rc = dout.reserve((size_t)s * s)) || (rc = drot.reserve(4)) ||
        (whole && ((rc = dcoef0.reserve((size_t)(rows * cols))) || (rc = dcoef1.reserve((size_t)(rows * cols))))))
        return rc;
    hipError_t e = hipSuccess;
    if (nr > 0 && nc > 0) e = hipMemcpy2D(dimg.p, (size_t)nc, img + row0 * stride + col0, (size_t)stride, (size_t)nc, (size_t)nr, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(drot.p, rot4, sizeof(double) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && whole) e = (hipError_t)sid::lw_spline_prefilter(dimg.p, rows, cols, nc, rot_order, dcoef0.p, dcoef1.p, nullptr);
    // (a template wholly outside the image samples nothing: every coordinate fails the bounds test and yields 0)
    if (e == hipSuccess) e = (hipError_t)sid::lw_get_template(dimg.p, nc > 0 ? nc : 1, row0, col0, nr, nc, rows, cols, c, r, drot.p, s, rot_order, dout.p, nullptr, whole ? dcoef1.p : nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, (size_t)s * s, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(SID_PM_ERR_HIP, "get_template: %s", hipGetErrorString(e));
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_get_hessian(int device, const float *ccm, int64_t rows, int64_t cols, uint32_t flags, float *hes)
{
    if (!ccm || !hes) return fail(SID_PM_ERR_ARG, "null argument");
    if (flags & ~(SID_PM_HES_NORM | SID_PM_HES_SMTH)) return fail(SID_PM_ERR_ARG, "get_hessian takes SID_PM_HES_NORM and SID_PM_HES_SMTH");
    // np.gradient needs two values along each axis (pmlib.py:51)
    if (rows < 2 || cols < 2 || rows * cols >= 0xffffffffll) return fail(SID_PM_ERR_ARG, "matrix %lldx%lld: at least 2x2, fewer than 2^32 values", (long long)rows, (long long)cols);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(SID_PM_ERR_NODEVICE, "no such device");
    Guard g(device);
    const size_t n = (size_t)(rows * cols);
    DevBuf<float> din, dout;
    sid::LwWorkspace W;
    struct Scope { sid::LwWorkspace &w; ~Scope() { sid::lw_workspace_release(w); } } w_scope{W};
    int rc = SID_PM_OK;
    if ((rc = din.reserve(n)) || (rc = dout.reserve(n))) return rc;
    double gw[5];
    gauss_taps(gw);
    hipError_t e = hipMemcpy(din.p, ccm, sizeof(float) * n, hipMemcpyHostToDevice);
    int le = 0;
    if (e == hipSuccess) le = sid::lw_get_hessian(din.p, (int)rows, (int)cols, flags, gw, dout.p, W, nullptr);
    if (le == 0 && e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (le == 0 && e == hipSuccess) e = hipMemcpy(hes, dout.p, sizeof(float) * n, hipMemcpyDeviceToHost);
    if (le == -1) return fail(SID_PM_ERR_NOMEM, "get_hessian: device scratch");
    if (le) return fail(SID_PM_ERR_HIP, "get_hessian: %s", hipGetErrorString((hipError_t)le));
    if (e != hipSuccess) return fail(SID_PM_ERR_HIP, "get_hessian: %s", hipGetErrorString(e));
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_debug_point(sid_pm_ctx *ctx, double c1, double r1, double c2fg, double r2fg,
                                  double border, int img_size, double alpha0, const double *angles,
                                  const double *rot, int n_angles, uint32_t flags,
                                  uint8_t *templates, float *ccm, float *hes, int64_t cap, int32_t rh_rw[2],
                                  double out5[5], int32_t ij3[3], int64_t phase_cycles[32])
{
    if (!ctx) return fail(SID_PM_ERR_ARG, "null ctx");
    if (!ctx->have_pair) return fail(SID_PM_ERR_STATE, "debug_point needs an image pair");
    if (int rc = check_sweep(img_size, angles, n_angles, flags)) return rc;
    Guard g(ctx->device);
    const int s = img_size, K = n_angles;
    const Switches sw = read_switches();
    const bool rp = use_rp(sw, s);
    const int rpp = rp ? rp_paired(sw, K) : 0;
    int wh = 0, ww = 0, lds = lds_need(sw, rp, rpp, s + 1, s + 1, s, K, flags);
    bool clipped = false;
    if (window_dims(c2fg, r2fg, border, s, ctx->cur[1].rows, ctx->cur[1].cols, wh, ww, &clipped))
        lds = lds_need(sw, rp, rpp, wh, ww, s, K, flags);
    // (the one-point kernels do not take windows clipped by the edge of image 2: the batch entry points run them through the
    // large-window pipeline - classify_points)
    if (clipped) return fail(SID_PM_ERR_UNSUPPORTED, "debug_point: the search window is clipped by the edge of image 2 (%dx%d); "
                                                     "sid_pm_run / sid_pm_batch take such points", wh, ww);
    if (lds > sid::max_lds_bytes()) return fail(SID_PM_ERR_UNSUPPORTED, "search window too large for LDS");
    (void)alpha0;
    if (!sid::mfma_img_size_supported(s)) return fail(SID_PM_ERR_UNSUPPORTED, "debug_point: template sides 2..64 (sid_pm_rotate_and_match returns the matrix and the template of any size)");
    std::vector<double> rotv;
    if (int rc = make_rot(K, rot, rotv)) return rc;

    DevBuf<double> dv, dang, drot, dout;
    DevBuf<int32_t> dord, dij, dshape;
    DevBuf<uint8_t> dt;
    DevBuf<uint16_t> dsamp;
    std::vector<uint16_t> sampv;
    int nflag = 0;
    // (rot_order = 1: no offset table - every template sample is interpolated in float64 by the general sampler)
    if (!sw.no_samp_table && ((flags >> 3) & 7u) == 0u) nflag = make_samp(rotv, K, s, sampv);
    DevBuf<float> dccm, dhes;
    DevBuf<uint8_t> dpre;                                              // rot_order 2..5: this point's templates, sampled from the spline coefficients
    DevBuf<long long> dcyc;
    DevBuf<uint32_t> dgs;                                              // row-pair kernel: this point's sum w'^2 block + its offset (0)
    DevBuf<sid::PointRec> drec;                                        // ... and its record
    int rc = SID_PM_OK;
    const size_t tcount = (size_t)K * s * s;
    if ((rc = dv.reserve(5)) || (rc = dang.reserve((size_t)K)) || (rc = drot.reserve(4 * (size_t)K)) ||
        (rc = dout.reserve(5)) || (rc = dord.reserve(1)) || (rc = dij.reserve(3)) || (rc = dshape.reserve(2)) ||
        (rc = dt.reserve(tcount)) || (rc = dccm.reserve((size_t)std::max<int64_t>(cap, 1))) ||
        (rc = dhes.reserve((size_t)std::max<int64_t>(cap, 1))) || (rc = dcyc.reserve(32)) ||
        (rc = dsamp.reserve(sampv.size() + 4)) || (rc = dgs.reserve(64 + (size_t)(wh > s ? sid::rp_block_entries(wh - s + 1, ww - s + 1, rp_rows(rpp, 4), 16 >> rpp, false, keep_acc_policy(sw, rp, rpp, K)) : 64))) || (rc = drec.reserve(1))) return rc;
    const double v5[5] = {c1, r1, c2fg, r2fg, border};
    const int32_t zero = 0, shape0[2] = {0, 0};
    hipError_t e = hipSuccess;
    auto step = [&](hipError_t x) { if (e == hipSuccess) e = x; };
    step(hipStreamSynchronize(ctx->stream));
    if (ctx->copy_stream) step(hipStreamSynchronize(ctx->copy_stream));   // a pending upload of the selected pair
    step(hipMemcpy(dv.p, v5, sizeof v5, hipMemcpyHostToDevice));
    step(hipMemcpy(dang.p, angles, sizeof(double) * K, hipMemcpyHostToDevice));
    step(hipMemcpy(drot.p, rotv.data(), sizeof(double) * rotv.size(), hipMemcpyHostToDevice));
    step(hipMemcpy(dord.p, &zero, sizeof zero, hipMemcpyHostToDevice));
    step(hipMemset(dgs.p, 0, 64 * sizeof(uint32_t)));                  // entry 0 = the offset (0 granules); the block starts at entry 64
    {
        const sid::PointRec r1rec{0, 0u, c1, r1, c2fg, r2fg, border};
        step(hipMemcpy(drec.p, &r1rec, sizeof r1rec, hipMemcpyHostToDevice));
    }
    if (!sampv.empty()) step(hipMemcpy(dsamp.p, sampv.data(), sizeof(uint16_t) * sampv.size(), hipMemcpyHostToDevice));
    step(hipMemcpy(dshape.p, shape0, sizeof shape0, hipMemcpyHostToDevice));
    step(hipMemset(dt.p, 0, tcount));
    step(hipMemset(dcyc.p, 0, sizeof(long long) * 32));
    if (cap > 0) { step(hipMemset(dccm.p, 0, sizeof(float) * cap)); step(hipMemset(dhes.p, 0, sizeof(float) * cap)); }
    if (e == hipSuccess) {
        sid::PMArgs A;
        memset(&A, 0, sizeof A);
        set_images(ctx, A);
        A.c1 = dv.p; A.r1 = dv.p + 1; A.c2fg = dv.p + 2; A.r2fg = dv.p + 3; A.border = dv.p + 4;
        A.order = dord.p; A.n_launch = 1; A.img_size = s; A.n_angles = K; A.flags = flags;
        A.angles = dang.p; A.rot = drot.p; A.out = dout.p; A.out_ij = dij.p;
        A.dbg_templates = dt.p; A.dbg_ccm = dccm.p; A.dbg_hes = dhes.p; A.dbg_shape = dshape.p; A.dbg_cap = cap;
        A.dbg_cycles = dcyc.p;
        gauss_taps(A.gauss_w);
        A.samp = sampv.empty() ? nullptr : dsamp.p; A.samp_nflag = nflag;
        A.lds_bytes = lds;
        const int order = (int)((flags >> 3) & 7u);
        if (order >= 2) {
            if (int rc2 = ensure_coef(ctx, order)) return rc2;
            if (int rc2 = dpre.reserve(tcount)) return rc2;
            step((hipError_t)sid::lw_presample(ctx->coef[1].p, ctx->cur[0].rows, ctx->cur[0].cols, dv.p, dv.p + 1, 1, drot.p, K, s, order, dpre.p, ctx->stream));
            A.pre = dpre.p;
        }
        A.gsii = dgs.p + 64; A.gsii_off = dgs.p; A.rec = drec.p;
        A.gs_keep_acc = keep_acc_policy(sw, rp, rpp, K) ? 1u : 0u;
        step((hipError_t)(rp ? sid::launch_pm_rp(A, lds, 256, 4, rpp, 0, 3, ctx->stream)
                                       : sid::launch_pm_mfma(A, lds, 256, 4, use_paired(sw, K), ctx->stream)));
        step(hipStreamSynchronize(ctx->stream));
        if (templates) step(hipMemcpy(templates, dt.p, tcount, hipMemcpyDeviceToHost));
        if (ccm && cap > 0) step(hipMemcpy(ccm, dccm.p, sizeof(float) * cap, hipMemcpyDeviceToHost));
        if (hes && cap > 0) step(hipMemcpy(hes, dhes.p, sizeof(float) * cap, hipMemcpyDeviceToHost));
        if (rh_rw) step(hipMemcpy(rh_rw, dshape.p, sizeof(int32_t) * 2, hipMemcpyDeviceToHost));
        if (out5) step(hipMemcpy(out5, dout.p, sizeof(double) * 5, hipMemcpyDeviceToHost));
        if (ij3) step(hipMemcpy(ij3, dij.p, sizeof(int32_t) * 3, hipMemcpyDeviceToHost));
        if (phase_cycles) step(hipMemcpy(phase_cycles, dcyc.p, sizeof(long long) * 32, hipMemcpyDeviceToHost));
    }
    if (e != hipSuccess) return fail(SID_PM_ERR_HIP, "debug_point: %s", hipGetErrorString(e));
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_debug_rsqrt(sid_pm_ctx *ctx, const double *x, double *y, int64_t n)
{
    if (!ctx || !x || !y || n < 0) return fail(SID_PM_ERR_ARG, "bad argument");
    Guard g(ctx->device);
    DevBuf<double> dx, dy;
    int rc;
    if ((rc = dx.reserve((size_t)n)) || (rc = dy.reserve((size_t)n))) return rc;
    hipError_t e = hipMemcpy(dx.p, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = (hipError_t)sid::launch_rsqrt(dx.p, dy.p, n, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(y, dy.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(SID_PM_ERR_HIP, "debug_rsqrt: %s", hipGetErrorString(e));
    return SID_PM_OK;
}


SID_EXPORT int sid_pm_debug_ncc_selftest(sid_pm_ctx *ctx, uint64_t seed, int64_t evaluations, int img_size, uint64_t counts[3])
{
    if (!ctx || !counts || evaluations <= 0 || img_size < 2 || img_size > 64) return fail(SID_PM_ERR_ARG, "bad argument");
    Guard g(ctx->device);
    DevBuf<unsigned long long> d;
    int rc;
    if ((rc = d.reserve(3))) return rc;
    const int per_thread = 256;
    const int blocks = (int)std::min<int64_t>((evaluations + 256 * per_thread - 1) / (256 * per_thread), 1 << 20);
    hipError_t e = hipMemsetAsync(d.p, 0, 3 * sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) e = (hipError_t)sid::launch_ncc_selftest(seed, blocks, per_thread, img_size, d.p, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    unsigned long long h[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(h, d.p, sizeof(h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(SID_PM_ERR_HIP, "debug_ncc_selftest: %s", hipGetErrorString(e));
    for (int k = 0; k < 3; ++k) counts[k] = h[k];
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_debug_hypot_selftest(sid_pm_ctx *ctx, uint64_t seed, int64_t evaluations, uint64_t counts[2])
{
    if (!ctx || !counts || evaluations <= 0) return fail(SID_PM_ERR_ARG, "bad argument");
    Guard g(ctx->device);
    DevBuf<unsigned long long> d;
    int rc;
    if ((rc = d.reserve(2))) return rc;
    const int per_thread = 256;
    const int blocks = (int)std::min<int64_t>((evaluations + 256 * per_thread - 1) / (256 * per_thread), 1 << 20);
    hipError_t e = hipMemsetAsync(d.p, 0, 2 * sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) e = (hipError_t)sid::launch_hypot_selftest(seed, blocks, per_thread, d.p, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    unsigned long long h[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpy(h, d.p, sizeof(h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(SID_PM_ERR_HIP, "debug_hypot_selftest: %s", hipGetErrorString(e));
    counts[0] = h[0]; counts[1] = h[1];
    return SID_PM_OK;
}

static int check_model_shape(int img_size, int n_angles)
{
    if (img_size < 2 || img_size > sid::kLargeMaxSide || n_angles < 1) return fail(SID_PM_ERR_UNSUPPORTED, "img_size / angle count not supported");
    return SID_PM_OK;
}

// the cost model of pm_plan.h (estimate_points) behind the argument checks of the ABI, with the switches of this call
static int estimate_checked(const Switches &sw, const double *border, int64_t n, int img_size, int n_angles, uint32_t flags, double *cost_ns, int32_t *per_cu_out)
{
    if (n < 0 || (n > 0 && (!border || (!cost_ns && !per_cu_out)))) return fail(SID_PM_ERR_ARG, "bad argument");
    if (int rc = check_model_shape(img_size, n_angles)) return rc;
    sid::plan::estimate_points(sw, border, n, img_size, n_angles, flags, cost_ns, per_cu_out);
    return SID_PM_OK;
}

SID_EXPORT int sid_pm_estimate_cost(const double *border, int64_t n, int img_size, int n_angles, uint32_t flags, double *cost_ns)
{
    if (n > 0 && !cost_ns) return fail(SID_PM_ERR_ARG, "bad argument");
    return estimate_checked(read_switches(), border, n, img_size, n_angles, flags, cost_ns, nullptr);
}

// Launch class of a point of that border (include/sid_pm.h): workgroups per CU in the low four bits - a launch runs 256 x that
// many points at a time, which is what the tail of a SHORT launch costs (dist.py) - plus the SID_PM_CLASS_* bits that tell the
// launches of equal residency apart (points of equal value share a launch).
SID_EXPORT int sid_pm_estimate_residency(const double *border, int64_t n, int img_size, int n_angles, uint32_t flags, int32_t *per_cu)
{
    if (n > 0 && !per_cu) return fail(SID_PM_ERR_ARG, "bad argument");
    return estimate_checked(read_switches(), border, n, img_size, n_angles, flags, nullptr, per_cu);
}

// the run-time model of pm_plan.h (estimate_run_time) behind the argument checks of the ABI, with the switches of this call
SID_EXPORT int sid_pm_estimate_run_time(const double *border, int64_t n, int img_size, int n_angles, uint32_t flags, double *time_ns)
{
    if (!time_ns || n < 0 || (n > 0 && !border)) return fail(SID_PM_ERR_ARG, "bad argument");
    *time_ns = 0.0;
    if (n == 0) return SID_PM_OK;
    if (int rc = check_model_shape(img_size, n_angles)) return rc;
    *time_ns = estimate_run_time(read_switches(), border, n, img_size, n_angles, flags);
    return SID_PM_OK;
}
