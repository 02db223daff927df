// host_util.h - the host scaffold of the units beside the pattern-matching core (ft_match, stage, orb, first_guess, defor, prep,
// landmask, drift_grid, warp, resize, local_corr, track, ft_guided).  Host code only.  Everything lives in an anonymous namespace: every unit
// keeps its OWN thread-local error text (sid_grid_last_error never shows sid_warp's message) and its own pools.
// pm_capi.hip / pm_large.hip keep their own error handling, which is tied to the handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <mutex>

#include "../../include/sid_pm.h"
#include "carve.h"

#define SID_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kMaxDevices = 16;                                        // slots of a DevicePool

thread_local char g_err[256] = "";
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return code;
}

#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(SID_PM_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)

inline int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SID_PM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return SID_PM_OK;
}

// Launches go to the device that holds `p` (the null stream belongs to the CURRENT device); the previous device comes back.
struct DeviceOf {
    int prev = -1;
    explicit DeviceOf(const void *p)
    {
        hipPointerAttribute_t at;
        int cur = 0; (void)hipGetDevice(&cur);
        if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice && at.device != cur) {
            prev = cur; (void)hipSetDevice(at.device);
        } else (void)hipGetLastError();                      // (a pointer HIP does not know leaves an error behind)
    }
    ~DeviceOf() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Select device `device` for a scope.  enter() is false for an index that is not a visible device with a pool slot (nothing
// is selected; `visible` says how many there are) and the caller phrases the failure: most units answer SID_PM_ERR_NODEVICE.
struct DeviceScope {
    int prev = -1, visible = 0;
    bool enter(int device)
    {
        if (hipGetDeviceCount(&visible) != hipSuccess) visible = 0;
        if (device < 0 || device >= visible || device >= kMaxDevices) return false;
        (void)hipGetDevice(&prev); (void)hipSetDevice(device);
        return true;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Grow-only device block: bytes + bytes / 4 when it has to grow, so that a slowly growing series does not allocate per call
inline int grow(unsigned char *&p, size_t &cap, size_t bytes)
{
    if (cap >= bytes) return SID_PM_OK;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 4;
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), want);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? SID_PM_ERR_NOMEM : SID_PM_ERR_HIP, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
    cap = want;
    return SID_PM_OK;
}

// Per device: the staging block of the host-buffer entry points (no hipMalloc / hipFree per call once warm) and the unit's own
// state `Extra` (cached(): holds something release must free; free(): frees it, on its device).  The caller holds
// mutex(device) around reserve / carve and for as long as it uses the block.  PerDevice: one mutex per device, so that calls on
// different devices run side by side (the matcher under devices=); else one for the unit.
struct NoExtra { bool cached() const { return false; } void free() {} };
template <class Extra = NoExtra, bool PerDevice = false>
struct DevicePool {
    struct Slot : Extra { unsigned char *blk = nullptr; size_t cap = 0; };
    Slot slot[kMaxDevices];
    std::mutex mu[PerDevice ? kMaxDevices : 1];
    std::mutex &mutex(int device) { return mu[PerDevice ? device : 0]; }
    int reserve(int device, size_t bytes) { return grow(slot[device].blk, slot[device].cap, bytes); }
    // One layout, run twice: measured, reserved, carved (carve.h)
    template <class Layout> int carve(int device, Layout layout)
    {
        Carver measure;
        layout(measure);
        if (int rc = reserve(device, measure.off)) return rc;
        Carver c(slot[device].blk);
        layout(c);
        return SID_PM_OK;
    }
    // device < 0: every device.  No HIP call when nothing is cached (a machine without a GPU may call it).
    int release(int device)
    {
        int prev = -1;
        for (int i = 0; i < kMaxDevices; ++i) {
            if (device >= 0 && i != device) continue;
            std::lock_guard<std::mutex> lock(mutex(i));
            Slot &s = slot[i];
            if (!s.blk && !s.cached()) continue;
            if (prev < 0) (void)hipGetDevice(&prev);
            (void)hipSetDevice(i);
            if (s.blk) (void)hipFree(s.blk);
            s.free();
            s = Slot();
        }
        if (prev >= 0) (void)hipSetDevice(prev);
        return SID_PM_OK;
    }
};

// The frame of a host-buffer entry point: the device selected, the pool's mutex held, and on every way out but done() - a
// failed copy or launch - the null stream drained BEFORE the mutex is given up, so that nothing of a failed call is still in
// flight in a block the next call carves differently.  A call that succeeded has synchronised itself and says done().
struct Staging {
    DeviceScope dev;
    std::unique_lock<std::mutex> lock;
    bool clean = false;
    template <class Pool> bool enter(Pool &pool, int device)
    {
        if (!dev.enter(device)) return false;
        lock = std::unique_lock<std::mutex>(pool.mutex(device));
        return true;
    }
    void done() { clean = true; }
    ~Staging() { if (lock.owns_lock() && !clean) (void)hipStreamSynchronize(nullptr); }   // (then the members: unlock, device back)
};

}  // namespace
