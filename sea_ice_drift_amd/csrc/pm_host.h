// pm_host.h - host pieces of the pattern-matching core that own or lay out device memory, without a HIP call in them, so that
// tests/cpp/lifetime_check.cpp runs them with g++ and a sanitizer alone: the scoped device buffer (pm_capi.hip: DevBuf) and the
// layout of the resident points' arena (sid_pm_set_points).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "carve.h"

namespace {

// n elements of T from Alloc, freed when the buffer leaves its scope.  Move-only: one owner per allocation.
// Alloc::alloc(void **, bytes) returns 0 or an error code (and says why in its own way); Alloc::free(void *).
template <typename T, class Alloc>
struct ScopedBuf {
    T *p = nullptr;
    size_t cap = 0;
    ScopedBuf() = default;
    ScopedBuf(const ScopedBuf &) = delete;
    ScopedBuf &operator=(const ScopedBuf &) = delete;
    ScopedBuf(ScopedBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ScopedBuf &operator=(ScopedBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~ScopedBuf() { release(); }
    // grow-only; what it held is gone (not copied) once it grows
    int reserve(size_t n)
    {
        if (n <= cap) return 0;
        release();
        void *q = nullptr;
        if (int rc = Alloc::alloc(&q, std::max<size_t>(n, 1) * sizeof(T))) return rc;
        p = static_cast<T *>(q); cap = n;
        return 0;
    }
    void release() { if (p) Alloc::free(p); p = nullptr; cap = 0; }   // (the places that free early on purpose)
};

// The arena of the resident points: one block, one upload per set_points.  [5n doubles: c1, r1, c2fg, r2fg, border | K angles |
// 4K rotation terms | launch order (int32 n) | sampling table + 4 entries of slack | the table sorted per angle (SID_PM_SAMP2=1)]
struct PointArena {
    double *vec, *angles, *rot;
    int32_t *order;
    uint16_t *samp;
    uint32_t *samp2;
};
inline PointArena point_arena(Carver &c, size_t n, size_t K, size_t n_samp, size_t n_samp2)
{
    PointArena a;
    a.vec = c.take<double>(5 * n);
    a.angles = c.take<double>(K);
    a.rot = c.take<double>(4 * K);
    a.order = c.take<int32_t>(n);
    a.samp = c.take<uint16_t>(n_samp + 4);
    a.samp2 = c.take<uint32_t>(n_samp2);
    return a;
}

}  // namespace
