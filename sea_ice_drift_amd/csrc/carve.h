// carve.h - the layout of a staging block, described once (host code; no HIP, so tests/cpp/carver_check.cpp compiles it alone).
// A layout is a function of a Carver& that take()s its regions in order.  It runs twice: on a Carver without a block, which only
// measures (off = the bytes the block needs), and on one with the block, which hands out the pointers.  The size that is
// reserved and the pointers that are used cannot disagree: they come from the same lines.
#pragma once
#include <stddef.h>

namespace {

inline size_t up(size_t bytes) { return (bytes + 255) / 256 * 256; }      // regions start 256 bytes apart at the least

struct Carver {
    unsigned char *base;
    size_t off = 0;
    explicit Carver(unsigned char *block = nullptr) : base(block) {}
    // n elements of T.  An absent region (n == 0 or !present) is nullptr and takes no room.
    template <typename T> T *take(size_t n, bool present = true)
    {
        if (!present || n == 0) return nullptr;
        T *r = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += up(n * sizeof(T));
        return r;
    }
};

}  // namespace
