// ft_plan.h - the launch plan of the Hamming matcher of include/sid_ft.h (csrc/ft_match.hip): which of the two forms a size
// takes, how the train set is cut into chunks, where the regions of the workspace lie, and the sizes the entry points accept.
// Plain C++ (no HIP), so that tests/cpp/ft_plan_check.cpp compiles it alone: what the kernels index with is what the check sweeps.
#ifndef SID_FT_PLAN_H
#define SID_FT_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#include "carve.h"

namespace sid_ft {

constexpr int kThreads = 256;
constexpr uint32_t kNone = 0xffffffffu;
constexpr int64_t kMaxTrain = (int64_t)1 << 22;             // index bits of the key
constexpr int64_t kMaxQueries = 0x7fffffff / 4;             // (the kernels index part[] and the outputs from 32-bit query numbers)
constexpr int kQB = 256;            // queries per workgroup
constexpr int kTB = 256;            // train descriptors per LDS batch

// the sizes sid_ft_knn2_device accepts
inline bool sizes_supported(int64_t n1, int64_t n2) { return !(n1 > kMaxQueries || n2 >= kMaxTrain); }

// chunk size: enough blocks to fill the chip (>= ~2048 blocks), at least 256 train descriptors per chunk
inline void plan(int64_t n1, int64_t n2, int &chunk, int &nchunks)
{
    const int64_t qblocks = (n1 + kThreads - 1) / kThreads;
    int64_t want = std::max<int64_t>(1, (2048 + qblocks - 1) / std::max<int64_t>(qblocks, 1));
    int64_t c = std::max<int64_t>(256, (n2 + want - 1) / want);
    c = std::min<int64_t>(c, std::max<int64_t>(n2, 1));
    chunk = (int)c;
    nchunks = (int)((n2 + c - 1) / c);
    if (nchunks < 1) nchunks = 1;
}

// MFMA form: queries and train descriptors padded to 256; chunks of whole LDS batches, >= ~512 workgroups (two per CU)
struct MfmaPlan { int64_t n1pad, n2pad; int chunk, nchunks; size_t off_e1, off_e2, off_c, total; };
constexpr int64_t kMfmaMinPairs = (int64_t)1 << 24;                    // below this the one-thread-per-query kernel is as fast
inline bool use_mfma(int64_t n1, int64_t n2) { return n1 * n2 >= kMfmaMinPairs && n2 >= 1024 && getenv("SID_FT_NO_MFMA") == nullptr; }
inline MfmaPlan plan_mfma(int64_t n1, int64_t n2)
{
    MfmaPlan P;
    P.n1pad = (std::max<int64_t>(n1, 1) + kQB - 1) / kQB * kQB; P.n2pad = (std::max<int64_t>(n2, 1) + kTB - 1) / kTB * kTB;   // (empty sets: sized, never run)
    const int64_t qblocks = P.n1pad / kQB, batches = P.n2pad / kTB;
    int64_t want = std::max<int64_t>(1, (512 + qblocks - 1) / qblocks);
    want = std::min<int64_t>(want, batches);
    const int64_t per = (batches + want - 1) / want;
    P.chunk = (int)(per * kTB); P.nchunks = (int)((batches + per - 1) / per);
    P.off_e1 = up(sizeof(uint32_t) * 2 * (size_t)std::max<int64_t>(n1, 1) * P.nchunks);
    P.off_e2 = P.off_e1 + (size_t)P.n1pad * 256;
    P.off_c = P.off_e2 + (size_t)P.n2pad * 256;
    P.total = P.off_c + up(sizeof(uint32_t) * (size_t)P.n2pad);
    return P;
}

// sid_ft_workspace_bytes: room for either form (which one runs depends on SID_FT_NO_MFMA too, not on the sizes alone)
inline int64_t workspace_bytes(int64_t n1, int64_t n2)
{
    if (n1 < 0 || n2 < 0) return 0;
    int chunk, nchunks;
    plan(n1, n2, chunk, nchunks);
    const int64_t valu = (int64_t)sizeof(uint32_t) * 2 * std::max<int64_t>(n1, 1) * nchunks;
    return std::max<int64_t>(valu, (int64_t)plan_mfma(n1, n2).total);      // (either kernel may run: SID_FT_NO_MFMA, size)
}

}  // namespace sid_ft

#endif
