// am_rows.h -- what the row-per-lane stages share (records, select, split, subst, extract, coords, spans, postings, near, score, matrix, rules, hist and the chain
// selector of am_chain.h): the match record, the launch of one lane per row in workgroups of 256, and the owner search over ascending offsets.  A kernel with a
// tile geometry of its own (the gathers, the histograms, the prefix maximum, k_score, ...) keeps its own launch.
// AM_HD marks what runs on the host as well: the plain g++ programs under tests/native include this header, so nothing of HIP is needed without __HIPCC__.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AM_HD __host__ __device__ __forceinline__
#else
#define AM_HD inline
#endif

namespace am {
namespace dev {

// 16-byte match record in HBM.  Same layout as am_match in include/am.h.
struct alignas(16) Record { uint64_t end_pos; uint32_t haystack; uint32_t state; };

constexpr uint32_t kRowThreads = 256;                       // lanes of a workgroup: one row each
inline uint32_t row_blocks(uint64_t n) { return (uint32_t)((n + kRowThreads - 1) / kRowThreads); }

// the largest f in [lo, hi] with off[f] <= x (off ascending, off[lo] <= x): the owner of x among ascending offsets
template <class T, class I>
AM_HD I last_at_or_before(const T* off, I lo, I hi, uint64_t x)
{
    while (lo < hi) { const I mid = lo + ((hi - lo + 1) >> 1); if ((uint64_t)off[mid] <= x) lo = mid; else hi = mid - 1; }
    return lo;
}

#if defined(__HIPCC__)
__device__ __forceinline__ uint64_t global_row() { return (uint64_t)blockIdx.x * kRowThreads + threadIdx.x; }

// `kernel` over n rows, one lane each; no launch for no rows.  A site whose kernel also writes a trailing element passes n + 1.
template <class Kernel, class... Args>
hipError_t launch_rows(Kernel kernel, uint64_t n, hipStream_t st, const Args&... args)
{
    if (n == 0) return hipSuccess;
    if (n > 0x7FFFFFFFull * kRowThreads) return hipErrorInvalidValue;      // (beyond the grid's 2^31 - 1 workgroups)
    hipLaunchKernelGGL(kernel, dim3(row_blocks(n)), dim3(kRowThreads), 0, st, args...);
    return hipGetLastError();
}
#endif

}  // namespace dev
}  // namespace am
