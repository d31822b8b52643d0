// am_select.hip -- select on the device (include/am.h "select"): the haystacks of a batch that a predicate keeps, as ascending indices and as a batch of their own.
//
// The predicate arrives as one byte per haystack in HBM: the flags of the containsAny / containsAll scans, or of k_hay_flags_spans (am_records.hip) over the sorted
// records of a scan -- haystack h is flagged when row h of AM_SPANS_ALL is not empty.
//
// The compaction works on RUNS.  A batch stores its haystacks back to back, so a maximal sequence of consecutive kept haystacks is ONE contiguous piece of the source
// text.  k_select_plan turns the flags into keep / run_head / the kept lengths, three exclusive sums (am_scan.hip) give every kept haystack its rank and its new offset
// and every run its rank, and k_select_emit writes the indices, the new offsets and per run (source position, destination position).  The bytes then move with
// launch_split_gather (am_split.hip) with the runs as its fragments: keeping everything is one run and a straight copy, keeping alternate haystacks gives `kept` runs.
// All positions and totals are 64-bit; the only 32-bit quantities are haystack indices (n_hay < 2^32 - 1 for every batch).  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include "am_bounds.h"
#include "am_device.h"

AM_BOUNDS_TU("am_select.hip")

namespace am {
namespace dev {

namespace {

// one lane per haystack (+ one for the trailing zero of the scans' inputs)
__global__ void __launch_bounds__(kRowThreads) k_select_plan(const uint8_t* __restrict__ flags, uint32_t constant, uint32_t invert, const uint64_t* __restrict__ src_offsets,
                                                             uint64_t n, uint64_t src_total, uint32_t* __restrict__ keep, uint32_t* __restrict__ run_head,
                                                             uint64_t* __restrict__ klen)
{
    const uint64_t i = global_row();
    if (i > n) return;
    if (i == n) { keep[i] = 0; run_head[i] = 0; klen[i] = 0; return; }
    const bool inv = invert != 0;
    const bool k = ((flags ? flags[i] : constant) != 0) != inv;
    const bool before = i > 0 && ((flags ? flags[i - 1] : constant) != 0) != inv;
    const uint64_t o0 = src_offsets[i], o1 = src_offsets[i + 1];
    AM_BOUNDS(o0 <= o1 && o1 <= src_total);
    const uint64_t len = o0 <= o1 && o1 <= src_total ? o1 - o0 : 0;
    keep[i] = k ? 1u : 0u;
    run_head[i] = k && !before ? 1u : 0u;
    klen[i] = k ? len : 0;
}

// one lane per haystack (+ one for the closing entries)
__global__ void __launch_bounds__(kRowThreads) k_select_emit(const uint32_t* __restrict__ keep, const uint32_t* __restrict__ run_head, const uint64_t* __restrict__ rank,
                                                             const uint64_t* __restrict__ run_rank, const uint64_t* __restrict__ koff,
                                                             const uint64_t* __restrict__ src_offsets, uint64_t n, uint64_t n_kept, uint64_t n_runs,
                                                             uint32_t* __restrict__ indices, uint64_t* __restrict__ new_off, uint64_t* __restrict__ run_src,
                                                             uint64_t* __restrict__ run_dst)
{
    const uint64_t i = global_row();
    if (i > n) return;
    if (i == n) {
        AM_BOUNDS(rank[n] == n_kept && run_rank[n] == n_runs);
        new_off[n_kept] = koff[n];
        run_dst[n_runs] = koff[n];
        run_src[n_runs] = 0;
        return;
    }
    if (!keep[i]) return;
    const uint64_t r = rank[i];
    AM_BOUNDS(r < n_kept);
    if (r >= n_kept) return;
    indices[r] = (uint32_t)i;
    new_off[r] = koff[i];
    if (!run_head[i]) return;
    const uint64_t q = run_rank[i];
    AM_BOUNDS(q < n_runs);
    if (q >= n_runs) return;
    run_src[q] = src_offsets[i];
    run_dst[q] = koff[i];
}

}  // namespace

hipError_t launch_select_plan(const uint8_t* flags, uint32_t constant, uint32_t invert, const uint64_t* src_offsets, uint64_t n, uint64_t src_total, uint32_t* keep,
                              uint32_t* run_head, uint64_t* klen, hipStream_t st)
{
    return launch_rows(k_select_plan, n + 1, st, flags, constant, invert, src_offsets, n, src_total, keep, run_head, klen);
}

hipError_t launch_select_emit(const uint32_t* keep, const uint32_t* run_head, const uint64_t* rank, const uint64_t* run_rank, const uint64_t* koff, const uint64_t* src_offsets,
                              uint64_t n, uint64_t n_kept, uint64_t n_runs, uint32_t* indices, uint64_t* new_off, uint64_t* run_src, uint64_t* run_dst, hipStream_t st)
{
    return launch_rows(k_select_emit, n + 1, st, keep, run_head, rank, run_rank, koff, src_offsets, n, n_kept, n_runs, indices, new_off, run_src, run_dst);
}

}  // namespace dev
}  // namespace am
