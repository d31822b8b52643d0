// am_chain.h -- greedy selection along chains: from an ascending list of intervals keep an element iff it is the first of its row or starts at or after the end of
// the last element kept in its row.  The Splitter's separators (am_split.hip) and the leftmost-longest spans (am_spans.hip) are both this fold.
//
// The fold is sequential as written.  What makes it parallel:
//   * an element is a HEAD when nothing before it in its row ends beyond its start.  A head is always kept, and what happens before a head has no influence on what
//     happens from it on: the CHAINS between heads are independent.  Which elements are heads is the stage's own business (the Splitter's records are sorted by end,
//     so a comparison with the predecessor decides; the spans' candidates need a prefix maximum of the ends).  For "\n" or "," every chain has length 1.
//   * inside a chain, next[i] = the first element that starts at or after the end of i (chain_next), and the kept elements are exactly the path head, next[head],
//     next[next[head]], ...  A short chain is walked by its head's lane (chain_walk, at most `limit` elements looked at).  A chain beyond the limit -- "aa" over a run
//     of a's is ONE chain through the whole text -- is finished by pointer doubling over all elements: per round every kept element marks J[i] and J becomes J o J
//     (chain_double), so a path of k elements is marked after log2(k) rounds; the host stops when a round marks nothing.  Every mark is an element of the true path
//     (J[i] is a power of `next` applied to a kept element), so marks from partly walked chains and marks seen within the same round do no harm.
// A CHAIN VIEW answers start(i), end(i) and same_row(i, j) for the n elements; the per-element steps below are host and device code (tests/native/chain_select_main.cpp
// runs them on the CPU), the kernels around them are am_chain.hip's, and select_chains (am_fold.h) is the host sequence.  All indices are 64-bit.
#pragma once
#include "am_rows.h"

#if defined(__HIPCC__)
#include "am_bounds.h"
#elif !defined(AM_BOUNDS)
#define AM_BOUNDS(cond) ((void)0)
#endif

namespace am {
namespace dev {

// the Splitter's records with their separators' starts: positions are relative to the haystack, so the row is the haystack
struct SplitChain {
    const Record* recs; const uint64_t* starts; uint64_t n;
    AM_HD uint64_t start(uint64_t i) const { return starts[i]; }
    AM_HD uint64_t end(uint64_t i) const { return recs[i].end_pos; }
    AM_HD bool same_row(uint64_t i, uint64_t j) const { return recs[i].haystack == recs[j].haystack; }
};

// the spans' candidates in global byte positions (best = len << 32 | ~needle): one row, a later haystack's candidates start at or after every end of an earlier one
struct SpansChain {
    const uint64_t* cand_g; const uint64_t* best; uint64_t n;
    AM_HD uint64_t start(uint64_t i) const { return cand_g[i]; }
    AM_HD uint64_t end(uint64_t i) const { return cand_g[i] + (best[i] >> 32); }
    AM_HD bool same_row(uint64_t, uint64_t) const { return true; }
};

// head i walks its chain and keeps what the fold keeps; true: the chain needs more than `limit` looks and is left to the doubling rounds
template <class View>
AM_HD bool chain_walk(const View& v, const uint8_t* head, uint32_t* kept, uint32_t limit, uint64_t i)
{
    uint64_t end = v.end(i);
    uint32_t looks = 0;
    for (uint64_t j = i + 1; j < v.n && !head[j]; j++) {
        if (++looks > limit) return true;
        if (v.start(j) >= end) { kept[j] = 1; end = v.end(j); }        // (only this lane writes inside its chain)
    }
    return false;
}

// next[i]: the first element of i's chain that starts at or after the end of i; i itself when there is none or when it is a head (the next chain's own).  (row,
// start) is sorted, so a galloping search from i + 1 finds it.  same_row belongs to the predicate: j > i lies in i's row or a later one, and a later row's starts
// begin again below end(i).
template <class View>
AM_HD uint64_t chain_next(const View& v, const uint8_t* head, uint64_t i)
{
    const uint64_t n = v.n, end = v.end(i);
    auto before = [&](uint64_t j) { return v.same_row(i, j) && v.start(j) < end; };
    uint64_t lo = i + 1, step = 1, probe = i + 1;
    while (probe < n && before(probe)) { lo = probe + 1; step <<= 1; probe = i + step; }
    uint64_t hi = probe < n ? probe : n;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (before(mid)) lo = mid + 1; else hi = mid; }
    AM_BOUNDS(lo > i && lo <= n);
    return (lo >= n || head[lo]) ? i : lo;
}

// element i's part of one round of pointer doubling: a kept element marks where it jumps to, the jumps double; true: it marked one
AM_HD bool chain_double(const uint64_t* jump_in, uint64_t* jump_out, uint64_t n, uint32_t* kept, uint64_t i)
{
    uint64_t j = jump_in[i];
    AM_BOUNDS(j < n);
    if (j >= n) j = i;
    jump_out[i] = jump_in[j];
    if (!kept[i] || kept[j]) return false;
    kept[j] = 1;
    return true;
}

#if defined(__HIPCC__)
// one lane per element (am_chain.hip; View = SplitChain or SpansChain).  *long_chains / *marked, cleared by the caller, != 0 when a chain needed more than `limit`
// looks / when the round marked an element
template <class View> hipError_t launch_chain_walk(const View& v, const uint8_t* head, uint32_t* kept, uint32_t limit, uint32_t* long_chains, hipStream_t st);
template <class View> hipError_t launch_chain_next(const View& v, const uint8_t* head, uint64_t* jump, hipStream_t st);
hipError_t launch_chain_double(const uint64_t* jump_in, uint64_t* jump_out, uint64_t n, uint32_t* kept, uint32_t* marked, hipStream_t st);
#endif

}  // namespace dev
}  // namespace am
