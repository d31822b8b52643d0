// am_near.h -- what the proximity stage rests on (include/am.h "proximity"), ONE definition for the device and the host: the pick of one (anchor, p, n, query), the
// bit arithmetic that finds p and n in the group bitmaps, the running maximum behind the word links, and what the kernels of am_near.hip are launched with.
// A GROUP BITMAP is one bit per span of the data array, bit i % 64 of word i / 64 set iff span i is in the group.  The nearest member below span i is the highest set
// bit below bit i of i's own word, or -- none there -- the highest bit of the last non-zero word before it, which prev_nz names per word; the nearest member above
// is the mirror image through next_nz.  So a lane finds both partners with two word loads and two link loads at the most, whatever the text looks like: no lane
// walks spans.  Whether the span found lies in the anchor's haystack is near_pick's to decide (the rows ascend by haystack, so the nearest member overall lying in
// another haystack means there is none in this one).  Plain C++: tests/native/near_pick_main.cpp compiles all of it with g++ and holds it to a brute-force loop under
// a sanitizer.
#pragma once
#include "am_rows.h"

namespace am {
namespace dev {

constexpr uint32_t kNearMaxGroups = 32;                     // AM_NEAR_MAX_GROUPS
constexpr uint32_t kNearMaxQueries = 64;                    // AM_NEAR_MAX_QUERIES
constexpr uint32_t kNearOrdered = 1u;                       // AM_NEAR_ORDERED
constexpr uint64_t kNearNone = ~0ull;                       // no span
constexpr uint32_t kNearNoWord = ~0u;                       // no word (the links are 32-bit: a data array has fewer than 2^32 - 1 words of 64 spans)
constexpr uint32_t kNearLdsNeedles = 8192;                  // masks k_near_bits stages in LDS (32 KiB); a larger table is read from HBM

struct alignas(8) NearQuery { uint32_t group_a, group_b, flags, reserved; uint64_t max_gap; };      // = am_near_query in include/am.h
struct alignas(8) NearPair { uint64_t a, b, gap; uint32_t haystack, query; };                       // = am_near_pair in include/am.h
struct NearSide { bool has; uint64_t idx, start, len; uint32_t haystack; };                         // a candidate: span idx with its fields, or nothing
struct NearPicked { bool hit; uint64_t b, gap; };

// The partner of an anchor among its two candidates: p lies before it, n behind it; a candidate of another haystack is none.  Under kNearOrdered only n counts.  The
// rows do not overlap, so both gaps are differences of unsigned numbers that do not wrap.  The smaller gap wins, a tie goes to p; a pair iff the gap <= max_gap.
AM_HD NearPicked near_pick(uint64_t a_start, uint64_t a_len, uint32_t a_haystack, const NearSide& p, const NearSide& n, uint32_t flags, uint64_t max_gap)
{
    const bool has_p = (flags & kNearOrdered) == 0 && p.has && p.haystack == a_haystack;
    const bool has_n = n.has && n.haystack == a_haystack;
    const uint64_t gap_p = has_p ? a_start - (p.start + p.len) : 0;
    const uint64_t gap_n = has_n ? n.start - (a_start + a_len) : 0;
    if (!has_p && !has_n) return NearPicked{false, 0, 0};
    const bool take_p = has_p && (!has_n || gap_p <= gap_n);
    const uint64_t gap = take_p ? gap_p : gap_n;
    return NearPicked{gap <= max_gap, take_p ? p.idx : n.idx, gap};
}

// the highest set bit of `word` below bit `bit` / the lowest above it (bit < 64); 64: none
AM_HD uint32_t near_bit_below(uint64_t word, uint32_t bit)
{
    const uint64_t below = word & ((1ull << bit) - 1ull);
    return below ? 63u - (uint32_t)__builtin_clzll(below) : 64u;
}
AM_HD uint32_t near_bit_above(uint64_t word, uint32_t bit)
{
    const uint64_t above = bit >= 63u ? 0ull : word & ~((2ull << bit) - 1ull);
    return above ? (uint32_t)__builtin_ctzll(above) : 64u;
}

// the nearest member of a group below / above span i: `row` = the group's bitmap (n_words words), prev_nz / next_nz = its links; kNearNone: none
AM_HD uint64_t near_prev(const uint64_t* row, const uint32_t* prev_nz, uint64_t i)
{
    const uint64_t w = i >> 6;
    const uint32_t b = near_bit_below(row[w], (uint32_t)(i & 63u));
    if (b < 64u) return (w << 6) | b;
    const uint32_t pw = prev_nz[w];
    if (pw == kNearNoWord) return kNearNone;
    return ((uint64_t)pw << 6) | (63u - (uint32_t)__builtin_clzll(row[pw] | 1ull));      // (| 1: a link names a non-zero word; a zero one would be a bug, not a crash)
}
AM_HD uint64_t near_next(const uint64_t* row, const uint32_t* next_nz, uint64_t i)
{
    const uint64_t w = i >> 6;
    const uint32_t b = near_bit_above(row[w], (uint32_t)(i & 63u));
    if (b < 64u) return (w << 6) | b;
    const uint32_t nw = next_nz[w];
    if (nw == kNearNoWord) return kNearNone;
    return ((uint64_t)nw << 6) | (uint32_t)__builtin_ctzll(row[nw] | (1ull << 63));
}

// The links are running maxima.  Walking the words in one direction, step k = 0, 1, ... (forwards: word k; backwards: word n_words - 1 - k), a non-zero word has
// the value k + 1 and a zero word 0; E_k = the maximum of the values of the steps before k (0: none).  Forwards E_k - 1 is the last non-zero word before word k,
// backwards n_words - E_k is the first non-zero word behind it.  k_near_words takes the maxima in sweeps with a carry; a sequential caller keeps one variable.
AM_HD uint32_t near_link_value(uint64_t word, uint32_t step) { return word ? step + 1u : 0u; }
AM_HD uint32_t near_link_word(uint32_t excl_max, bool backwards, uint32_t n_words) { return excl_max == 0u ? kNearNoWord : (backwards ? n_words - excl_max : excl_max - 1u); }
AM_HD uint32_t near_link_index(uint32_t step, bool backwards, uint32_t n_words) { return backwards ? n_words - 1u - step : step; }

// the compiled form of a query set: the groups any query names get a bitmap row each, in ascending order of the group
struct NearPlan {
    uint32_t n_queries, n_rows;
    uint32_t used;                                          // bit g: some query names group g
    uint8_t row_of[kNearMaxGroups];                         // group -> its row (groups no query names: 0, never looked at)
};
inline NearPlan near_plan(const NearQuery* q, uint32_t n_queries)
{
    NearPlan p{};
    p.n_queries = n_queries;
    for (uint32_t i = 0; i < n_queries; i++) p.used |= (1u << q[i].group_a) | (1u << q[i].group_b);
    for (uint32_t g = 0; g < kNearMaxGroups; g++)
        if (p.used >> g & 1u) p.row_of[g] = (uint8_t)p.n_rows++;
    return p;
}

// a query as the kernels read it: group_a as a bit of the anchor's mask, group_b as the bitmap row it got
struct alignas(8) NearQueryDev { uint32_t bit_a, row_b, flags, reserved; uint64_t max_gap; };

struct Span;                                                // am_device.h
// what the kernels read and write.  n_span spans in n_words = ceil(n_span / 64) words; rows: bits[n_rows][n_words], prev_nz / next_nz[n_rows][n_words]
struct NearIn {
    const Span* spans; uint64_t n_span; uint32_t n_words;
    const uint64_t* span_off; uint64_t n_hay;               // the spans' row offsets, n_hay + 1
    const uint32_t* group_mask; uint32_t n_needles;
    const NearQueryDev* dq;                                 // plan.n_queries, in HBM
    NearPlan plan;
    uint64_t* bits; uint32_t* prev_nz; uint32_t* next_nz;
    uint64_t* hit_mask; uint32_t* hit_count;                // per span: the queries that hit (n_span), their number (n_span + 1, the last one 0)
    const uint64_t* pos;                                    // the exclusive sum of hit_count (n_span + 1)
    uint64_t* fired; uint64_t hay_words;                    // uint64[n_queries][hay_words], cleared by the caller
    uint64_t* counts;                                       // uint64[n_queries], cleared by the caller
    NearPair* pairs; uint64_t n_pairs;
    uint64_t* out_off;                                      // n_hay + 1
};

}  // namespace dev
}  // namespace am
