// am_postings.h -- what the postings stage rests on (include/am.h "postings"), ONE definition for the device and the host: the plan of the least-significant-digit
// radix sort over the needle handles of a spans result (how many passes, which bits each pass sorts, the digit of a key in a pass), the index of a (digit, tile)
// cell in the table the exclusive sum turns into bases, and what the kernels of am_postings.hip are launched with.
// THE PLAN.  Keys are needle handles below n_needles, so only B = bitlen(n_needles - 1) bits differ.  passes = ceil(B / 8) (0 for n_needles <= 1, 4 at the most), and
// the B bits are divided EVENLY among them, the low passes taking the remainder: 17 bits are 6 + 6 + 5, not 8 + 8 + 1 -- a pass's table has 2^bits rows per tile, so
// even digits keep every table small.  Pass p sorts bits [shift[p], shift[p] + bits[p]).
// THE TABLE of a pass is digit-major: cell (d, t) at d * n_tiles + t holds the keys of tile t whose digit is d.  Its exclusive sum in that order is, per cell, the
// number of keys with a smaller digit anywhere plus the keys with the same digit in an earlier tile: where the cell's first key goes in a stable sort.
// Plain C++: tests/native/postings_sort_main.cpp compiles all of it with g++ and holds the pass plan, run on the CPU, to std::stable_sort.
#pragma once
#include "am_rows.h"

namespace am {
namespace dev {

constexpr uint32_t kPostMaxPasses = 4;
constexpr uint32_t kPostMaxDigitBits = 8;
constexpr uint32_t kPostThreads = 256;                      // lanes per workgroup of am_postings.hip: four wavefronts
constexpr uint32_t kPostWaveSpans = 2048;                   // consecutive spans a wavefront owns: 32 rounds of 64
constexpr uint32_t kPostTileSpans = kPostWaveSpans * (kPostThreads / 64);      // spans per workgroup tile
constexpr uint64_t kPostMaxSpans = 0xFFFFFFFFull;           // the sort carries 32-bit row indices: n must stay below

struct PostPlan { uint32_t passes; uint32_t bits[kPostMaxPasses]; uint32_t shift[kPostMaxPasses]; };

// bits that can differ among keys below n_needles
AM_HD uint32_t post_key_bits(uint64_t n_needles)
{
    uint32_t b = 0;
    if (n_needles > 1) for (uint64_t x = n_needles - 1; x != 0; x >>= 1) b++;
    return b > 32 ? 32 : b;
}

AM_HD uint32_t post_passes(uint64_t n_needles) { return (post_key_bits(n_needles) + kPostMaxDigitBits - 1) / kPostMaxDigitBits; }

AM_HD PostPlan post_plan(uint64_t n_needles)
{
    PostPlan p{};
    const uint32_t b = post_key_bits(n_needles);
    p.passes = post_passes(n_needles);
    uint32_t at = 0;
    for (uint32_t k = 0; k < p.passes; k++) {
        p.bits[k] = b / p.passes + (k < b % p.passes ? 1u : 0u);
        p.shift[k] = at;
        at += p.bits[k];
    }
    return p;
}

AM_HD uint32_t post_digit(const PostPlan& p, uint32_t key, uint32_t pass) { return (key >> p.shift[pass]) & ((1u << p.bits[pass]) - 1u); }
AM_HD uint32_t post_digits(const PostPlan& p, uint32_t pass) { return 1u << p.bits[pass]; }
AM_HD uint64_t post_tiles(uint64_t n) { return (n + kPostTileSpans - 1) / kPostTileSpans; }
AM_HD uint64_t post_cell(uint32_t digit, uint64_t tile, uint64_t n_tiles) { return (uint64_t)digit * n_tiles + tile; }

// first k in [0, n) with a[k * stride] >= x (n: none); a ascends.  The search of k_post_offsets (stride 1 over the sorted keys) and of k_post_row_offsets (stride 6
// over the haystack field of 24-byte rows)
AM_HD uint64_t post_lower_bound(const uint32_t* a, uint64_t n, uint64_t stride, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)a[mid * stride] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct Span;
// the launchers of am_postings.hip (the host side: am_postings.cpp).  Every array is in HBM.
//   launch_post_keys         keys[i] = spans[i].needle, idx[i] = i, for i < n
//   launch_post_hist         one pass: counts[post_cell(d, t)] = keys of tile t with digit d, every cell of the pass's table written
//   launch_post_scatter      one pass: with base = the exclusive sum of counts, keys_out / idx_out = keys_in / idx_in stably ordered by the pass's digit
//   launch_post_gather       data[k] = spans[idx[k]], source[k] = idx[k]
//   launch_post_offsets      offsets[v] = first k with keys[k] >= v, for v <= n_needles (keys sorted)
//   launch_post_df           doc_freq[v] += rows k of needle v = keys[k] that open a run of one haystack (doc_freq cleared by the caller)
//   launch_post_row_offsets  out_off[h] = first k in row[0, n_row) with row[k].haystack >= h, for h <= n_hay
#if defined(__HIPCC__)
hipError_t launch_post_keys(const Span* spans, uint64_t n, uint32_t* keys, uint32_t* idx, hipStream_t st);
hipError_t launch_post_hist(const PostPlan& plan, uint32_t pass, const uint32_t* keys, uint64_t n, uint32_t* counts, hipStream_t st);
hipError_t launch_post_scatter(const PostPlan& plan, uint32_t pass, const uint32_t* keys_in, const uint32_t* idx_in, uint64_t n, const uint64_t* base, uint32_t* keys_out,
                               uint32_t* idx_out, hipStream_t st);
hipError_t launch_post_gather(const Span* spans, const uint32_t* idx, uint64_t n, Span* data, uint64_t* source, hipStream_t st);
hipError_t launch_post_offsets(const uint32_t* keys, uint64_t n, uint64_t n_needles, uint64_t* offsets, hipStream_t st);
hipError_t launch_post_df(const Span* data, const uint32_t* keys, uint64_t n, uint64_t n_needles, uint64_t* doc_freq, hipStream_t st);
hipError_t launch_post_row_offsets(const Span* row, uint64_t n_row, uint64_t n_hay, uint64_t* out_off, hipStream_t st);
#endif

}  // namespace dev
}  // namespace am
