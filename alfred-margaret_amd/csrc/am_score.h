// am_score.h -- the two functions the top-k of a score column rests on (include/am.h "scores"), ONE definition for the device and the host, and what k_score is
// launched with.  score_key maps an int64 score to a uint64 whose unsigned order is the order the caller asked for: the LARGEST key is the best score in either
// direction.  The k best keys are found by an 8-bit radix select from the top byte down: a pass counts, among the keys that share the digits chosen so far, how many
// carry each value of the next digit (hist[256]); topk_pick walks the bins from 255 down and names the digit of the k-th best key and how many of that digit's keys
// are still wanted.  After eight passes the digits are the k-th best key T and what remains of k is the tie quota q: the keys above T are all taken and the first q of
// the keys equal to T, in ascending haystack order.  Plain C++: tests/native/score_topk_main.cpp compiles both with g++ and holds the eight passes to std::sort under a
// sanitizer.
#pragma once
#include "am_rows.h"

namespace am {
namespace dev {

constexpr uint32_t kScoreMaxColumns = 8;                    // AM_SCORE_MAX_COLUMNS
constexpr uint32_t kTopkDigits = 8, kTopkBins = 256;        // eight passes of eight bits

// order-preserving: a < b as int64 iff score_key(a, true) < score_key(b, true) as uint64 (the sign bit biased); complemented for "smallest", so that the best
// score has the largest key either way
AM_HD uint64_t score_key(int64_t score, bool largest)
{
    const uint64_t k = (uint64_t)score ^ 0x8000000000000000ull;
    return largest ? k : ~k;
}

// the digit d of the k_left-th best key among the keys counted in hist (1 <= k_left <= the sum of hist): fewer than k_left keys carry a digit above d, at least
// k_left carry d or a digit above it.  *k_left becomes the rank among the keys with digit d (1 .. hist[d]).  A k_left beyond the sum (not reachable for a caller
// that keeps 1 <= k <= n) answers digit 0.
AM_HD uint32_t topk_pick(const uint64_t* hist, uint64_t* k_left)
{
    uint64_t above = 0;
    for (uint32_t d = kTopkBins; d-- > 0;) {
        const uint64_t c = hist[d];
        if (*k_left <= above + c || d == 0) { *k_left -= above; return d; }
        above += c;
    }
    return 0;
}

// does the key still take part in pass `digit` (7: the top byte, every key does; below: the keys whose bytes above `digit` are the chosen prefix)
AM_HD bool topk_in_prefix(uint64_t key, uint64_t prefix, uint32_t digit)
{
    return digit + 1 >= kTopkDigits || (key >> (8 * (digit + 1))) == prefix;
}

AM_HD uint32_t topk_digit(uint64_t key, uint32_t digit) { return (uint32_t)(key >> (8 * digit)) & (kTopkBins - 1); }

// the state of a radix select in HBM: the chosen digits (the key's bytes above the current pass, right-aligned) and what remains of k
struct TopkState { uint64_t prefix, k_left; };

// the weights of a scoring call as k_score reads them, and where the sums go: score[c][h] lives at scores[c * stride + h] for the haystacks h the records name
struct ScoreOut {
    const int64_t* weights; uint32_t n_cols, n_needles;     // int64[n_cols][n_needles]
    unsigned long long* scores; uint64_t stride;            // (unsigned: the adds wrap modulo 2^64, which is two's complement)
};

}  // namespace dev
}  // namespace am
