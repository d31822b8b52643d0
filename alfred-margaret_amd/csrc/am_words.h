// am_words.h -- the span of a (record, value) pair and the whole-word predicate on it (include/am.h "whole words"), shared by the span expansion (am_spans.hip), the
// whole-word histogram (am_hist.hip), the whole-word scores (am_score.hip) and the select's flags (am_records.hip): all decide `keep` with the same device function,
// so a row the expansion writes is a value the others add or flag.  The record and its value come from the walk of am_records.h.
// A WORD CLASS is 256 flags packed into 8 dwords (bit b & 31 of word b >> 5): 32 bytes, one cache line for every lane, in HBM beside the table's lengths or staged in
// LDS.  A span (start, len) of a haystack of L bytes is a whole word iff (start == 0 or hay[start - 1] is no word byte) and (start + len == L or hay[start + len] is no
// word byte): the neighbours are bytes of the SAME haystack, never of the one before or after it in the batch, never the zero padding behind the text.
// EXACT CASE (include/am.h "exact case") is a second predicate of the same kind, between the expansion and the selection: a handle may carry a spelling, and a span
// of it is a row only where the text spells it so.  The byte comparison is am_cased.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "am_bounds.h"
#include "am_cased.h"
#include "am_device.h"
#include "am_wave.h"

namespace am {
namespace dev {

// start of the match of needle v that ends at r.end_pos, relative to the haystack (Replacer.hs:264-274 makeMatch; a needle of length 0 starts where it ends)
template <bool IC>
__device__ __forceinline__ uint64_t span_start(const SpansIn& in, const Record& r, uint32_t v)
{
    AM_BOUNDS(v < in.n_needles);
    const uint32_t nb = in.len_bytes[v];
    if (nb == 0) return r.end_pos;
    if (!IC) return r.end_pos >= nb ? r.end_pos - nb : 0;
    AM_BOUNDS(r.haystack < in.n_hay);
    if (r.haystack >= in.n_hay || r.end_pos == 0) return 0;
    const uint64_t base = in.offsets[r.haystack];
    AM_BOUNDS(base + r.end_pos <= in.total);
    if (base + r.end_pos > in.total) return 0;
    const uint8_t* hay = in.text + base;
    return skip_code_points_backwards(hay, r.end_pos, in.len_cps[v] - 1);      // (nb != 0: the table has at least one code point for it)
}

__device__ __forceinline__ bool is_word_byte(const uint32_t* words, uint8_t b) { return ((words[b >> 5] >> (b & 31u)) & 1u) != 0; }

// the whole-word rule for the span [start, start + len) of haystack h; `words`: the 8 dwords of the class, in HBM or LDS.  A span that does not lie inside its
// haystack (not reachable for a record of a scan of this batch) is dropped without a read.
__device__ __forceinline__ bool whole_word(const SpansIn& in, uint32_t h, uint64_t start, uint64_t len, const uint32_t* words)
{
    AM_BOUNDS(h < in.n_hay);
    if (h >= in.n_hay) return false;
    const uint64_t base = in.offsets[h], next = in.offsets[h + 1];
    AM_BOUNDS(base <= next && next <= in.total && start + len <= next - base);
    if (base > next || next > in.total || start + len > next - base) return false;
    if (start > 0 && is_word_byte(words, in.text[base + start - 1])) return false;           // base <= base + start - 1 < next <= total
    if (base + start + len < next && is_word_byte(words, in.text[base + start + len])) return false;      // < next <= total: a byte of this haystack
    return true;
}

// (start, len) of value v < n_needles of record r, and whether the table keeps it: always without a predicate; WORDS: the whole-word rule; EXACT (include/am.h
// "exact case"): a handle with a spelling of e bytes is kept only where the text spells it so, byte for byte -- with both, both must hold.
// EXACT takes a shortcut the definition allows: the row is kept iff end_pos >= e and hay[end_pos - e, end_pos) == exact[v], and then start = end_pos - e, without the
// backwards walk.  The table was made only after checking that the spelling begins with a START byte and holds exactly len_code_points[v] of them, so where the bytes
// are equal skip_code_points_backwards lands on end_pos - e (len == e, the definition keeps the row), and where they are not the definition drops the row whatever its
// len is.  Case-sensitive spans take the needle's own len_bytes instead of a walk: there the definition's len == e is tested as it stands.
template <bool IC, bool WORDS, bool EXACT = false>
__device__ __forceinline__ bool span_of(const SpansIn& in, const Record& r, uint32_t v, const uint32_t* words, uint64_t& start, uint64_t& len)
{
    if (EXACT) {
        AM_BOUNDS(v < in.n_needles);
        const ExactRef x = in.exact[v];
        if (x.len != 0) {
            start = r.end_pos; len = 0;
            AM_BOUNDS(r.haystack < in.n_hay);
            if (r.haystack >= in.n_hay || r.end_pos < x.len) return false;
            if (!IC && in.len_bytes[v] != x.len) return false;
            const uint64_t base = in.offsets[r.haystack], next = in.offsets[r.haystack + 1];
            AM_BOUNDS(base <= next && next <= in.total && r.end_pos <= next - base);
            if (base > next || next > in.total || r.end_pos > next - base) return false;
            start = r.end_pos - x.len; len = x.len;
            if (!cased_equal(in.text, base, next, base + start, in.exact_pool, (uint64_t)x.at16 * kCasedGroup, x.len)) return false;
            return WORDS ? whole_word(in, r.haystack, start, len, words) : true;
        }
    }
    start = span_start<IC>(in, r, v);
    len = r.end_pos >= start ? r.end_pos - start : 0;
    if (!WORDS) return true;
    return whole_word(in, r.haystack, start, len, words);
}

}  // namespace dev
}  // namespace am
