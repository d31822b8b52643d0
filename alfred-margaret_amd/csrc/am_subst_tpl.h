// am_subst_tpl.h -- the piece plan of a substitution TEMPLATE (include/am.h "substitute templates"), ONE definition for the device and the host: how many pieces a
// span owns, which index each of them has, and what piece one (span, segment) is.  A template is a sequence of segments, each a literal (bytes of the pool) or the
// match itself (bytes of the text).  Span j (global index) of haystack h owns 1 + nseg[needle_j] pieces: with pbase = the exclusive sum of those counts over the
// spans, its gap is piece pbase[j] + h and segment s of its template piece pbase[j] + h + 1 + s; the tail of haystack h is piece pbase[span_off[h + 1]] + h, and
// there are P = pbase[S] + n_hay pieces (one more piece per haystack before h shifts everything by h, as in the fixed plan 2j + h of am_subst.hip).  A piece is a
// (length, tagged source) pair as k_subst_gather reads it: a literal is kSubstRepl | pool offset, a match is the span's own bytes of the text, untagged.
// Plain C++: tests/native/subst_templates_main.cpp compiles all of it with g++ and holds it to the sequential definition (host/spans.hpp substituteTemplates) under
// a sanitizer.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AM_SUBST_HD __host__ __device__ __forceinline__
#else
#define AM_SUBST_HD inline
#endif

namespace am {
namespace dev {

constexpr uint64_t kSubstRepl = 1ull << 63;                 // a piece's source: offset into the replacement pool instead of the batch text
constexpr uint32_t kSubstMaxSegments = 64;                  // AM_SUBST_MAX_SEGMENTS
constexpr uint32_t kSegLiteral = 0, kSegMatch = 1;          // AM_SEG_LITERAL, AM_SEG_MATCH

struct alignas(8) SubstSeg { uint64_t at; uint32_t len, kind; };        // a segment as the kernels read it: a literal is pool[at, at + len); a match has at = len = 0
struct SubstPiece { uint64_t len, src; };

// the segments of the template of `needle`: [first, first + n); a handle the table does not know (never, for the spans of its own span table) has none
AM_SUBST_HD uint32_t subst_tpl_segments(const uint64_t* seg_off, uint32_t n_needles, uint32_t needle, uint64_t* first)
{
    if (needle >= n_needles) { *first = 0; return 0; }
    const uint64_t s0 = seg_off[needle], s1 = seg_off[needle + 1];
    *first = s0;
    return s1 >= s0 && s1 - s0 <= kSubstMaxSegments ? (uint32_t)(s1 - s0) : 0u;
}

// pieces span j owns: its gap and one per segment
AM_SUBST_HD uint32_t subst_tpl_count(const uint64_t* seg_off, uint32_t n_needles, uint32_t needle)
{
    uint64_t first;
    return 1u + subst_tpl_segments(seg_off, n_needles, needle, &first);
}

// the gap before span j of haystack h (pbase_j = pbase[j]); with j = span_off[h + 1] the tail of h, with j = span_off[h] the piece haystack h begins with
AM_SUBST_HD uint64_t subst_tpl_gap_piece(uint64_t pbase_j, uint64_t h) { return pbase_j + h; }
AM_SUBST_HD uint64_t subst_tpl_seg_piece(uint64_t pbase_j, uint64_t h, uint32_t s) { return pbase_j + h + 1u + s; }

// the piece of one (span, segment): the span's bytes are text[match_at, match_at + match_len).  A literal that would leave the pool (never, for a table that
// am_subst_table_create_templates made) and an unknown kind are pieces of length 0.
AM_SUBST_HD SubstPiece subst_tpl_piece(const SubstSeg& sg, uint64_t pool_bytes, uint64_t match_at, uint64_t match_len)
{
    if (sg.kind == kSegMatch) return SubstPiece{match_len, match_at};
    const bool ok = sg.kind == kSegLiteral && sg.at <= pool_bytes && sg.len <= pool_bytes - sg.at;
    return SubstPiece{ok ? (uint64_t)sg.len : 0ull, kSubstRepl | sg.at};
}

}  // namespace dev
}  // namespace am
