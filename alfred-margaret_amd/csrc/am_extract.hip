// am_extract.hip -- extract on the device (include/am.h "extract"): the stage between am_spans and am_fragments.  Every span becomes its WINDOW -- the span with up to
// `before` code points of its own haystack in front of it and up to `after` behind it -- as a fragment of the haystack, one per span (AM_EXTRACT_EACH) or, per haystack,
// the union of the windows as disjoint ascending pieces (AM_EXTRACT_MERGED, over leftmost-longest rows: ws and we are both non-decreasing there, so a comparison with
// the neighbour decides).
//
// k_extract_windows takes one lane per span and walks ALIGNED 16-byte groups of the batch's text in batch-absolute coordinates (the text is 16-byte aligned and readable
// to round_up(total, 16) for every batch): one 16-byte load, the 16-bit mask of the group's START bytes ((b & 0xC0) != 0x80), ANDed with the bits that lie inside the
// span's own haystack and on the walk's side of the span, a popcount; the group that holds the wanted START byte selects it (the n-th set bit from the top going left,
// from the bottom going right), any other group is subtracted and the walk moves one group on.  Bytes of the neighbouring haystacks and of the padding behind the text
// are masked away before they are counted, so what they hold does not matter.  Loads per side: see DESIGN 7.8.
// MERGED: k_extract_heads flags the spans that open a piece, one exclusive sum (am_scan.hip) ranks them, k_extract_emit writes the pieces and the piece offsets.
// All positions are 64-bit; the only 32-bit quantities are haystack indices and the two context widths.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "am_bounds.h"
#include "am_device.h"

AM_BOUNDS_TU("am_extract.hip")

namespace am {
namespace dev {

namespace {

constexpr uint32_t kGroup = 16;                             // bytes of an aligned group of the walk
constexpr uint32_t kHeadWalk = 16;                          // spans the last lane of a run looks back at before it searches the ranks for its head

// bit j (0..3) = byte j of the dword (little endian: the lowest address first) is a START byte
__host__ __device__ __forceinline__ uint32_t start_bits4(uint32_t w)
{
    const uint32_t t = (w & 0xC0C0C0C0u) ^ 0x80808080u;     // a byte of t is zero iff the byte is a continuation byte; only its bits 7 and 6 can be set
    const uint32_t nz = ((t | (t << 1)) & 0x80808080u) >> 7;      // bit 0 of every byte: the byte of t is not zero
    return ((nz * 0x01020408u) >> 24) & 0xFu;               // bits 0, 8, 16, 24 gathered into bits 24..27
}

// bit j (0..15) = byte j of the aligned group is a START byte
__host__ __device__ __forceinline__ uint32_t start_mask16(const uint4& v)
{
    return start_bits4(v.x) | (start_bits4(v.y) << 4) | (start_bits4(v.z) << 8) | (start_bits4(v.w) << 12);
}

// the bits [lo, hi) of a 16-bit mask, 0 <= lo, hi <= 16 (lo >= hi: none)
__host__ __device__ __forceinline__ uint32_t bits_between(uint32_t lo, uint32_t hi)
{
    return lo < hi ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}

// position of the n-th set bit of the 16-bit mask m counted from bit 0, 1 <= n <= popcount(m)
__host__ __device__ __forceinline__ uint32_t nth_set_from_bottom(uint32_t m, uint32_t n)
{
    uint32_t pos = 0, c;
    c = (uint32_t)__builtin_popcount(m & 0xFFu); if (n > c) { n -= c; pos += 8; m >>= 8; }
    c = (uint32_t)__builtin_popcount(m & 0xFu);  if (n > c) { n -= c; pos += 4; m >>= 4; }
    c = (uint32_t)__builtin_popcount(m & 0x3u);  if (n > c) { n -= c; pos += 2; m >>= 2; }
    c = m & 1u;                                  if (n > c) { pos += 1; }
    return pos;
}

// ... counted from bit 15 downwards
__host__ __device__ __forceinline__ uint32_t nth_set_from_top(uint32_t m, uint32_t n)
{
    return 15u - nth_set_from_bottom(__builtin_bitreverse32(m) >> 16, n);
}

__host__ __device__ __forceinline__ uint4 load_group(const uint8_t* __restrict__ text, uint64_t g)
{
    return *reinterpret_cast<const uint4*>(text + g);
}

// the batch-absolute index of the n-th START byte among the indices [base, s), counted leftwards from s; base when there are fewer.  n >= 1, base <= s <= padded:
// every group read begins below s, so it ends at or before round_up(s, 16) <= padded.
__host__ __device__ __forceinline__ uint64_t walk_left(const uint8_t* __restrict__ text, uint64_t base, uint64_t s, uint32_t n, uint64_t padded)
{
    if (s <= base) return base;
    uint64_t g = (s - 1) & ~(uint64_t)(kGroup - 1);
    for (;;) {
        AM_BOUNDS(g + kGroup <= padded);
        if (g + kGroup > padded) return base;
        const uint32_t lo = base > g ? (uint32_t)(base - g) : 0u;                  // < 16: base < s <= g + 16 and base > g
        const uint32_t hi = s - g < kGroup ? (uint32_t)(s - g) : kGroup;           // >= 1: g < s
        const uint32_t m = start_mask16(load_group(text, g)) & bits_between(lo, hi);
        const uint32_t c = (uint32_t)__builtin_popcount(m);
        if (c >= n) return g + nth_set_from_top(m, n);
        n -= c;
        if (g <= base) return base;
        g -= kGroup;
    }
}

// the batch-absolute index of the n-th START byte among the indices (e, next), counted rightwards from e; next when there are fewer.  n >= 1, e <= next <= total:
// every group read begins below next, so it ends at or before round_up(next, 16) <= padded.
__host__ __device__ __forceinline__ uint64_t walk_right(const uint8_t* __restrict__ text, uint64_t e, uint64_t next, uint32_t n, uint64_t padded)
{
    if (e + 1 >= next) return next;
    uint64_t g = (e + 1) & ~(uint64_t)(kGroup - 1);
    for (;;) {
        AM_BOUNDS(g + kGroup <= padded);
        if (g + kGroup > padded) return next;
        const uint32_t lo = e + 1 > g ? (uint32_t)(e + 1 - g) : 0u;                // < 16: g is the group of e + 1, or lies beyond it
        const uint32_t hi = next - g < kGroup ? (uint32_t)(next - g) : kGroup;     // >= 1: g < next
        const uint32_t m = start_mask16(load_group(text, g)) & bits_between(lo, hi);
        const uint32_t c = (uint32_t)__builtin_popcount(m);
        if (c >= n) return g + nth_set_from_bottom(m, n);
        n -= c;
        g += kGroup;
        if (g >= next) return next;
    }
}

// one lane per span: its window, relative to its haystack.  EACH: the fragment itself.  MERGED: ws / we for the heads and the emit.  A span that does not lie inside
// its haystack (not reachable for a row of a spans call over this batch) becomes the empty window at 0 without a read.
template <bool EACH>
__global__ void __launch_bounds__(kRowThreads) k_extract_windows(const Span* __restrict__ spans, uint64_t n_span, const uint8_t* __restrict__ text,
                                                                 const uint64_t* __restrict__ src_offsets, uint32_t n_hay, uint64_t total, uint32_t before, uint32_t after,
                                                                 Fragment* __restrict__ frags, uint64_t* __restrict__ ws_out, uint64_t* __restrict__ we_out)
{
    const uint64_t i = global_row();
    if (i >= n_span) return;
    const Span sp = spans[i];
    uint64_t ws = 0, we = 0;
    AM_BOUNDS(sp.haystack < n_hay);
    if (sp.haystack < n_hay) {
        const uint64_t base = src_offsets[sp.haystack], next = src_offsets[sp.haystack + 1];
        AM_BOUNDS(base <= next && next <= total && sp.start <= next - base && sp.len <= next - base - sp.start);
        if (base <= next && next <= total && sp.start <= next - base && sp.len <= next - base - sp.start) {
            const uint64_t padded = (total + (kGroup - 1)) & ~(uint64_t)(kGroup - 1);
            const uint64_t s = base + sp.start, e = s + sp.len;
            ws = (before ? walk_left(text, base, s, before, padded) : s) - base;
            we = (after ? walk_right(text, e, next, after, padded) : e) - base;
            AM_BOUNDS(ws <= sp.start && we >= sp.start + sp.len && we <= next - base);
        }
    }
    if (EACH) frags[i] = Fragment{ws, we - ws};
    else { ws_out[i] = ws; we_out[i] = we; }
}

// one lane per span (+ one for the trailing zero of the sum's input): the span opens a piece
__global__ void __launch_bounds__(kRowThreads) k_extract_heads(const Span* __restrict__ spans, uint64_t n_span, const uint64_t* __restrict__ ws, const uint64_t* __restrict__ we,
                                                               uint32_t* __restrict__ head)
{
    const uint64_t i = global_row();
    if (i > n_span) return;
    if (i == n_span) { head[i] = 0; return; }
    head[i] = i == 0 || spans[i].haystack != spans[i - 1].haystack || ws[i] > we[i - 1] ? 1u : 0u;
}

// lanes [0, n_span): with rank = the exclusive sum of head (rank[n_span] = n_pieces), the head of piece p = rank[head] writes the piece's start and the last span of
// the run its length -- it finds its head among the kHeadWalk spans before it, or, in a longer run, as the last span whose rank is <= p (every later span of the run
// has rank p + 1).  Lanes [0, n_hay]: the piece offsets, out_off[h] = rank[span_off[h]] (the first span of a haystack opens a piece, so its rank counts the pieces of
// the haystacks before it; the closing entry is rank[n_span] = n_pieces).
__global__ void __launch_bounds__(kRowThreads) k_extract_emit(const uint32_t* __restrict__ head, const uint64_t* __restrict__ rank, const uint64_t* __restrict__ ws,
                                                              const uint64_t* __restrict__ we, uint64_t n_span, uint64_t n_pieces, const uint64_t* __restrict__ span_off,
                                                              uint64_t n_hay, Fragment* __restrict__ frags, uint64_t* __restrict__ out_off)
{
    const uint64_t i = global_row();
    if (i <= n_hay) {
        const uint64_t k = span_off[i];
        AM_BOUNDS(k <= n_span && rank[k <= n_span ? k : n_span] <= n_pieces);
        out_off[i] = rank[k <= n_span ? k : n_span];
    }
    if (i >= n_span) return;
    const bool is_head = head[i] != 0;
    const uint64_t p = rank[i] + (is_head ? 1u : 0u) - 1u;  // (head[0] = 1: no lane forms 0 - 1)
    AM_BOUNDS(p < n_pieces);
    if (p >= n_pieces) return;
    if (is_head) frags[p].start = ws[i];
    if (!head[i + 1] && i + 1 < n_span) return;             // (head has n_span + 1 entries, the last one 0)
    uint64_t j = i;
    for (uint32_t k = 0; k < kHeadWalk && j > 0 && !head[j]; k++) j--;
    if (!head[j]) j = last_at_or_before(rank, (uint64_t)0, j, p);       // (rank ascends, rank[0] = 0 <= p)
    AM_BOUNDS(head[j] && rank[j] == p && ws[j] <= we[i]);
    frags[p].len = we[i] >= ws[j] ? we[i] - ws[j] : 0;
}

}  // namespace

hipError_t launch_extract_windows(const Span* spans, uint64_t n_span, const uint8_t* text, const uint64_t* src_offsets, uint32_t n_hay, uint64_t total, uint32_t before,
                                  uint32_t after, Fragment* frags, uint64_t* ws, uint64_t* we, hipStream_t st)
{
    return launch_rows(frags ? k_extract_windows<true> : k_extract_windows<false>, n_span, st, spans, n_span, text, src_offsets, n_hay, total, before, after, frags, ws, we);
}

hipError_t launch_extract_heads(const Span* spans, uint64_t n_span, const uint64_t* ws, const uint64_t* we, uint32_t* head, hipStream_t st)
{
    return launch_rows(k_extract_heads, n_span + 1, st, spans, n_span, ws, we, head);
}

hipError_t launch_extract_emit(const uint32_t* head, const uint64_t* rank, const uint64_t* ws, const uint64_t* we, uint64_t n_span, uint64_t n_pieces, const uint64_t* span_off,
                               uint64_t n_hay, Fragment* frags, uint64_t* out_off, hipStream_t st)
{
    return launch_rows(k_extract_emit, std::max(n_span, n_hay + 1), st, head, rank, ws, we, n_span, n_pieces, span_off, n_hay, frags, out_off);
}

}  // namespace dev
}  // namespace am
