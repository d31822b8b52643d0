// am_coords.h -- match coordinates (include/am.h "coordinates"): the class masks of an aligned 16-byte group, the tile counts' host twin and the lookup over the prefix
// arrays, as host and device code: the kernels of am_coords.hip and tests/native/coords_lookup_main.cpp (the same functions on the CPU against byte loops) run it.
//
// Three byte classes: START ((b & 0xC0) != 0x80, the rule of am_extract.hip), FOUR (b >= 0xF0: the lead byte of a four-byte sequence, a surrogate pair in UTF-16) and
// NEWLINE (b == 0x0A).  A TILE is 128 aligned bytes of the batch's text (one L2 line); the index keeps, per class it carries, prefix[t] = the class count of the bytes
// [0, 128 * t) as a uint64, t = 0 .. n_tiles.  The prefix knows nothing about haystacks: a haystack-relative value is always count(base + p) - count(base), which is
// what makes seams, empty haystacks and the padding harmless.  Every load is an aligned 16-byte group that begins below the byte asked about, so it ends at or before
// round_up(total, 16), which every batch can read; a lookup at a tile boundary loads no text at all.  Internal: nothing here is part of the C ABI.
// Plain C++: the test program compiles all of it with g++.
#pragma once
#include "am_rows.h"

#if defined(__HIPCC__)
#include "am_bounds.h"
#elif !defined(AM_BOUNDS)
#define AM_BOUNDS(cond) ((void)0)
#endif

namespace am {
namespace dev {

constexpr uint32_t kCoordsTile = 128;                       // bytes of a tile
constexpr uint32_t kCoordsTileShift = 7;
constexpr uint32_t kCoordsGroup = 16;                       // bytes of an aligned group: one load
enum CoordsClass : uint32_t { kCoordsStart = 0, kCoordsFour = 1, kCoordsNewline = 2, kCoordsClasses = 3 };

// bits 0, 8, 16, 24 of nz gathered into bits 0 .. 3 (the sixteen partial products land on distinct bits: no carry)
AM_HD uint32_t coords_gather4(uint32_t nz) { return ((nz * 0x01020408u) >> 24) & 0xFu; }

// bit j (0..3) = byte j of the dword (the lowest address first) belongs to the class
template <uint32_t CLS>
AM_HD uint32_t coords_bits4(uint32_t w)
{
    if (CLS == kCoordsStart) {
        const uint32_t t = (w & 0xC0C0C0C0u) ^ 0x80808080u; // a byte of t is zero iff the byte is a continuation byte; only its bits 7 and 6 can be set
        return coords_gather4(((t | (t << 1)) & 0x80808080u) >> 7);
    }
    if (CLS == kCoordsFour) {                               // the four high bits all set: bit 7 of (w << k) is bit 7 - k of the same byte for k <= 3
        return coords_gather4((w & (w << 1) & (w << 2) & (w << 3) & 0x80808080u) >> 7);
    }
    const uint32_t x = w ^ 0x0A0A0A0Au;                     // a byte of x is zero iff the byte is 0x0A; (x & 0x7F) + 0x7F <= 0xFE: no carry between bytes
    return coords_gather4((~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u) >> 7);
}

struct alignas(16) CoordsWords { uint32_t x, y, z, w; };   // an aligned group as one 16-byte load
AM_HD CoordsWords coords_load(const uint8_t* __restrict__ text, uint64_t g)
{
    return *reinterpret_cast<const CoordsWords*>(text + g);
}

// bit j (0..15) = byte j of the aligned group belongs to the class
template <uint32_t CLS>
AM_HD uint32_t coords_mask16(const CoordsWords& v)
{
    return coords_bits4<CLS>(v.x) | (coords_bits4<CLS>(v.y) << 4) | (coords_bits4<CLS>(v.z) << 8) | (coords_bits4<CLS>(v.w) << 12);
}

// the bits [0, n) of a 16-bit mask, n <= 16
AM_HD uint32_t coords_low_bits(uint32_t n) { return (1u << n) - 1u; }

// position of the n-th set bit of the 16-bit mask m counted from bit 0, 1 <= n <= popcount(m)
AM_HD uint32_t coords_nth_set(uint32_t m, uint32_t n)
{
    uint32_t pos = 0, c;
    c = (uint32_t)__builtin_popcount(m & 0xFFu); if (n > c) { n -= c; pos += 8; m >>= 8; }
    c = (uint32_t)__builtin_popcount(m & 0xFu);  if (n > c) { n -= c; pos += 4; m >>= 4; }
    c = (uint32_t)__builtin_popcount(m & 0x3u);  if (n > c) { n -= c; pos += 2; m >>= 2; }
    c = m & 1u;                                  if (n > c) { pos += 1; }
    return pos;
}

// the class bits of the group at q, a multiple of 16, cut at `total`: what the tile pass counts (bytes of the padding never count)
template <uint32_t CLS>
AM_HD uint32_t coords_group_count(const CoordsWords& v, uint64_t q, uint64_t total)
{
    uint32_t m = coords_mask16<CLS>(v);
    if (total - q < kCoordsGroup) m &= coords_low_bits((uint32_t)(total - q));
    return (uint32_t)__builtin_popcount(m);
}

// the tile pass's host twin: counts[t] for the tiles of text[0, total), counts[n_tiles] = 0 (the sum's trailing element); text is readable to round_up(total, 16)
template <uint32_t CLS>
inline void coords_tile_counts_host(const uint8_t* text, uint64_t total, uint32_t* counts)
{
    const uint64_t n_tiles = (total + kCoordsTile - 1) >> kCoordsTileShift;
    for (uint64_t t = 0; t <= n_tiles; t++) counts[t] = 0;
    for (uint64_t q = 0; q < total; q += kCoordsGroup) counts[q >> kCoordsTileShift] += coords_group_count<CLS>(coords_load(text, q), q, total);
}

// the class count of the bytes [0, g), g <= total: one prefix entry and at most eight groups of g's own tile, the last one cut at g.  Every group read begins below
// g, so it ends at or before round_up(g, 16) <= padded; g at a tile boundary reads no text.
template <uint32_t CLS>
AM_HD uint64_t coords_count(const uint8_t* __restrict__ text, const uint64_t* __restrict__ prefix, uint64_t g, uint64_t padded)
{
    uint64_t c = prefix[g >> kCoordsTileShift];
    for (uint64_t q = g & ~(uint64_t)(kCoordsTile - 1); q < g; q += kCoordsGroup) {
        AM_BOUNDS(q + kCoordsGroup <= padded);
        uint32_t m = coords_mask16<CLS>(coords_load(text, q));
        if (g - q < kCoordsGroup) m &= coords_low_bits((uint32_t)(g - q));
        c += (uint32_t)__builtin_popcount(m);
    }
    return c;
}

// 1 + the index of the last 0x0A among the bytes [base, g), or base when there is none; base <= g <= total.  n_g / n_base: the newlines of [0, g) / [0, base), which
// the caller has (coords_count).  The newline wanted is the n_g-th of the text.  It lies in g's own tile when that tile's prefix is below n_g -- the common case --,
// else in the last tile between base's and g's whose prefix is below n_g, found by a binary search; an n-th-set-bit select inside the tile finishes.  The tile found
// is g's own (the newline lies below g) or a whole tile below g: every group read ends at or before `padded`.
AM_HD uint64_t coords_linestart(const uint8_t* __restrict__ text, const uint64_t* __restrict__ nl_prefix, uint64_t base, uint64_t g, uint64_t n_g,
                                       uint64_t n_base, uint64_t padded)
{
    if (n_g <= n_base) return base;
    uint64_t t = g >> kCoordsTileShift;
    if (nl_prefix[t] >= n_g) t = last_at_or_before(nl_prefix, base >> kCoordsTileShift, t - 1, n_g - 1);      // (prefix[tile of base] <= n_base <= n_g - 1)
    uint64_t n = n_g - nl_prefix[t];
    AM_BOUNDS(n >= 1 && n <= kCoordsTile);
    uint64_t q = t << kCoordsTileShift;
    for (uint32_t k = 0; k < kCoordsTile / kCoordsGroup; k++, q += kCoordsGroup) {
        AM_BOUNDS(q + kCoordsGroup <= padded);
        const uint32_t m = coords_mask16<kCoordsNewline>(coords_load(text, q));
        const uint32_t c = (uint32_t)__builtin_popcount(m);
        if (n <= c) return q + coords_nth_set(m, (uint32_t)n) + 1;
        n -= c;
    }
    AM_BOUNDS(false);
    return base;
}

// what a consumer reads: the text and the prefix arrays the index carries (null: not carried; the host has checked that the call's unit has what it needs)
struct CoordsIn {
    const uint8_t* text; const uint64_t* offsets;           // the batch's
    const uint64_t* prefix[kCoordsClasses];
    uint64_t total, padded; uint32_t n_hay;
};

// U(g) for unit 0 bytes / 1 code points / 2 UTF-16 code units (AM_UNIT_*), over the bytes [0, g)
AM_HD uint64_t coords_units(const CoordsIn& in, int unit, uint64_t g)
{
    if (unit == 0) return g;
    uint64_t u = coords_count<kCoordsStart>(in.text, in.prefix[kCoordsStart], g, in.padded);
    if (unit == 2) u += coords_count<kCoordsFour>(in.text, in.prefix[kCoordsFour], g, in.padded);
    return u;
}

struct CoordsLineCol { uint64_t line, col, linestart, newlines; };
// line and column of the byte g of the haystack at base (n_base: the newlines of [0, base)); reuse: a position on the same line whose line start is known (null: none)
AM_HD CoordsLineCol coords_line_col(const CoordsIn& in, int unit, uint64_t base, uint64_t n_base, uint64_t g, const CoordsLineCol* reuse)
{
    CoordsLineCol r;
    r.newlines = coords_count<kCoordsNewline>(in.text, in.prefix[kCoordsNewline], g, in.padded);
    r.line = r.newlines - n_base;
    r.linestart = reuse && reuse->newlines == r.newlines ? reuse->linestart : coords_linestart(in.text, in.prefix[kCoordsNewline], base, g, r.newlines, n_base, in.padded);
    r.col = coords_units(in, unit, g) - coords_units(in, unit, r.linestart);
    return r;
}

}  // namespace dev
}  // namespace am

#if defined(__HIPCC__)
#include "am_device.h"

namespace am {
namespace dev {

struct SpanRange { uint64_t start_line, start_col, end_line, end_col; };      // = am_span_range in include/am.h

// am_coords.hip.  k_coords_tiles: counts[c][t] = the class-c bytes of tile t for every class c with counts[c] given (null: not asked for), t < n_tiles; the entry
// counts[c][n_tiles] is the caller's to clear (the sum's trailing element).  Bytes from `total` on never count.
hipError_t launch_coords_tiles(const uint8_t* text, uint64_t total, uint32_t* const counts[kCoordsClasses], hipStream_t st);
// one lane per row; `unit` is AM_UNIT_CODE_POINTS or AM_UNIT_UTF16 for the first two (bytes is a copy, made by the host), any unit for the columns and positions
hipError_t launch_coords_spans(const CoordsIn& in, int unit, const Span* spans, uint64_t n, Span* out, hipStream_t st);
hipError_t launch_coords_fragments(const CoordsIn& in, int unit, const Fragment* frags, const uint64_t* frag_off, uint64_t n, Fragment* out, hipStream_t st);
hipError_t launch_coords_ranges(const CoordsIn& in, int unit, const Span* spans, uint64_t n, SpanRange* out, hipStream_t st);
// out[i] = U(pos[i]) of haystack hay[i]; hay[i] >= n_hay or pos[i] beyond the haystack: *flag = 1 (a plain store; the caller cleared it), out[i] unspecified
hipError_t launch_coords_positions(const CoordsIn& in, int unit, const uint32_t* hay, const uint64_t* pos, uint64_t n, uint64_t* out, uint64_t* flag, hipStream_t st);

}  // namespace dev
}  // namespace am
#endif
