// am_subst.hip -- the splice of include/am.h "substitute": `replace :: [Match] -> Text -> Text` (reference: src/Data/Text/AhoCorasick/Replacer.hs:163-180) applied to the
// leftmost-longest spans of a batch (am_spans.hip), in HBM.  A haystack with k spans is 2k + 1 PIECES: gaps read from the source text, replacements read from the pool.
// Span j (global index) of haystack h owns pieces 2j + h (the gap before it) and 2j + h + 1 (its replacement); piece 2 * span_off[h + 1] + h is the tail of h: P = 2S + n_hay.
//   * k_subst_pieces: one lane per span writes its two pieces, one lane per haystack its tail: (length, tagged source offset) and whether the piece owns a byte.
//   * two exclusive sums (am_scan.hip): the lengths give every piece its destination, the flags give every LIVE piece (length > 0) its place in the compacted table.
//     Adjacent matches with empty replacements make unbounded runs of empty pieces; without them a tile of T destination bytes meets at most T pieces (each owns a
//     byte of it), every destination offset occurs once and the searches below see no duplicates.
//   * k_subst_compact: the live pieces as (destination, source) pairs + a sentinel; out_offsets[h] = destination of piece 2 * span_off[h] + h.
//   * k_subst_gather: a persistent grid over tiles of the NEW text.  The tile's slice of the piece table is staged in LDS (destination relative to the tile, 16 bits;
//     a piece that began before the tile is clipped to it), a lane owns one aligned 16-byte store and assembles it from the pieces it covers: per piece up to five
//     aligned dword loads that touch only dwords holding bytes of the piece, a byte shift (v_alignbyte) and a byte mask.  No byte loop: natural text has a piece end in
//     nearly every group.
// A table of TEMPLATES (am_subst_tpl.h) changes the piece plan and nothing else: k_subst_tpl_count gives span j its 1 + nseg pieces, their exclusive sum pbase numbers
// them (gap pbase[j] + h, segment s pbase[j] + h + 1 + s, tail pbase[span_off[h + 1]] + h, P = pbase[S] + n_hay), k_subst_tpl_pieces writes them -- a literal from the
// pool, the match itself from the text -- and the scans, k_subst_compact and k_subst_gather run as they are.  A table of plain replacements keeps k_subst_pieces.
// The bytes written depend on nothing but the piece table: no atomic takes part.  All indices are 64-bit.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "am_bounds.h"
#include "am_device.h"

AM_BOUNDS_TU("am_subst.hip")

namespace am {
namespace dev {

namespace {

constexpr uint32_t kSubstThreads = 256;                                // lanes of a k_subst_gather workgroup
constexpr uint32_t kSubstGroup = 16;                                   // bytes a lane of k_subst_gather writes with one store
constexpr uint32_t kSubstTile = kSubstThreads * kSubstGroup;           // bytes of new text per staging of the piece table
constexpr int kSubstBlocksPerCu = 3;                                   // 40 KiB of LDS each

__device__ __forceinline__ void put_piece(uint64_t* __restrict__ lens, uint64_t* __restrict__ src_at, uint32_t* __restrict__ live, uint64_t n_pieces, uint64_t i,
                                          uint64_t len, uint64_t at)
{
    AM_BOUNDS(i < n_pieces);
    if (i >= n_pieces) return;
    lens[i] = len;
    src_at[i] = at;
    live[i] = len != 0 ? 1u : 0u;
}

// lanes [0, n_span): the gap before a span and its replacement; lanes [n_span, n_span + n_hay): the tail of a haystack; the last lane: the scans' trailing zero.
// A piece whose source would leave the text or the pool (never, for the spans of this batch) is written with length 0.
__global__ void __launch_bounds__(kRowThreads) k_subst_pieces(SubstIn in, uint64_t* __restrict__ lens, uint64_t* __restrict__ src_at, uint32_t* __restrict__ live)
{
    const uint64_t i = global_row();
    const uint64_t n_pieces = 2 * in.n_span + in.n_hay;
    if (i > in.n_span + in.n_hay) return;
    if (i == in.n_span + in.n_hay) { lens[n_pieces] = 0; live[n_pieces] = 0; return; }
    if (i < in.n_span) {
        const Span sp = in.spans[i];
        const uint32_t h = sp.haystack;
        AM_BOUNDS(h < in.n_hay && sp.needle < in.n_needles);
        if (h >= in.n_hay) return;                                     // (its pieces cannot be named; never, see above)
        const uint64_t base = in.src_off[h], hay_len = in.src_off[h + 1] - base, first = in.span_off[h];
        AM_BOUNDS(first <= i && i < in.span_off[h + 1]);
        uint64_t prev_end = 0;
        if (i > first) { const Span q = in.spans[i - 1]; prev_end = q.start + q.len; }
        const bool ok = sp.needle < in.n_needles && sp.start >= prev_end && sp.start + sp.len <= hay_len && base + hay_len <= in.src_total;
        AM_BOUNDS(ok);
        uint64_t r0 = 0, r1 = 0;
        if (ok) { r0 = in.repl_off[sp.needle]; r1 = in.repl_off[sp.needle + 1]; }
        AM_BOUNDS(r0 <= r1 && r1 <= in.pool_bytes);
        const bool rok = r0 <= r1 && r1 <= in.pool_bytes;
        put_piece(lens, src_at, live, n_pieces, 2 * i + h, ok ? sp.start - prev_end : 0, base + prev_end);
        put_piece(lens, src_at, live, n_pieces, 2 * i + h + 1, rok ? r1 - r0 : 0, kSubstRepl | r0);
        return;
    }
    const uint64_t h = i - in.n_span;
    const uint64_t base = in.src_off[h], hay_len = in.src_off[h + 1] - base, e0 = in.span_off[h], e1 = in.span_off[h + 1];
    AM_BOUNDS(e0 <= e1 && e1 <= in.n_span);
    uint64_t last_end = 0;
    if (e1 > e0 && e1 <= in.n_span) { const Span q = in.spans[e1 - 1]; last_end = q.start + q.len; }
    const bool ok = last_end <= hay_len && base + hay_len <= in.src_total && e1 <= in.n_span;
    AM_BOUNDS(ok);
    put_piece(lens, src_at, live, n_pieces, 2 * (e1 <= in.n_span ? e1 : in.n_span) + h, ok ? hay_len - last_end : 0, base + last_end);
}

// ---- a table of templates (am_subst_tpl.h): span j owns 1 + nseg[needle_j] pieces, numbered through pbase = the exclusive sum of those counts

// lanes [0, n_span): the pieces span j owns; the last lane: the scan's trailing zero
__global__ void __launch_bounds__(kRowThreads) k_subst_tpl_count(SubstIn in, SubstTpl tpl, uint32_t* __restrict__ cnt)
{
    const uint64_t i = global_row();
    if (i > in.n_span) return;
    if (i == in.n_span) { cnt[i] = 0; return; }
    const uint32_t needle = in.spans[i].needle;
    AM_BOUNDS(needle < in.n_needles);
    cnt[i] = subst_tpl_count(tpl.seg_off, in.n_needles, needle);
}

// the lanes of k_subst_pieces with the template's pieces in the place of the replacement: lanes [0, n_span): the gap before a span and one piece per segment of its
// template; lanes [n_span, n_span + n_hay): the tail of a haystack; the last lane: the scans' trailing zero.  A span that fails the checks of k_subst_pieces (never,
// for the spans of this batch) leaves all its pieces at length 0, as the caller's memset made them.
__global__ void __launch_bounds__(kRowThreads) k_subst_tpl_pieces(SubstIn in, SubstTpl tpl, const uint64_t* __restrict__ pbase, uint64_t n_pieces, uint64_t* __restrict__ lens,
                                                                    uint64_t* __restrict__ src_at, uint32_t* __restrict__ live)
{
    const uint64_t i = global_row();
    if (i > in.n_span + in.n_hay) return;
    if (i == in.n_span + in.n_hay) { lens[n_pieces] = 0; live[n_pieces] = 0; return; }
    if (i < in.n_span) {
        const Span sp = in.spans[i];
        const uint32_t h = sp.haystack;
        AM_BOUNDS(h < in.n_hay && sp.needle < in.n_needles);
        if (h >= in.n_hay) return;                                     // (its pieces cannot be named; never, see above)
        const uint64_t base = in.src_off[h], hay_len = in.src_off[h + 1] - base, first = in.span_off[h];
        AM_BOUNDS(first <= i && i < in.span_off[h + 1]);
        uint64_t prev_end = 0;
        if (i > first) { const Span q = in.spans[i - 1]; prev_end = q.start + q.len; }
        const bool ok = sp.needle < in.n_needles && sp.start >= prev_end && sp.start + sp.len <= hay_len && base + hay_len <= in.src_total;
        AM_BOUNDS(ok);
        const uint64_t p0 = pbase[i];
        AM_BOUNDS(pbase[i + 1] - p0 == subst_tpl_count(tpl.seg_off, in.n_needles, sp.needle));
        put_piece(lens, src_at, live, n_pieces, subst_tpl_gap_piece(p0, h), ok ? sp.start - prev_end : 0, base + prev_end);
        if (!ok) return;
        uint64_t s0;
        const uint32_t nseg = subst_tpl_segments(tpl.seg_off, in.n_needles, sp.needle, &s0);
        AM_BOUNDS(s0 + nseg <= tpl.n_seg);
        if (s0 + nseg > tpl.n_seg) return;
        for (uint32_t s = 0; s < nseg; s++) {
            const SubstPiece pc = subst_tpl_piece(tpl.segs[s0 + s], in.pool_bytes, base + sp.start, sp.len);
            AM_BOUNDS(tpl.segs[s0 + s].kind == kSegMatch || pc.len == tpl.segs[s0 + s].len);
            put_piece(lens, src_at, live, n_pieces, subst_tpl_seg_piece(p0, h, s), pc.len, pc.src);
        }
        return;
    }
    const uint64_t h = i - in.n_span;
    const uint64_t base = in.src_off[h], hay_len = in.src_off[h + 1] - base, e0 = in.span_off[h], e1 = in.span_off[h + 1];
    AM_BOUNDS(e0 <= e1 && e1 <= in.n_span);
    uint64_t last_end = 0;
    if (e1 > e0 && e1 <= in.n_span) { const Span q = in.spans[e1 - 1]; last_end = q.start + q.len; }
    const bool ok = last_end <= hay_len && base + hay_len <= in.src_total && e1 <= in.n_span;
    AM_BOUNDS(ok);
    put_piece(lens, src_at, live, n_pieces, subst_tpl_gap_piece(pbase[e1 <= in.n_span ? e1 : in.n_span], h), ok ? hay_len - last_end : 0, base + last_end);
}

// lanes [0, n_pieces]: a live piece goes to its place in the compacted table, the last lane writes the sentinel; lanes beyond: out_offsets (n_hay + 1).  pbase: the
// piece numbering of a table of templates; null: the fixed plan 2j + h
__global__ void __launch_bounds__(kRowThreads) k_subst_compact(const uint64_t* __restrict__ src_at, const uint32_t* __restrict__ live, const uint64_t* __restrict__ dst_at,
                                                                 const uint64_t* __restrict__ cidx, uint64_t n_pieces, uint64_t* __restrict__ cdst, uint64_t* __restrict__ csrc,
                                                                 uint64_t n_live, const uint64_t* __restrict__ span_off, const uint64_t* __restrict__ pbase, uint64_t n_span,
                                                                 uint64_t n_hay, uint64_t* __restrict__ out_off)
{
    const uint64_t i = global_row();
    if (i <= n_pieces) {
        if (i == n_pieces) { AM_BOUNDS(cidx[i] == n_live); cdst[n_live] = dst_at[i]; csrc[n_live] = 0; return; }
        if (!live[i]) return;
        const uint64_t c = cidx[i];
        AM_BOUNDS(c < n_live);
        if (c >= n_live) return;
        cdst[c] = dst_at[i];
        csrc[c] = src_at[i];
        return;
    }
    const uint64_t h = i - n_pieces - 1;
    if (h > n_hay) return;
    const uint64_t e = span_off[h];
    const uint64_t ec = std::min<uint64_t>(e, n_span), p = pbase ? subst_tpl_gap_piece(pbase[ec], h) : 2 * ec + h;
    AM_BOUNDS(e <= n_span && p <= n_pieces);
    out_off[h] = dst_at[std::min<uint64_t>(p, n_pieces)];
}

__device__ __forceinline__ uint32_t bytes_below(int x) { return x <= 0 ? 0u : x >= 4 ? 0xFFFFFFFFu : (1u << (8 * x)) - 1u; }

// bytes [at, at + n) of `base` at bytes [p, p + n) of a 16-byte group, zeros elsewhere (n >= 1, p + n <= 16).  Only the aligned dwords that hold a byte of the piece
// are read: they lie inside round_up(at + n, 4), which is inside the text's and the pool's padding.
__device__ __forceinline__ uint4 load_piece(const uint8_t* __restrict__ base, uint64_t at, uint32_t n, uint32_t p)
{
    const int64_t s0 = (int64_t)at - (int64_t)p;                       // where byte 0 of the group would come from (may lie before the piece, even before `base`)
    const uint32_t a = (uint32_t)(s0 & 3);
    const int64_t first = s0 - (int64_t)a, lo = (int64_t)at, hi = (int64_t)at + (int64_t)n;
    uint32_t w[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int64_t d = first + 4 * j;
        w[j] = (d + 4 > lo && d < hi) ? *reinterpret_cast<const uint32_t*>(base + d) : 0u;
    }
    const int q = (int)p, e = (int)(p + n);
    uint4 v;
    v.x = __builtin_amdgcn_alignbyte(w[1], w[0], a) & bytes_below(e) & ~bytes_below(q);
    v.y = __builtin_amdgcn_alignbyte(w[2], w[1], a) & bytes_below(e - 4) & ~bytes_below(q - 4);
    v.z = __builtin_amdgcn_alignbyte(w[3], w[2], a) & bytes_below(e - 8) & ~bytes_below(q - 8);
    v.w = __builtin_amdgcn_alignbyte(w[4], w[3], a) & bytes_below(e - 12) & ~bytes_below(q - 12);
    return v;
}

__global__ void __launch_bounds__(kSubstThreads) k_subst_gather(const uint8_t* __restrict__ text, uint64_t src_total, const uint8_t* __restrict__ pool, uint64_t pool_bytes,
                                                                const uint64_t* __restrict__ cdst, const uint64_t* __restrict__ csrc, uint64_t n_live, uint64_t total,
                                                                uint8_t* __restrict__ dst)
{
    __shared__ uint64_t s_src[kSubstTile + 1];                         // tagged source of the tile's pieces, the first one advanced to the tile's start
    __shared__ uint64_t s_edge[2];                                     // the pieces of the tile's first and last byte
    __shared__ uint16_t s_rel[kSubstTile + 2];                         // where they start, relative to the tile; [n] = the tile's bytes
    const uint64_t n_tiles = (total + kSubstTile - 1) / kSubstTile;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {      // (the same tiles for every lane of the workgroup: the barriers are uniform)
        const uint64_t t0 = t * kSubstTile;
        const uint32_t bytes = (uint32_t)std::min<uint64_t>(total - t0, kSubstTile);
        __syncthreads();                                               // (the lanes of the tile before have read their pieces)
        if (threadIdx.x < 2) s_edge[threadIdx.x] = last_at_or_before<uint64_t, uint64_t>(cdst, 0, n_live - 1, threadIdx.x == 0 ? t0 : t0 + bytes - 1);
        __syncthreads();
        const uint64_t f0 = s_edge[0];
        AM_BOUNDS(s_edge[1] >= f0 && s_edge[1] - f0 < kSubstTile && s_edge[1] < n_live);
        const uint32_t n = (uint32_t)std::min<uint64_t>(s_edge[1] - f0 + 1, kSubstTile);
        for (uint32_t k = threadIdx.x; k < n; k += kSubstThreads) {
            const uint64_t d = cdst[f0 + k];
            uint64_t s = csrc[f0 + k];
            AM_BOUNDS(k == 0 ? d <= t0 : (d > t0 && d < t0 + bytes));
            uint32_t rel = 0;
            if (d < t0) s += t0 - d;
            else rel = (uint32_t)std::min<uint64_t>(d - t0, bytes);
            AM_BOUNDS(k <= kSubstTile);
            s_rel[k] = (uint16_t)rel;
            s_src[k] = s;
        }
        if (threadIdx.x == 0) s_rel[n] = (uint16_t)bytes;
        __syncthreads();
        const uint32_t g0 = threadIdx.x * kSubstGroup;
        if (g0 < bytes) {
            uint32_t k = last_at_or_before<uint16_t, uint32_t>(s_rel, 0, n - 1, g0);
            const uint32_t g1 = std::min(g0 + kSubstGroup, bytes);
            uint32_t pos = g0;
            uint4 v = make_uint4(0, 0, 0, 0);
            for (uint32_t step = 0; step < kSubstGroup && pos < g1; step++, k++) {      // (every piece owns a byte: at most 16 of them)
                AM_BOUNDS(k < n);
                if (k >= n) break;
                const uint32_t p0 = s_rel[k], p1 = s_rel[k + 1];
                AM_BOUNDS(p0 <= pos && pos < p1 && p1 <= bytes);
                if (!(p0 <= pos && pos < p1)) break;
                const uint32_t nb = std::min(p1, g1) - pos;
                const uint64_t tagged = s_src[k];
                const bool repl = (tagged & kSubstRepl) != 0;
                const uint64_t at = (tagged & ~kSubstRepl) + (pos - p0);
                const uint64_t limit = repl ? pool_bytes : src_total;
                AM_BOUNDS(at + nb <= limit);
                if (at + nb <= limit) {
                    const uint4 x = load_piece(repl ? pool : text, at, nb, pos - g0);
                    v.x |= x.x; v.y |= x.y; v.z |= x.z; v.w |= x.w;
                }
                pos += nb;
            }
            AM_BOUNDS(pos == g1);
            *reinterpret_cast<uint4*>(dst + t0 + g0) = v;              // (bytes beyond the end of the text are zeros: the buffer is padded to a whole group)
        }
    }
}

}  // namespace

void subst_geometry(uint32_t* group_bytes, uint32_t* tile_bytes) { *group_bytes = kSubstGroup; *tile_bytes = kSubstTile; }

hipError_t launch_subst_pieces(const SubstIn& in, uint64_t* lens, uint64_t* src_at, uint32_t* live, hipStream_t st)
{
    return launch_rows(k_subst_pieces, in.n_span + in.n_hay + 1, st, in, lens, src_at, live);
}

hipError_t launch_subst_tpl_count(const SubstIn& in, const SubstTpl& tpl, uint32_t* cnt, hipStream_t st)
{
    return launch_rows(k_subst_tpl_count, in.n_span + 1, st, in, tpl, cnt);
}

hipError_t launch_subst_tpl_pieces(const SubstIn& in, const SubstTpl& tpl, const uint64_t* pbase, uint64_t n_pieces, uint64_t* lens, uint64_t* src_at, uint32_t* live,
                                   hipStream_t st)
{
    return launch_rows(k_subst_tpl_pieces, in.n_span + in.n_hay + 1, st, in, tpl, pbase, n_pieces, lens, src_at, live);
}

hipError_t launch_subst_compact(const uint64_t* src_at, const uint32_t* live, const uint64_t* dst_at, const uint64_t* cidx, uint64_t n_pieces, uint64_t* cdst, uint64_t* csrc,
                                uint64_t n_live, const uint64_t* span_off, const uint64_t* pbase, uint64_t n_span, uint64_t n_hay, uint64_t* out_off, hipStream_t st)
{
    return launch_rows(k_subst_compact, n_pieces + 1 + n_hay + 1, st, src_at, live, dst_at, cidx, n_pieces, cdst, csrc, n_live, span_off, pbase, n_span, n_hay, out_off);
}

hipError_t launch_subst_gather(const uint8_t* text, uint64_t src_total, const uint8_t* pool, uint64_t pool_bytes, const uint64_t* cdst, const uint64_t* csrc, uint64_t n_live,
                               uint64_t total, uint8_t* dst, int n_cu, hipStream_t st)
{
    if (total == 0 || n_live == 0) return hipSuccess;
    const uint64_t n_tiles = (total + kSubstTile - 1) / kSubstTile;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)(n_cu > 0 ? n_cu : 1) * kSubstBlocksPerCu);
    hipLaunchKernelGGL(k_subst_gather, dim3(grid), dim3(kSubstThreads), 0, st, text, src_total, pool, pool_bytes, cdst, csrc, n_live, total, dst);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace am
