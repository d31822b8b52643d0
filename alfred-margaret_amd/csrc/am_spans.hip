// am_spans.hip -- match spans on the device: every fold step `Match pos v` of runWithCase (reference: src/Data/Text/AhoCorasick/Automaton.hs:442-553) turned into
// (start, len, haystack, needle) the way makeMatch does it (src/Data/Text/AhoCorasick/Replacer.hs:264-274), over the sorted records a scan has left in HBM.
//
// EXPAND (both modes): one lane per record counts its values < n_needles, am_scan.hip turns the counts into offsets, a second pass writes the spans in fold order
// (records ascend by (haystack, end), the values of a record come in list order).  Natural text carries 1.25 values per record: a lane per record is the right shape.
// IgnoreCase walks len_code_points - 1 code points backwards from the last byte of the match (src/Data/Text/Utf8.hs:256-276), per value; the walk never leaves the
// haystack (clamped to 0 where the reference calls `error`).
// A table with a WORD CLASS (am_span_table_create_words) keeps the whole-word spans only: both passes decide that with span_of (am_words.h), the count pass counts
// kept rows, and everything below runs on a compact span array as if the other spans had never matched.  A table with SPELLINGS (am_span_table_create_cased) is
// filtered at the same place by the same function: a handle with a spelling is a row only where the text spells it so.
//
// LEFTMOST-LONGEST without a sort, in global byte positions g = offsets[haystack] + start.  Haystacks are contiguous and len > 0 implies g < total, so ascending g is
// ascending (haystack, start), and a span of an earlier haystack ends at or before every g of a later one: nothing below needs a haystack comparison.
//   * bit g of a bitmap for every span with len > 0 (atomicOr); popcount per word + exclusive sum = the rank of every distinct start, D of them;
//   * best[rank] = atomicMax(len << 32 | ~needle): the longest span of that start, then the smallest handle.  Integer max and or do not depend on arrival order: the
//     result is bit-identical from run to run;
//   * a pass over the bitmap words writes the D CANDIDATES' positions in ascending g (the rank is the sort);
//   * candidate i is a HEAD when g_i >= the maximum end of all candidates before it (an exclusive prefix maximum).  A head is always kept:
//       (1) the cursor is 0 at the start of a haystack or the end of a kept candidate before i, so cursor <= max end before i <= g_i whenever the selection is before g_i;
//       (2) the selection takes the smallest start >= cursor, which is <= g_i because g_i qualifies, and no candidate before i ends beyond g_i, so it cannot step over g_i;
//       (3) hence it arrives at start g_i exactly, where candidate i is the longest span with the smallest handle.
//     What happens before a head has no influence on what happens from it on: the CHAINS between heads are independent;
//   * inside a chain the kept candidates are head, next[head], ... with next[i] = the first candidate with g >= g_i + len_i: the chain selector of am_chain.h;
//   * kept flags -> exclusive sum -> the spans, and per haystack the index of its first one.
// All indices are 64-bit.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "am_bounds.h"
#include "am_device.h"
#include "am_records.h"
#include "am_wave.h"
#include "am_words.h"

AM_BOUNDS_TU("am_spans.hip")

namespace am {
namespace dev {

namespace {

// (kSpThreads, the lanes of a workgroup of the prefix maximum: am_device.h, beside kSpansMaxTile)
constexpr uint32_t kSpMaxPer = (uint32_t)(kSpansMaxTile / kSpThreads);      // candidates per lane of the prefix maximum

// one lane per record (+ one for the trailing zero of the scan's input): its values < n_needles; WORDS / EXACT: those the word class and the spellings keep (span_of,
// am_words.h -- under IC the backwards walk runs here and again in k_spans_write: no span that is dropped is ever written)
template <bool IC, bool WORDS, bool EXACT>
__global__ void __launch_bounds__(kRowThreads) k_spans_count(SpansIn in, uint32_t* __restrict__ cnt)
{
    const uint64_t i = global_row();
    if (i > in.n_rec) return;
    if (i == in.n_rec) { cnt[i] = 0; return; }
    const Record r = in.recs[i];
    uint64_t v0, v1;
    value_range(in, r, v0, v1);
    uint32_t c = 0;
    for (uint64_t k = v0; k < v1; k++) {
        const uint32_t v = in.vals[k];
        if (!WORDS && !EXACT) { c += v < in.n_needles ? 1u : 0u; continue; }
        if (v >= in.n_needles) continue;
        uint64_t s, n;
        c += span_of<IC, WORDS, EXACT>(in, r, v, in.words, s, n) ? 1u : 0u;
    }
    cnt[i] = c;
}

// one lane per record: its spans, in list order, at voff[i]
template <bool IC, bool WORDS, bool EXACT>
__global__ void __launch_bounds__(kRowThreads) k_spans_write(SpansIn in, const uint64_t* __restrict__ voff, Span* __restrict__ spans, uint64_t n_span)
{
    const uint64_t i = global_row();
    if (i >= in.n_rec) return;
    const Record r = in.recs[i];
    if (i > 0) {
        const Record p = in.recs[i - 1];
        AM_BOUNDS(p.haystack < r.haystack || (p.haystack == r.haystack && p.end_pos < r.end_pos));       // sorted by (haystack, end)
    }
    uint64_t v0, v1;
    value_range(in, r, v0, v1);
    uint64_t o = voff[i];
    for (uint64_t k = v0; k < v1; k++) {
        const uint32_t v = in.vals[k];
        if (v >= in.n_needles) continue;                               // the am_needle_ids convention: skipped
        uint64_t s, n;
        if (!span_of<IC, WORDS, EXACT>(in, r, v, in.words, s, n)) continue;      // (a predicate only: not kept, no row -- voff counted the kept ones)
        AM_BOUNDS(o < n_span && o < voff[i + 1] && s <= r.end_pos);
        if (o >= n_span) return;
        Span x;
        x.start = s; x.len = n; x.haystack = r.haystack; x.needle = v;
        spans[o++] = x;
    }
}

// one lane per haystack (+ one for the end): the index of its first span
__global__ void __launch_bounds__(kRowThreads) k_spans_offsets(const uint64_t* __restrict__ rec_first, const uint64_t* __restrict__ voff, uint64_t n_rec, uint32_t n_hay,
                                                              uint64_t* __restrict__ span_off)
{
    const uint64_t h = global_row();
    if (h > n_hay) return;
    const uint64_t r0 = rec_first[h];
    AM_BOUNDS(r0 <= n_rec);
    span_off[h] = voff[r0 <= n_rec ? r0 : n_rec];
}

// ---- leftmost-longest

// the global position of a span with len > 0; false when it does not lie inside the text
__device__ __forceinline__ bool span_global(const SpansIn& in, const Span& x, uint64_t& g)
{
    AM_BOUNDS(x.haystack < in.n_hay);
    if (x.haystack >= in.n_hay) return false;
    g = in.offsets[x.haystack] + x.start;
    AM_BOUNDS(g < in.total && g + x.len <= in.total);
    return g < in.total;
}

__global__ void __launch_bounds__(kRowThreads) k_spans_mark(const Span* __restrict__ spans, uint64_t n_span, SpansIn in, uint32_t* __restrict__ bits, uint64_t n_words)
{
    const uint64_t i = global_row();
    if (i >= n_span) return;
    const Span x = spans[i];
    uint64_t g;
    if (x.len == 0 || !span_global(in, x, g)) return;                  // zero-length spans are never selected
    AM_BOUNDS((g >> 5) < n_words);
    if ((g >> 5) >= n_words) return;
    atomicOr(&bits[g >> 5], 1u << (g & 31u));
}

__global__ void __launch_bounds__(kRowThreads) k_spans_popcount(const uint32_t* __restrict__ bits, uint64_t n_words, uint32_t* __restrict__ pc)
{
    const uint64_t w = global_row();
    if (w > n_words) return;
    pc[w] = w < n_words ? (uint32_t)__popc(bits[w]) : 0u;
}

__global__ void __launch_bounds__(kRowThreads) k_spans_best(const Span* __restrict__ spans, uint64_t n_span, SpansIn in, const uint32_t* __restrict__ bits,
                                                           const uint64_t* __restrict__ rank, uint64_t n_words, uint64_t* __restrict__ best, uint64_t n_cand)
{
    const uint64_t i = global_row();
    if (i >= n_span) return;
    const Span x = spans[i];
    uint64_t g;
    if (x.len == 0 || !span_global(in, x, g)) return;
    const uint64_t w = g >> 5;
    AM_BOUNDS(w < n_words);
    if (w >= n_words) return;
    const uint32_t word = bits[w], bit = (uint32_t)(g & 31u);
    const uint64_t k = rank[w] + (uint64_t)__popc(word & ((1u << bit) - 1u));
    AM_BOUNDS(((word >> bit) & 1u) != 0 && k < n_cand && x.len < (1ull << 32));
    if (k >= n_cand) return;
    atomicMax((unsigned long long*)&best[k], (unsigned long long)((x.len << 32) | (uint64_t)(~x.needle)));
}

// one lane per bitmap word: the positions of its set bits, ascending, from rank[w] on
__global__ void __launch_bounds__(kRowThreads) k_spans_candidates(const uint32_t* __restrict__ bits, const uint64_t* __restrict__ rank, uint64_t n_words,
                                                                 uint64_t* __restrict__ cand_g, uint64_t n_cand)
{
    const uint64_t w = global_row();
    if (w >= n_words) return;
    uint32_t m = bits[w];
    uint64_t k = rank[w];
    while (m) {
        const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
        AM_BOUNDS(k < n_cand && k < rank[w + 1]);
        if (k >= n_cand) return;
        cand_g[k++] = (w << 5) + b;
        m &= m - 1u;
    }
}

__device__ __forceinline__ uint64_t cand_end(const uint64_t* __restrict__ cand_g, const uint64_t* __restrict__ best, uint64_t i) { return cand_g[i] + (best[i] >> 32); }

__device__ __forceinline__ uint64_t wave_incl_max(uint64_t x, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint64_t y = __shfl_up(x, d, 64); if (lane >= (uint32_t)d && y > x) x = y; }
    return x;
}

// exclusive maximum over the workgroup's 256 values (0 before the first); *total = the workgroup's maximum
__device__ __forceinline__ uint64_t block_exclusive_max(uint64_t v, uint64_t* total)
{
    __shared__ uint64_t wmax[kSpThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t incl = wave_incl_max(v, lane);
    uint64_t prev = __shfl_up(incl, 1, 64);
    if (lane == 0) prev = 0;
    __syncthreads();                                         // (wmax may still be read by the previous call's last phase)
    if (lane == 63u) wmax[w] = incl;
    __syncthreads();
    uint64_t all = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSpThreads / 64; k++) { if (k < w) prev = std::max(prev, wmax[k]); all = std::max(all, wmax[k]); }
    *total = all;
    return prev;
}

// the maximum end of every tile of kSpansMaxTile candidates
__global__ void __launch_bounds__(kSpThreads) k_spans_tile_max(const uint64_t* __restrict__ cand_g, const uint64_t* __restrict__ best, uint64_t n_cand,
                                                               uint64_t* __restrict__ tile_max)
{
    const uint64_t i0 = (uint64_t)blockIdx.x * kSpansMaxTile + (uint64_t)threadIdx.x * kSpMaxPer;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSpMaxPer; k++) if (i0 + k < n_cand) v = std::max(v, cand_end(cand_g, best, i0 + k));
    uint64_t total;
    (void)block_exclusive_max(v, &total);
    if (threadIdx.x == 0) tile_max[blockIdx.x] = total;
}

// one workgroup: tile_max[0 .. nt) -> their exclusive prefix maxima, in place
__global__ void __launch_bounds__(kSpThreads) k_spans_tiles_max(uint64_t* __restrict__ tile_max, uint64_t nt)
{
    uint64_t carry = 0;
    for (uint64_t i0 = 0; i0 < nt; i0 += kSpThreads) {
        const uint64_t i = i0 + threadIdx.x;
        const uint64_t v = i < nt ? tile_max[i] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive_max(v, &total);
        if (i < nt) tile_max[i] = std::max(carry, ex);
        carry = std::max(carry, total);
    }
}

// head[i] = g_i >= the maximum end of all candidates before i; kept = head (n_cand + 1 entries, the last one 0: the scan's trailing element)
__global__ void __launch_bounds__(kSpThreads) k_spans_heads(const uint64_t* __restrict__ cand_g, const uint64_t* __restrict__ best, uint64_t n_cand,
                                                            const uint64_t* __restrict__ tile_base, uint8_t* __restrict__ head, uint32_t* __restrict__ kept)
{
    const uint64_t i0 = (uint64_t)blockIdx.x * kSpansMaxTile + (uint64_t)threadIdx.x * kSpMaxPer;
    uint64_t g[kSpMaxPer], e[kSpMaxPer], v = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSpMaxPer; k++) {
        g[k] = e[k] = 0;
        if (i0 + k < n_cand) { g[k] = cand_g[i0 + k]; e[k] = g[k] + (best[i0 + k] >> 32); AM_BOUNDS(e[k] > g[k]); }
        v = std::max(v, e[k]);
    }
    uint64_t total;
    uint64_t run = std::max(tile_base[blockIdx.x], block_exclusive_max(v, &total));
#pragma unroll
    for (uint32_t k = 0; k < kSpMaxPer; k++) {
        const uint64_t i = i0 + k;
        if (i < n_cand) {
            const bool h = g[k] >= run;
            AM_BOUNDS(i > 0 || h);
            head[i] = h ? 1 : 0;
            kept[i] = h ? 1u : 0u;
            run = std::max(run, e[k]);
        } else if (i == n_cand) {
            kept[i] = 0;
        }
    }
}

// one lane per candidate: a kept one becomes a span of the haystack its position lies in
__global__ void __launch_bounds__(kRowThreads) k_spans_emit(const uint64_t* __restrict__ cand_g, const uint64_t* __restrict__ best, const uint32_t* __restrict__ kept,
                                                           const uint64_t* __restrict__ kidx, uint64_t n_cand, SpansIn in, Span* __restrict__ out, uint64_t n_out)
{
    const uint64_t i = global_row();
    if (i >= n_cand || !kept[i]) return;
    const uint64_t g = cand_g[i], b = best[i];
    const uint64_t lo = last_at_or_before(in.offsets, (uint64_t)0, (uint64_t)in.n_hay - 1, g);      // offsets[lo] <= g < offsets[lo + 1]: the haystack that owns byte g
    const uint64_t o = kidx[i];
    AM_BOUNDS(o < n_out && in.offsets[lo] <= g && g + (b >> 32) <= in.offsets[lo + 1]);
    if (o >= n_out) return;
    Span x;
    x.start = g - in.offsets[lo]; x.len = b >> 32; x.haystack = (uint32_t)lo; x.needle = ~(uint32_t)b;
    out[o] = x;
}

// one lane per haystack (+ one for the end): the index of its first kept span = kidx of the first candidate at or after its first byte
__global__ void __launch_bounds__(kRowThreads) k_spans_ll_offsets(const uint64_t* __restrict__ cand_g, const uint64_t* __restrict__ kidx, uint64_t n_cand, SpansIn in,
                                                                 uint64_t* __restrict__ span_off, uint64_t n_out)
{
    const uint64_t h = global_row();
    if (h > in.n_hay) return;
    const uint64_t at = in.offsets[h];
    uint64_t lo = 0, hi = n_cand;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (cand_g[mid] < at) lo = mid + 1; else hi = mid; }
    AM_BOUNDS(lo <= n_cand && kidx[lo] <= n_out && (h < in.n_hay || kidx[lo] == n_out));
    span_off[h] = kidx[lo];
}

}  // namespace

hipError_t launch_spans_count(bool ic, const SpansIn& in, uint32_t* cnt, hipStream_t st)
{
    // (no predicate: the count needs no start, so no case mode)
    const auto kernel = in.exact ? (in.words ? (ic ? k_spans_count<true, true, true> : k_spans_count<false, true, true>) : (ic ? k_spans_count<true, false, true> : k_spans_count<false, false, true>))
                                 : !in.words ? k_spans_count<false, false, false> : ic ? k_spans_count<true, true, false> : k_spans_count<false, true, false>;
    return launch_rows(kernel, in.n_rec + 1, st, in, cnt);
}

hipError_t launch_spans_write(bool ic, const SpansIn& in, const uint64_t* voff, Span* spans, uint64_t n_span, hipStream_t st)
{
    if (n_span == 0) return hipSuccess;
    const auto kernel = in.exact ? (in.words ? (ic ? k_spans_write<true, true, true> : k_spans_write<false, true, true>) : (ic ? k_spans_write<true, false, true> : k_spans_write<false, false, true>))
                                 : in.words ? (ic ? k_spans_write<true, true, false> : k_spans_write<false, true, false>) : (ic ? k_spans_write<true, false, false> : k_spans_write<false, false, false>);
    return launch_rows(kernel, in.n_rec, st, in, voff, spans, n_span);
}

hipError_t launch_spans_offsets(const uint64_t* rec_first, const uint64_t* voff, uint64_t n_rec, uint32_t n_hay, uint64_t* span_off, hipStream_t st)
{
    return launch_rows(k_spans_offsets, (uint64_t)n_hay + 1, st, rec_first, voff, n_rec, n_hay, span_off);
}

hipError_t launch_spans_mark(const Span* spans, uint64_t n_span, const SpansIn& in, uint32_t* bits, uint64_t n_words, hipStream_t st)
{
    return launch_rows(k_spans_mark, n_span, st, spans, n_span, in, bits, n_words);
}

hipError_t launch_spans_popcount(const uint32_t* bits, uint64_t n_words, uint32_t* pc, hipStream_t st)
{
    return launch_rows(k_spans_popcount, n_words + 1, st, bits, n_words, pc);
}

hipError_t launch_spans_best(const Span* spans, uint64_t n_span, const SpansIn& in, const uint32_t* bits, const uint64_t* rank, uint64_t n_words, uint64_t* best, uint64_t n_cand,
                             hipStream_t st)
{
    return launch_rows(k_spans_best, n_span, st, spans, n_span, in, bits, rank, n_words, best, n_cand);
}

hipError_t launch_spans_candidates(const uint32_t* bits, const uint64_t* rank, uint64_t n_words, uint64_t* cand_g, uint64_t n_cand, hipStream_t st)
{
    return launch_rows(k_spans_candidates, n_words, st, bits, rank, n_words, cand_g, n_cand);
}

hipError_t launch_spans_heads(const uint64_t* cand_g, const uint64_t* best, uint64_t n_cand, uint64_t* tile_max, uint8_t* head, uint32_t* kept, hipStream_t st)
{
    const uint64_t nt = (n_cand + 1 + kSpansMaxTile - 1) / kSpansMaxTile;      // (+ 1: the tile that holds kept's trailing element)
    if (nt > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_spans_tile_max, dim3((uint32_t)nt), dim3(kSpThreads), 0, st, cand_g, best, n_cand, tile_max);
    hipLaunchKernelGGL(k_spans_tiles_max, dim3(1), dim3(kSpThreads), 0, st, tile_max, nt);
    hipLaunchKernelGGL(k_spans_heads, dim3((uint32_t)nt), dim3(kSpThreads), 0, st, cand_g, best, n_cand, (const uint64_t*)tile_max, head, kept);
    return hipGetLastError();
}

hipError_t launch_spans_emit(const uint64_t* cand_g, const uint64_t* best, const uint32_t* kept, const uint64_t* kidx, uint64_t n_cand, const SpansIn& in, Span* out, uint64_t n_out,
                             uint64_t* span_off, hipStream_t st)
{
    const hipError_t e = launch_rows(k_spans_emit, in.n_hay ? n_cand : 0, st, cand_g, best, kept, kidx, n_cand, in, out, n_out);
    return e != hipSuccess ? e : launch_rows(k_spans_ll_offsets, (uint64_t)in.n_hay + 1, st, cand_g, kidx, n_cand, in, span_off, n_out);
}

}  // namespace dev
}  // namespace am
