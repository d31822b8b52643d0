// am_split.hip -- Splitter's fold on the device: stepAccum / finalizeAccum (reference: src/Data/Text/AhoCorasick/Splitter.hs:141-170) over the sorted records a scan of
// the one-needle automaton has left in HBM, and the gather that turns the fragments into a batch of their own.
//
// The fold is sequential as written: a match is a separator iff it starts at or after the end of the last separator kept (:163-164).  Heads, chains and pointer
// doubling make it parallel: am_chain.h.  A record is a HEAD when it is the first of its haystack or starts at or after the end of the record before it (the records
// are sorted by end, so every record kept before it ends at or before its start; starts are ordered like ends: every match spans the same number of code points).
//   * kept flags -> exclusive sum -> fragment k of a haystack runs from the end of its kept separator k - 1 (or 0) to the start of kept separator k (or the length).
//     A haystack with m kept separators has m + 1 fragments, so the fragment that ends at kept record i has the global index kidx[i] + haystack(i).
// IgnoreCase: the start of a match is found by walking sep_len_code_points - 1 code points backwards from its last byte (Splitter.hs:117-121, Utf8.hs:256-276); the
// walk reads at most 4 bytes per code point and never leaves the haystack (a walk that would is clamped to 0, where the reference calls `error`).
// All indices are 64-bit.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "am_bounds.h"
#include "am_device.h"
#include "am_wave.h"

AM_BOUNDS_TU("am_split.hip")

namespace am {
namespace dev {

namespace {

constexpr uint32_t kGatherThreads = 256;                                // lanes of a k_split_gather workgroup
constexpr uint32_t kGatherGroup = 16;                                  // bytes a lane of k_split_gather writes with one store
constexpr uint64_t kGatherTile = (uint64_t)kGatherThreads * kGatherGroup;
constexpr int kGatherGroupsPerCu = 8;

// sepStart of the match that record r reports, relative to its haystack (Splitter.hs:105-107 / :117-121)
template <bool IC>
__device__ __forceinline__ uint64_t sep_start(const SplitIn& in, const Record& r)
{
    if (!IC) return r.end_pos >= in.sep_bytes ? r.end_pos - in.sep_bytes : 0;
    AM_BOUNDS(r.haystack < in.n_hay);
    if (r.haystack >= in.n_hay || r.end_pos == 0) return 0;
    const uint64_t base = in.offsets[r.haystack];
    AM_BOUNDS(base + r.end_pos <= in.total);
    if (base + r.end_pos > in.total) return 0;
    const uint8_t* hay = in.text + base;
    return skip_code_points_backwards(hay, r.end_pos, in.sep_cps - 1);
}

// one lane per record (+ one for the trailing zero of the scan's input): start, head, kept = head
template <bool IC>
__global__ void __launch_bounds__(kRowThreads) k_split_start(SplitIn in, uint64_t* __restrict__ start, uint8_t* __restrict__ head, uint32_t* __restrict__ kept)
{
    const uint64_t i = global_row();
    if (i > in.n_rec) return;
    if (i == in.n_rec) { kept[i] = 0; return; }
    const Record r = in.recs[i];
    const uint64_t s = sep_start<IC>(in, r);
    bool h = true;
    if (i > 0) {
        const Record p = in.recs[i - 1];
        AM_BOUNDS(p.haystack < r.haystack || (p.haystack == r.haystack && p.end_pos < r.end_pos));       // sorted by (haystack, end)
        h = p.haystack != r.haystack || s >= p.end_pos;                // (positions are relative to the haystack: the haystack comparison comes first)
    }
    start[i] = s;
    head[i] = h ? 1 : 0;
    kept[i] = h ? 1u : 0u;
}

// one lane per haystack (+ one for the end): its first fragment index; the start of its first fragment and the end of its last
__global__ void __launch_bounds__(kRowThreads) k_split_offsets(SplitIn in, const uint64_t* __restrict__ rec_first, const uint64_t* __restrict__ kidx,
                                                                 uint64_t* __restrict__ frag_off, Fragment* __restrict__ frags, uint64_t n_frag)
{
    const uint64_t h = global_row();
    if (h > in.n_hay) return;
    const uint64_t r0 = rec_first[h];
    AM_BOUNDS(r0 <= in.n_rec);
    const uint64_t o0 = kidx[r0 <= in.n_rec ? r0 : in.n_rec] + h;
    frag_off[h] = o0;
    if (h == in.n_hay) { AM_BOUNDS(o0 == n_frag); return; }
    const uint64_t r1 = rec_first[h + 1];
    const uint64_t o1 = kidx[r1 <= in.n_rec ? r1 : in.n_rec] + h + 1;
    AM_BOUNDS(o0 < o1 && o1 <= n_frag);
    if (o0 >= n_frag || o1 > n_frag || o1 <= o0) return;
    frags[o0].start = 0;
    frags[o1 - 1].len = in.offsets[h + 1] - in.offsets[h];            // (the fragment's END until k_split_lengths has run)
}

// one lane per record: a kept separator ends one fragment and starts the next
__global__ void __launch_bounds__(kRowThreads) k_split_emit(const Record* __restrict__ recs, uint64_t n_rec, const uint64_t* __restrict__ start,
                                                              const uint32_t* __restrict__ kept, const uint64_t* __restrict__ kidx,
                                                              Fragment* __restrict__ frags, uint64_t n_frag)
{
    const uint64_t i = global_row();
    if (i >= n_rec || !kept[i]) return;
    const Record r = recs[i];
    const uint64_t f = kidx[i] + r.haystack;
    AM_BOUNDS(f + 1 < n_frag);
    if (f + 1 >= n_frag) return;
    frags[f].len = start[i];                                           // (its END until k_split_lengths has run)
    frags[f + 1].start = r.end_pos;
}

__global__ void __launch_bounds__(kRowThreads) k_split_lengths(Fragment* __restrict__ frags, uint64_t n_frag)
{
    const uint64_t f = global_row();
    if (f >= n_frag) return;
    Fragment v = frags[f];
    AM_BOUNDS(v.start <= v.len);
    v.len = v.len >= v.start ? v.len - v.start : 0;
    frags[f] = v;
}

// ---- am_batch_from_fragments

// one lane per fragment (+ one for the trailing zero of the scan's input): its length, and where its bytes start in the source batch's text
__global__ void __launch_bounds__(kRowThreads) k_split_sources(const Fragment* __restrict__ frags, uint64_t n_frag, const uint64_t* __restrict__ frag_off,
                                                                 const uint64_t* __restrict__ src_offsets, uint64_t n_hay, uint64_t src_total,
                                                                 uint64_t* __restrict__ lens, uint64_t* __restrict__ src_at)
{
    const uint64_t k = global_row();
    if (k > n_frag) return;
    if (k == n_frag) { lens[k] = 0; return; }
    const Fragment v = frags[k];
    const uint64_t h = last_at_or_before(frag_off, (uint64_t)0, n_hay, k);      // frag_off[h] <= k < frag_off[h + 1]: every haystack has a fragment
    AM_BOUNDS(h < n_hay);
    const uint64_t at = src_offsets[h < n_hay ? h : 0] + v.start;
    AM_BOUNDS(at + v.len <= src_total);
    const bool ok = h < n_hay && at + v.len <= src_total;
    lens[k] = ok ? v.len : 0;
    src_at[k] = ok ? at : 0;
}

// 16 source bytes from any address with five aligned dword loads (the text is readable to the next multiple of 16 beyond its end)
__device__ __forceinline__ uint4 load16_unaligned(const uint8_t* __restrict__ text, uint64_t at)
{
    const uint32_t a = (uint32_t)(at & 3u);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(text + (at - a));
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    if (a == 0) return make_uint4(w0, w1, w2, w3);
    const uint32_t w4 = w[4];
    return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, a), __builtin_amdgcn_alignbyte(w2, w1, a), __builtin_amdgcn_alignbyte(w3, w2, a), __builtin_amdgcn_alignbyte(w4, w3, a));
}

// persistent grid over tiles of the NEW text: every lane owns 16 destination bytes (one aligned 16-byte store), finds the fragment its first byte belongs to --
// between the fragments of the tile's first and last byte, which two lanes look up for the workgroup -- and reads the source wherever it lies.  Fragments of
// length 0 own no byte and are never found.  Bytes beyond the end of the text are written as zeros.
__global__ void __launch_bounds__(kGatherThreads) k_split_gather(const uint8_t* __restrict__ src, uint64_t src_total, const uint64_t* __restrict__ src_at,
                                                                const uint64_t* __restrict__ dst_off, uint64_t n_frag, uint64_t total, uint8_t* __restrict__ dst)
{
    __shared__ uint64_t tile_frag[2];
    const uint64_t n_tiles = (total + kGatherTile - 1) / kGatherTile;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {      // (the same tiles for every lane of the workgroup: the barriers are uniform)
        const uint64_t t0 = t * kGatherTile, t1 = std::min<uint64_t>(total, t0 + kGatherTile) - 1;
        __syncthreads();
        if (threadIdx.x < 2) tile_frag[threadIdx.x] = last_at_or_before(dst_off, (uint64_t)0, n_frag - 1, threadIdx.x == 0 ? t0 : t1);
        __syncthreads();
        const uint64_t d = t0 + (uint64_t)threadIdx.x * kGatherGroup;
        if (d >= total) continue;
        uint64_t f = last_at_or_before(dst_off, tile_frag[0], tile_frag[1], d);
        AM_BOUNDS(f < n_frag && dst_off[f] <= d && d < dst_off[f + 1]);
        uint64_t f_end = dst_off[f + 1];
        uint4 v;
        if (d + kGatherGroup <= f_end) {
            const uint64_t at = src_at[f] + (d - dst_off[f]);
            AM_BOUNDS(at + kGatherGroup <= src_total);
            v = at + kGatherGroup <= src_total ? load16_unaligned(src, at) : make_uint4(0, 0, 0, 0);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            uint64_t at = src_at[f] + (d - dst_off[f]);
            for (uint32_t k = 0; k < kGatherGroup && d + k < total; k++) {
                while (d + k >= f_end) {                               // (ends before n_frag: d + k < total = dst_off[n_frag])
                    f++;
                    AM_BOUNDS(f < n_frag);
                    if (f >= n_frag) break;
                    f_end = dst_off[f + 1];
                    at = src_at[f];
                }
                if (f >= n_frag) break;
                AM_BOUNDS(at < src_total);
                const uint32_t byte = at < src_total ? src[at] : 0u;
                at++;
                w[k >> 2] |= byte << (8 * (k & 3));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(dst + d) = v;
    }
}

}  // namespace

uint32_t split_gather_tile_bytes() { return (uint32_t)kGatherTile; }

hipError_t launch_split_start(bool ic, const SplitIn& in, uint64_t* start, uint8_t* head, uint32_t* kept, hipStream_t st)
{
    return launch_rows(ic ? k_split_start<true> : k_split_start<false>, in.n_rec + 1, st, in, start, head, kept);
}

hipError_t launch_split_emit(const SplitIn& in, const uint64_t* start, const uint32_t* kept, const uint64_t* kidx, const uint64_t* rec_first, uint64_t* frag_off,
                             Fragment* frags, uint64_t n_frag, hipStream_t st)
{
    hipError_t e = launch_rows(k_split_offsets, (uint64_t)in.n_hay + 1, st, in, rec_first, kidx, frag_off, frags, n_frag);
    if (e == hipSuccess) e = launch_rows(k_split_emit, in.n_rec, st, in.recs, in.n_rec, start, kept, kidx, frags, n_frag);
    if (e == hipSuccess) e = launch_rows(k_split_lengths, n_frag, st, frags, n_frag);
    return e;
}

hipError_t launch_split_sources(const Fragment* frags, uint64_t n_frag, const uint64_t* frag_off, const uint64_t* src_offsets, uint64_t n_hay, uint64_t src_total,
                                uint64_t* lens, uint64_t* src_at, hipStream_t st)
{
    return launch_rows(k_split_sources, n_frag + 1, st, frags, n_frag, frag_off, src_offsets, n_hay, src_total, lens, src_at);
}

hipError_t launch_split_gather(const uint8_t* src, uint64_t src_total, const uint64_t* src_at, const uint64_t* dst_off, uint64_t n_frag, uint64_t total, uint8_t* dst,
                               int n_cu, hipStream_t st)
{
    if (total == 0 || n_frag == 0) return hipSuccess;
    const uint64_t n_tiles = (total + kGatherTile - 1) / kGatherTile;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)(n_cu > 0 ? n_cu : 1) * kGatherGroupsPerCu);
    hipLaunchKernelGGL(k_split_gather, dim3(grid), dim3(kGatherThreads), 0, st, src, src_total, src_at, dst_off, n_frag, total, dst);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace am
