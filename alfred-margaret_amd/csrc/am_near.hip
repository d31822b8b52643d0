// am_near.hip -- proximity on the device (include/am.h "proximity"): for every span of a group A of an AM_SPANS_LEFTMOST_LONGEST result, the nearest other span of a
// group B in the same haystack, a pair where the gap between the two is at most max_gap bytes; per query the haystacks with a pair as a bitmap, and the pair counts.
// Up to 64 queries over up to 32 groups from one spans result.  The join needs no sort, no atomic per pair and no lane loop whose trip count depends on the text:
// the gap is bounded in BYTES, so a lane that walked its neighbours until it left the window would walk as far as the text lets it.  Instead:
//
//   k_near_bits   one lane per span, 64 consecutive spans per wavefront: the ballot of "span i is in group g" IS word i / 64 of the group's bitmap row -- one 8-byte
//                 store per wavefront and group a query names, no atomics.  The needle -> mask table is staged in LDS where it fits (kNearLdsNeedles), read in
//                 HBM otherwise (a dictionary of 100 000 words: 400 KB, L2-resident).
//   k_near_words  per row and direction ONE workgroup walks the words in sweeps of kNearSweepWords with a carry and writes, for every word, the last non-zero word
//                 before it (prev_nz) or the first non-zero word behind it (next_nz): an exclusive running maximum (near_link_value, am_near.h), the wavefronts'
//                 maxima combined through LDS.  The sweeps of a row are sequential -- 2 x rows workgroups at work, each over n_span / 64 words: not tuned, see
//                 DESIGN 7.11 for what it costs.
//   k_near_count  one lane per span.  For each query whose group_a the span is in: p and n by near_prev / near_next (the lane's own word by bit arithmetic, else
//                 the linked word's highest / lowest bit), two loads of {start, len, haystack}, near_pick.  The queries that hit go into a 64-bit mask per span,
//                 their number into the array the library's exclusive sum (am_scan.hip) turns into the pairs' places.  `fired`: where the 64 spans of a wavefront
//                 share a haystack, ONE 64-bit atomic OR per query with a hit; otherwise one per run of hits in one haystack; none where the bit is seen set already (a
//                 document of a million spans would send every wavefront to one word).  ORs commute: bit-identical.
//   k_near_emit   one lane per span again: the same pick for the queries of its mask, each pair written at pos[i] + (the mask's bits below q): rows ascend by
//                 (haystack, a, query) because the spans do.  out_off[h] = pos[span_off[h]].  counts: popcount(ballot) per wavefront and query into LDS, one
//                 64-bit global add per workgroup and query that hit.
// The loops over the queries have a wave-uniform trip count (n_queries) and skip a query none of the 64 lanes takes part in by a ballot.  Plain C++ and vector
// stores only.  LDS: 32 KiB of masks in k_near_bits<true>, 512 B of counters in k_near_emit, 64 B in k_near_words.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "am_bounds.h"
#include "am_device.h"
#include "am_near.h"
#include "am_wave.h"

AM_BOUNDS_TU("am_near.hip")

namespace am {
namespace dev {

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kNearThreads = 256;
constexpr uint32_t kNearTile = kNearThreads;                // spans per workgroup step: a lane per span
// (kNearLdsNeedles, the masks k_near_bits stages in LDS: am_near.h)
constexpr uint32_t kNearWordsPerThread = 4;
constexpr uint32_t kNearSweepWords = kNearThreads * kNearWordsPerThread;      // words per sweep of k_near_words = 4 x tile_spans (am_near_geometry)
constexpr int kNearGroupsPerCu = 8;
constexpr uint32_t kNoHay = 0xFFFFFFFFu;

template <bool STAGED>
__global__ void __launch_bounds__(kNearThreads) k_near_bits(NearIn in)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t near_masks[];
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1);
    if (STAGED) {
        AM_BOUNDS(in.n_needles <= kNearLdsNeedles);
        for (uint32_t v = t; v < in.n_needles; v += kNearThreads) near_masks[v] = in.group_mask[v];
        __syncthreads();
    }
    const uint64_t n_tiles = (in.n_span + kNearTile - 1) / kNearTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = tile * kNearTile + t;
        uint32_t m = 0;
        if (i < in.n_span) {
            const uint32_t v = in.spans[i].needle;
            AM_BOUNDS(v < in.n_needles);
            if (v < in.n_needles) m = STAGED ? near_masks[v] : in.group_mask[v];
        }
        const uint64_t w = i / kWave;                       // (wave-uniform: a wavefront's 64 spans are one word)
        if (w >= in.n_words) continue;
        uint32_t row = 0;
        for (uint32_t g = 0; g < kNearMaxGroups; g++) {
            if ((in.plan.used >> g & 1u) == 0) continue;
            const uint64_t word = __ballot((m >> g & 1u) != 0);      // (lanes beyond the spans hold 0: the bits beyond n_span are zero)
            AM_BOUNDS(row < in.plan.n_rows);
            if (lane == 0) in.bits[(uint64_t)row * in.n_words + w] = word;
            row++;
        }
    }
}

// blockIdx.x = 2 * row + direction (0: prev_nz, forwards; 1: next_nz, backwards)
__global__ void __launch_bounds__(kNearThreads) k_near_words(NearIn in)
{
    __shared__ uint32_t wave_max[kNearThreads / kWave];
    const uint32_t row = blockIdx.x >> 1;
    const bool backwards = (blockIdx.x & 1u) != 0;
    AM_BOUNDS(row < in.plan.n_rows);
    const uint64_t* __restrict__ bits = in.bits + (uint64_t)row * in.n_words;
    uint32_t* __restrict__ link = (backwards ? in.next_nz : in.prev_nz) + (uint64_t)row * in.n_words;
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    uint32_t carry = 0;                                     // the maximum of every sweep before this one
    for (uint32_t s0 = 0; s0 < in.n_words; s0 += kNearSweepWords) {
        uint32_t v[kNearWordsPerThread], mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < kNearWordsPerThread; k++) {
            const uint32_t step = s0 + t * kNearWordsPerThread + k;
            v[k] = 0;
            if (step < in.n_words) {
                const uint32_t w = near_link_index(step, backwards, in.n_words);
                AM_BOUNDS(w < in.n_words);
                v[k] = near_link_value(bits[w], step);
            }
            mine = v[k] > mine ? v[k] : mine;
        }
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(incl, d, 64); if (lane >= (uint32_t)d && y > incl) incl = y; }
        __syncthreads();                                    // (the last sweep's readers have finished)
        if (lane == kWave - 1) wave_max[wv] = incl;
        __syncthreads();
        uint32_t before = carry, all = carry;
#pragma unroll
        for (uint32_t k = 0; k < kNearThreads / kWave; k++) {
            const uint32_t x = wave_max[k];
            if (k < wv && x > before) before = x;
            if (x > all) all = x;
        }
        const uint32_t left = __shfl_up(incl, 1, 64);       // the lanes before this one, in its wavefront
        uint32_t run = lane != 0 && left > before ? left : before;
#pragma unroll
        for (uint32_t k = 0; k < kNearWordsPerThread; k++) {
            const uint32_t step = s0 + t * kNearWordsPerThread + k;
            if (step < in.n_words) link[near_link_index(step, backwards, in.n_words)] = near_link_word(run, backwards, in.n_words);
            run = v[k] > run ? v[k] : run;
        }
        carry = all;
    }
}

// the two candidates of anchor i for a query and the pick between them
__device__ __forceinline__ NearPicked near_find(const NearIn& in, uint64_t i, const Span& a, const NearQueryDev& q)
{
    AM_BOUNDS(q.row_b < in.plan.n_rows && i < in.n_span);
    const uint64_t* __restrict__ row = in.bits + (uint64_t)q.row_b * in.n_words;
    NearSide p{false, 0, 0, 0, 0}, n{false, 0, 0, 0, 0};
    if ((q.flags & kNearOrdered) == 0) {
        const uint64_t j = near_prev(row, in.prev_nz + (uint64_t)q.row_b * in.n_words, i);
        AM_BOUNDS(j == kNearNone || j < i);
        if (j != kNearNone && j < in.n_span) { const Span s = in.spans[j]; p = NearSide{true, j, s.start, s.len, s.haystack}; }
    }
    {
        const uint64_t j = near_next(row, in.next_nz + (uint64_t)q.row_b * in.n_words, i);
        AM_BOUNDS(j == kNearNone || (j > i && j < in.n_span));
        if (j != kNearNone && j < in.n_span) { const Span s = in.spans[j]; n = NearSide{true, j, s.start, s.len, s.haystack}; }
    }
    return near_pick(a.start, a.len, a.haystack, p, n, q.flags, q.max_gap);
}

__device__ __forceinline__ uint32_t mask_of(const NearIn& in, const Span& a)
{
    AM_BOUNDS(a.needle < in.n_needles);
    return a.needle < in.n_needles ? in.group_mask[a.needle] : 0u;
}

// a word of `fired` that other wavefronts OR into at the same time: a relaxed atomic load (a stale value costs an OR, never a bit)
__device__ __forceinline__ unsigned long long fired_word(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(kNearThreads) k_near_count(NearIn in)
{
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1);
    const uint64_t n_tiles = (in.n_span + kNearTile - 1) / kNearTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = tile * kNearTile + t;
        const bool active = i < in.n_span;
        Span a{0, 0, kNoHay, 0};
        uint32_t m = 0;
        if (active) { a = in.spans[i]; m = mask_of(in, a); }
        if (__ballot(active) == 0) continue;
        AM_BOUNDS(!active || a.haystack < in.n_hay);
        const uint32_t h0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.haystack);      // (lane 0 is active wherever a lane is)
        const bool one_haystack = __ballot(active && a.haystack != h0) == 0;
        uint64_t mask = 0;
        for (uint32_t q = 0; q < in.plan.n_queries; q++) {
            const NearQueryDev Q = in.dq[q];
            const bool in_a = active && (m >> Q.bit_a & 1u) != 0;
            if (__ballot(in_a) == 0) continue;
            bool hit = false;
            if (in_a) hit = near_find(in, i, a, Q).hit && a.haystack < in.n_hay;
            const uint64_t hits = __ballot(hit);
            if (hits == 0) continue;
            if (hit) mask |= 1ull << q;
            unsigned long long* const frow = (unsigned long long*)in.fired + (uint64_t)q * in.hay_words;
            if (one_haystack) {
                AM_BOUNDS(h0 / 64 < in.hay_words);
                if (lane == 0 && (fired_word(&frow[h0 / 64]) >> (h0 % 64) & 1ull) == 0) atomicOr(&frow[h0 / 64], 1ull << (h0 % 64));      // (a set bit stays set: a stale read costs an OR, never a bit)
            } else {
                const uint32_t left = __shfl_up(hit ? a.haystack : kNoHay, 1, 64);
                if (hit && (lane == 0 || left != a.haystack)) {      // the first hit of a run of hits in one haystack
                    AM_BOUNDS(a.haystack / 64 < in.hay_words);
                    if ((fired_word(&frow[a.haystack / 64]) >> (a.haystack % 64) & 1ull) == 0) atomicOr(&frow[a.haystack / 64], 1ull << (a.haystack % 64));
                }
            }
        }
        if (active) { in.hit_mask[i] = mask; in.hit_count[i] = (uint32_t)__popcll(mask); }
    }
}

__global__ void __launch_bounds__(kNearThreads) k_near_emit(NearIn in)
{
    __shared__ unsigned long long cnt[kNearMaxQueries];
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1);
    if (t < kNearMaxQueries) cnt[t] = 0;
    __syncthreads();
    for (uint64_t h = (uint64_t)blockIdx.x * kNearThreads + t; h <= in.n_hay; h += (uint64_t)gridDim.x * kNearThreads) {
        const uint64_t s = in.span_off[h];
        AM_BOUNDS(s <= in.n_span);
        in.out_off[h] = in.pos[s <= in.n_span ? s : in.n_span];
    }
    const uint64_t n_tiles = (in.n_span + kNearTile - 1) / kNearTile;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = tile * kNearTile + t;
        const bool active = i < in.n_span;
        const uint64_t mask = active ? in.hit_mask[i] : 0;
        if (__ballot(mask != 0) == 0) continue;
        Span a{0, 0, kNoHay, 0};
        uint64_t base = 0;
        if (mask != 0) { a = in.spans[i]; base = in.pos[i]; }
        for (uint32_t q = 0; q < in.plan.n_queries; q++) {
            const bool hit = (mask >> q & 1ull) != 0;
            const uint64_t hits = __ballot(hit);
            if (hits == 0) continue;
            if (hit) {
                const NearPicked r = near_find(in, i, a, in.dq[q]);
                const uint64_t at = base + (uint64_t)__popcll(mask & ((1ull << q) - 1ull));
                AM_BOUNDS(r.hit && at < in.n_pairs && at < in.pos[i + 1]);
                if (at < in.n_pairs) in.pairs[at] = NearPair{i, r.b, r.gap, a.haystack, q};
            }
            if (lane == 0) atomicAdd(&cnt[q], (unsigned long long)__popcll(hits));
        }
    }
    __syncthreads();
    if (t < in.plan.n_queries) {
        const unsigned long long k = cnt[t];
        if (k != 0) atomicAdd((unsigned long long*)&in.counts[t], k);
    }
}

uint32_t near_grid(uint64_t n_span, int n_cu)
{
    const uint64_t n_tiles = (n_span + kNearTile - 1) / kNearTile;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_tiles, (uint64_t)std::max(n_cu, 1) * kNearGroupsPerCu));
}

}  // namespace

void near_geometry(uint32_t* tile_spans, uint32_t* word_spans)
{
    if (tile_spans) *tile_spans = kNearTile;
    if (word_spans) *word_spans = kWave;
}

hipError_t launch_near_bits(const NearIn& in, int n_cu, hipStream_t st)
{
    if (in.n_span == 0 || in.plan.n_rows == 0) return hipSuccess;
    const uint32_t grid = near_grid(in.n_span, n_cu);
    if (in.n_needles <= kNearLdsNeedles) hipLaunchKernelGGL(k_near_bits<true>, dim3(grid), dim3(kNearThreads), (size_t)in.n_needles * 4, st, in);
    else hipLaunchKernelGGL(k_near_bits<false>, dim3(grid), dim3(kNearThreads), 0, st, in);
    return hipGetLastError();
}

hipError_t launch_near_words(const NearIn& in, hipStream_t st)
{
    if (in.n_words == 0 || in.plan.n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(k_near_words, dim3(in.plan.n_rows * 2), dim3(kNearThreads), 0, st, in);
    return hipGetLastError();
}

hipError_t launch_near_count(const NearIn& in, int n_cu, hipStream_t st)
{
    if (in.n_span == 0) return hipSuccess;
    hipLaunchKernelGGL(k_near_count, dim3(near_grid(in.n_span, n_cu)), dim3(kNearThreads), 0, st, in);
    return hipGetLastError();
}

hipError_t launch_near_emit(const NearIn& in, int n_cu, hipStream_t st)
{
    hipLaunchKernelGGL(k_near_emit, dim3(near_grid(in.n_span, n_cu)), dim3(kNearThreads), 0, st, in);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace am
