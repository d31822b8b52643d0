// am_postings.hip -- postings on the device (include/am.h "postings"): the rows of a spans result ordered by needle -- a stable least-significant-digit radix sort
// over (needle handle, row index) pairs in HBM -- with the row offsets per needle, the document frequencies and the per-haystack offsets of one needle's row.  The
// plan (passes, bits per pass, the digit of a key, the cell of the count table) is am_postings.h's, shared with the host.  Plain launches only: no kernel here waits
// for, or spins on, memory another workgroup writes.
//
//   k_post_keys         one lane per span: the needle column (4 of every 24 bytes, strided) into a compact key array, and the identity index array.  The one pass
//                       over the wide rows before the final gather.
//   k_post_hist         one workgroup per tile of kPostTileSpans keys: the tile's count per digit value in a 2^bits-entry LDS table (LDS atomic adds: a count does
//                       not depend on their order), then cell (d, tile) of the digit-major table for every d.  launch_scan (am_scan.hip) over the table gives the
//                       bases.
//   k_post_scatter      one workgroup per tile, four wavefronts, each owning kPostWaveSpans CONSECUTIVE keys.  Sweep 1: every wavefront counts its own portion per
//                       digit into its own LDS row (atomic adds, counts again).  Then its running counters start at base[d][tile] + the counts of the wavefronts before
//                       it.  Sweep 2, 64 consecutive keys per round: the lanes that hold the same digit find each other with one ballot per digit bit (match-any),
//                       a lane's rank is popcount(peers & lanes below), dest = counter[digit] + rank, and the LAST peer bumps the counter with a plain store.  The
//                       order of the output is decided by lane numbers and round numbers alone: stable, and the same on every run.
//   k_post_gather       one lane per posting: three 8-byte loads of S.data[idx[k]], three 8-byte stores, and idx[k] widened into source[k].
//   k_post_offsets      one lane per v in 0 .. N: a lower-bound search over the sorted keys.
//   k_post_df           one lane per posting: head = first of its needle or another haystack than the posting before it.  Needle runs are contiguous, so the first
//                       lane of every needle run inside a wavefront counts the heads of its run from one ballot and adds them with ONE 64-bit atomic; integer adds
//                       commute: bit-identical.
//   k_post_row_offsets  am_spans_of_needle: one lane per haystack h in 0 .. n_hay, a lower-bound search over the haystack field of the row.
// LDS: 1 KiB in k_post_hist, 8 KiB in k_post_scatter (two 4 x 256 tables).  Plain C++ and vector stores only.  NOT TUNED: the keys are read twice by the scatter, its
// stores land in up to 2^bits runs per tile, and whether staging a tile in LDS in sorted order pays off has not been tried.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "am_bounds.h"
#include "am_device.h"
#include "am_postings.h"
#include "am_wave.h"

AM_BOUNDS_TU("am_postings.hip")

namespace am {
namespace dev {

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kPostWaves = kPostThreads / kWave;
constexpr uint32_t kPostMaxDigits = 1u << kPostMaxDigitBits;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;
static_assert(kPostTileSpans % kPostThreads == 0 && kPostWaveSpans % kWave == 0 && kPostTileSpans == kPostWaveSpans * kPostWaves, "a tile is whole rounds of whole wavefronts");

__global__ void __launch_bounds__(kRowThreads) k_post_keys(const Span* __restrict__ spans, uint64_t n, uint32_t* __restrict__ keys, uint32_t* __restrict__ idx)
{
    const uint64_t i = global_row();
    if (i < n) { keys[i] = spans[i].needle; idx[i] = (uint32_t)i; }
}

__global__ void __launch_bounds__(kPostThreads) k_post_hist(PostPlan plan, uint32_t pass, const uint32_t* __restrict__ keys, uint64_t n, uint64_t n_tiles,
                                                            uint32_t* __restrict__ counts)
{
    __shared__ uint32_t cnt[kPostMaxDigits];
    const uint32_t t = threadIdx.x, digits = post_digits(plan, pass);
    const uint64_t tile = blockIdx.x;
    cnt[t] = 0;                                             // (kPostThreads == kPostMaxDigits)
    __syncthreads();
    const uint64_t i0 = tile * kPostTileSpans;
    for (uint32_t k = t; k < kPostTileSpans; k += kPostThreads) {
        const uint64_t i = i0 + k;
        if (i < n) atomicAdd(&cnt[post_digit(plan, keys[i], pass)], 1u);
    }
    __syncthreads();
    AM_BOUNDS(tile < n_tiles);
    if (t < digits && tile < n_tiles) counts[post_cell(t, tile, n_tiles)] = cnt[t];
}
static_assert(kPostThreads == kPostMaxDigits, "k_post_hist and k_post_scatter give every digit value a lane");

__global__ void __launch_bounds__(kPostThreads) k_post_scatter(PostPlan plan, uint32_t pass, const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ idx_in,
                                                               uint64_t n, uint64_t n_tiles, const uint64_t* __restrict__ base, uint32_t* __restrict__ keys_out,
                                                               uint32_t* __restrict__ idx_out)
{
    __shared__ uint32_t wave_cnt[kPostWaves][kPostMaxDigits];      // sweep 1: the keys of wavefront w with digit d
    __shared__ uint32_t run[kPostWaves][kPostMaxDigits];           // sweep 2: where the next key of wavefront w with digit d goes (a destination is below n < 2^32)
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const uint32_t digits = post_digits(plan, pass), bits = plan.bits[pass];
    const uint64_t tile = blockIdx.x;
    const uint64_t w0 = tile * kPostTileSpans + (uint64_t)w * kPostWaveSpans;      // the wavefront's first key
#pragma unroll
    for (uint32_t k = 0; k < kPostWaves; k++) wave_cnt[k][t] = 0;
    __syncthreads();
    for (uint32_t r = 0; r < kPostWaveSpans; r += kWave) {
        const uint64_t i = w0 + r + lane;
        if (i < n) atomicAdd(&wave_cnt[w][post_digit(plan, keys_in[i], pass)], 1u);
    }
    __syncthreads();
    if (t < digits) {
        AM_BOUNDS(tile < n_tiles && base[post_cell(t, tile, n_tiles)] <= n);
        uint32_t at = (uint32_t)base[post_cell(t, tile, n_tiles)];
#pragma unroll
        for (uint32_t k = 0; k < kPostWaves; k++) { run[k][t] = at; at += wave_cnt[k][t]; }
    }
    __syncthreads();
    // from here on a wavefront touches its own row of `run` only: no barrier, the rounds of a wavefront follow one another in program order
    for (uint32_t r = 0; r < kPostWaveSpans; r += kWave) {
        const uint64_t i = w0 + r + lane;
        const bool active = i < n;
        const uint64_t in_round = __ballot(active);
        if (in_round == 0) break;                           // (uniform: the portion ends here)
        uint32_t key = 0, ix = 0;
        if (active) { key = keys_in[i]; ix = idx_in[i]; }
        const uint32_t d = post_digit(plan, key, pass);
        uint64_t peers = in_round;                          // the active lanes of this round that hold digit d
        for (uint32_t b = 0; b < bits; b++) {
            const uint64_t set = __ballot((d >> b & 1u) != 0);
            peers &= (d >> b & 1u) != 0 ? set : ~set;
        }
        const uint64_t below = lane == 0 ? 0ull : ~0ull >> (kWave - lane);
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        uint32_t dest = 0;
        if (active) dest = run[w][d] + rank;
        wave_lds_fence();                                   // (every lane has read its counter before a last peer stores the next value)
        if (active) {
            AM_BOUNDS(dest < n);
            if (dest < n) { keys_out[dest] = key; idx_out[dest] = ix; }
            if ((peers >> lane >> 1) == 0) run[w][d] = dest + 1;      // the last peer: no peer in a higher lane
        }
        wave_lds_fence();
    }
}

__global__ void __launch_bounds__(kRowThreads) k_post_gather(const Span* __restrict__ spans, const uint32_t* __restrict__ idx, uint64_t n, Span* __restrict__ data,
                                                              uint64_t* __restrict__ source)
{
    const uint64_t k = global_row();
    if (k >= n) return;
    const uint64_t i = idx[k];
    AM_BOUNDS(i < n);
    if (i >= n) return;
    const uint64_t* __restrict__ src = (const uint64_t*)(spans + i);      // a row is 24 bytes at an 8-byte boundary: three loads, three stores
    uint64_t* __restrict__ dst = (uint64_t*)(data + k);
    const uint64_t a = src[0], b = src[1], c = src[2];
    dst[0] = a; dst[1] = b; dst[2] = c;
    source[k] = i;
}

__global__ void __launch_bounds__(kRowThreads) k_post_offsets(const uint32_t* __restrict__ keys, uint64_t n, uint64_t n_needles, uint64_t* __restrict__ offsets)
{
    const uint64_t v = global_row();
    if (v <= n_needles) offsets[v] = v == n_needles ? n : post_lower_bound(keys, n, 1, v);
}

__global__ void __launch_bounds__(kRowThreads) k_post_df(const Span* __restrict__ data, const uint32_t* __restrict__ keys, uint64_t n, uint64_t n_needles,
                                                          uint64_t* __restrict__ doc_freq)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t k = global_row();
    const bool active = k < n;
    uint32_t key = kNoKey;
    bool head = false;
    if (active) {
        key = keys[k];
        head = k == 0 || keys[k - 1] != key || data[k - 1].haystack != data[k].haystack;
    }
    const uint64_t heads = __ballot(head);
    if (heads == 0) return;                                 // (uniform)
    const uint32_t left = __shfl_up(key, 1, 64);
    const uint64_t firsts = __ballot(lane == 0 || left != key);      // the lanes that open a needle run inside this wavefront
    if (!active || !(lane == 0 || left != key)) return;
    const uint64_t above = firsts >> lane >> 1;             // the run ends before the next opening lane
    const uint32_t len = above == 0 ? kWave - lane : (uint32_t)__builtin_ctzll(above) + 1u;
    const uint64_t mine = (len == kWave ? ~0ull : (1ull << len) - 1ull) << lane;
    const uint32_t c = (uint32_t)__popcll(heads & mine);
    AM_BOUNDS(key < n_needles);
    if (c != 0 && key < n_needles) atomicAdd((unsigned long long*)&doc_freq[key], (unsigned long long)c);
}

__global__ void __launch_bounds__(kRowThreads) k_post_row_offsets(const Span* __restrict__ row, uint64_t n_row, uint64_t n_hay, uint64_t* __restrict__ out_off)
{
    const uint64_t h = global_row();
    if (h <= n_hay) out_off[h] = h == n_hay ? n_row : post_lower_bound((const uint32_t*)row + 4, n_row, sizeof(Span) / 4, h);      // (haystack: byte 16 of 24)
}
static_assert(sizeof(Span) == 24 && offsetof(Span, haystack) == 16 && offsetof(Span, needle) == 20, "Span: 0, 8, 16, 20");

}  // namespace

hipError_t launch_post_keys(const Span* spans, uint64_t n, uint32_t* keys, uint32_t* idx, hipStream_t st)
{
    if (n >= kPostMaxSpans) return hipErrorInvalidValue;
    return launch_rows(k_post_keys, n, st, spans, n, keys, idx);
}

hipError_t launch_post_hist(const PostPlan& plan, uint32_t pass, const uint32_t* keys, uint64_t n, uint32_t* counts, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    if (n >= kPostMaxSpans || pass >= plan.passes || plan.bits[pass] == 0 || plan.bits[pass] > kPostMaxDigitBits) return hipErrorInvalidValue;
    const uint64_t n_tiles = post_tiles(n);
    hipLaunchKernelGGL(k_post_hist, dim3((uint32_t)n_tiles), dim3(kPostThreads), 0, st, plan, pass, keys, n, n_tiles, counts);
    return hipGetLastError();
}

hipError_t launch_post_scatter(const PostPlan& plan, uint32_t pass, const uint32_t* keys_in, const uint32_t* idx_in, uint64_t n, const uint64_t* base, uint32_t* keys_out,
                               uint32_t* idx_out, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    if (n >= kPostMaxSpans || pass >= plan.passes || plan.bits[pass] == 0 || plan.bits[pass] > kPostMaxDigitBits) return hipErrorInvalidValue;
    const uint64_t n_tiles = post_tiles(n);
    hipLaunchKernelGGL(k_post_scatter, dim3((uint32_t)n_tiles), dim3(kPostThreads), 0, st, plan, pass, keys_in, idx_in, n, n_tiles, base, keys_out, idx_out);
    return hipGetLastError();
}

hipError_t launch_post_gather(const Span* spans, const uint32_t* idx, uint64_t n, Span* data, uint64_t* source, hipStream_t st)
{
    if (n >= kPostMaxSpans) return hipErrorInvalidValue;
    return launch_rows(k_post_gather, n, st, spans, idx, n, data, source);
}

hipError_t launch_post_offsets(const uint32_t* keys, uint64_t n, uint64_t n_needles, uint64_t* offsets, hipStream_t st)
{
    return launch_rows(k_post_offsets, n_needles + 1, st, keys, n, n_needles, offsets);
}

hipError_t launch_post_df(const Span* data, const uint32_t* keys, uint64_t n, uint64_t n_needles, uint64_t* doc_freq, hipStream_t st)
{
    if (n >= kPostMaxSpans) return hipErrorInvalidValue;
    return launch_rows(k_post_df, n, st, data, keys, n, n_needles, doc_freq);
}

hipError_t launch_post_row_offsets(const Span* row, uint64_t n_row, uint64_t n_hay, uint64_t* out_off, hipStream_t st)
{
    return launch_rows(k_post_row_offsets, n_hay + 1, st, row, n_row, n_hay, out_off);
}

}  // namespace dev
}  // namespace am
