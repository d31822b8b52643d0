// am_score.hip -- scores on the device (include/am.h "scores"): the fold `acc + weight v` over every (record, value of machineValues ! record.state) of a scan
// (reference: src/Data/Text/AhoCorasick/Automaton.hs:442-553 runWithCase and the folds over it), kept PER HAYSTACK and per weight column, and the top-k / range
// selection over a column of the result.
//
// k_score is a sibling of k_needle_hist (am_hist.hip): the same persistent grid, the same record tiles, a lane per RECORD and the record's value list looped by its
// lane.  What differs is where the adds go.  The records of a scan are sorted by (haystack, end position), so equal haystacks are consecutive: the score of a haystack
// is a SEGMENTED SUM over the record array and needs no table.  A wavefront owns kScoreWaveRecords consecutive records of a tile and takes them 64 at a time:
//   * a lane sums the weights of its own record's values in registers, one 64-bit sum per column;
//   * the lanes that hold the same haystack are combined across lanes: a segmented inclusive scan with shuffles, keyed on "my haystack differs from the previous
//     lane's" (one ballot gives every lane the start of its segment).  A wavefront whose 64 records are one haystack -- the ballot is 1 -- takes a plain reduction;
//   * a run that ends INSIDE the 64 records is finished: its last lane adds it to HBM, one 64-bit atomic per column.  The run the 64 records end with is carried in
//     scalar registers into the wavefront's next 64 records, its next tile included, and goes to HBM only when the haystack changes or the walk ends.
// So there is no atomic per value or per record: at most one add per column for each run of equal haystacks a wavefront holds.  A 1-MiB document costs a handful of
// adds per wavefront; a corpus of lines costs about one add per line and column, to addresses that are spread out.  Integer adds commute and wrap modulo 2^64: the
// scores are bit-identical from run to run and across groups and segments.  A sum of zero is not sent (the scores start at zero).
// k_score<WORDS = true> adds a value only where span_of (am_words.h) keeps the span it gives with its record: the rows am_count_spans_by_needle* counts.  EXACT: the
// same with the table's spellings (include/am.h "exact case").
//
// Top-k of a column: score_key / topk_pick (am_score.h) in eight passes of an 8-bit radix select -- k_topk_hist counts the next digit of the keys that share the
// digits chosen so far in LDS bins and adds the bins to 256 words of HBM, k_topk_pick (one wavefront) chooses the digit and clears the words -- leave the k-th key T
// and the tie quota q in HBM; no histogram crosses to the host.  k_topk_ties marks key == T, the library's exclusive sum (am_scan.hip) ranks the ties in haystack
// order, k_topk_flags writes flags[h] = key > T || (key == T && rank < q).  k_score_range writes lo <= score <= hi.  The flags go to the select's compaction
// (am_select.cpp); k_topk_gather collects the winners' {score, haystack} for am_scores_top_k.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "am_bounds.h"
#include "am_device.h"
#include "am_records.h"
#include "am_score.h"
#include "am_wave.h"
#include "am_words.h"

AM_BOUNDS_TU("am_score.hip")

namespace am {
namespace dev {

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kScoreThreads = 256;
constexpr uint32_t kScorePerThread = 4;                    // records a lane takes per tile: their loads are issued together
constexpr uint32_t kScoreWaveRecords = kWave * kScorePerThread;      // consecutive records a wavefront owns in a tile
constexpr uint32_t kScoreTile = kScoreThreads * kScorePerThread;
constexpr int kScoreGroupsPerCu = 4;
constexpr uint32_t kTopkThreads = 256;
constexpr uint32_t kTopkPerThread = 8;
constexpr uint32_t kTopkBlock = kTopkThreads * kTopkPerThread;       // keys per workgroup of k_topk_hist
static_assert(kTopkThreads == kTopkBins, "a thread per bin");

// NC: the columns the instantiation has registers for (out.n_cols <= NC; the loops over columns are unrolled and skip those beyond).  View: SpansIn or RecordsIn
template <bool WORDS, bool IC, uint32_t NC, class View, bool EXACT = false>
__device__ __forceinline__ void score_body(const uint32_t* words, const View& in, const ScoreOut& out)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const uint32_t n_cols = out.n_cols;
    AM_BOUNDS(n_cols >= 1 && n_cols <= NC);
    // the run this wavefront has not sent yet: wave-uniform
    uint32_t carry_h = kNoHay;
    uint64_t carry[NC];
#pragma unroll
    for (uint32_t c = 0; c < NC; c++) carry[c] = 0;
    auto send = [&](uint32_t h, const uint64_t* s) {       // one add per column of a finished run, by the lane that holds it
        AM_BOUNDS(h < in.n_hay);
        if (h >= in.n_hay) return;
#pragma unroll
        for (uint32_t c = 0; c < NC; c++)
            if (c < n_cols && s[c] != 0) atomicAdd(&out.scores[(uint64_t)c * out.stride + h], (unsigned long long)s[c]);
    };
    const uint64_t n_tiles = (in.n_rec + kScoreTile - 1) / kScoreTile;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t base = t * kScoreTile + (uint64_t)wv * kScoreWaveRecords;
        if (base >= in.n_rec) continue;                                      // (wave-uniform; no barrier in the walk)
        Record rec[kScorePerThread];
        uint64_t k[kScorePerThread], ke[kScorePerThread];
        load_records<kScorePerThread, true>(in, base + lane, kWave, rec, k, ke);      // (a record of a haystack beyond the batch: kNoHay, nothing added)
#pragma unroll
        for (uint32_t u = 0; u < kScorePerThread; u++) {
            if (base + u * kWave >= in.n_rec) break;                         // (wave-uniform)
            const uint32_t h = rec[u].haystack;
            uint64_t s[NC];
#pragma unroll
            for (uint32_t c = 0; c < NC; c++) s[c] = 0;
            for (uint64_t j = k[u]; j < ke[u]; j++) {
                const uint32_t id = in.vals[j];
                if (id >= in.n_needles) continue;                            // a handle beyond the table: skipped, as am_count_by_needle skips it
                if constexpr (WORDS || EXACT) {
                    uint64_t ss, sn;
                    if (!span_of<IC, WORDS, EXACT>(in, rec[u], id, words, ss, sn)) continue;      // not kept: no row of the span table, nothing added
                }
#pragma unroll
                for (uint32_t c = 0; c < NC; c++)
                    if (c < n_cols) s[c] += (uint64_t)out.weights[(uint64_t)c * in.n_needles + id];
            }
            // the carried run: continued by lane 0 where these records begin with its haystack, sent where they do not
            const uint32_t h0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)h);
            if (carry_h != kNoHay) {
                if (carry_h == h0) {
                    if (lane == 0) {
#pragma unroll
                        for (uint32_t c = 0; c < NC; c++) s[c] += carry[c];
                    }
                } else if (lane == 0) {
                    send(carry_h, carry);
                }
            }
            const uint32_t before = __shfl_up(h, 1, kWave);
            const bool head = lane == 0 || before != h;
            const uint64_t heads = __ballot(head);                           // (bit 0 is always set)
            if (heads == 1ull) {
                // one haystack in all 64 lanes: a plain reduction, and everything stays carried
#pragma unroll
                for (uint32_t c = 0; c < NC; c++) carry[c] = c < n_cols ? uniform_u64(wave_sum_u64(s[c])) : 0;
                carry_h = h0;
                continue;
            }
            // segmented inclusive scan: a lane takes what lies d lanes below it while that is still inside its own run
            const uint32_t start = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));
            const uint32_t dist = lane - start;
#pragma unroll
            for (uint32_t d = 1; d < kWave; d <<= 1) {
#pragma unroll
                for (uint32_t c = 0; c < NC; c++) {
                    if (c < n_cols) {
                        const uint64_t y = __shfl_up(s[c], d, kWave);
                        if (dist >= d) s[c] += y;
                    }
                }
            }
            // the last lane of a run that ends inside these 64 records sends it; the run of lane 63 is carried on
            const bool last_of_run = lane < kWave - 1 && ((heads >> (lane + 1)) & 1ull) != 0;
            if (last_of_run && h != kNoHay) send(h, s);
            carry_h = (uint32_t)__builtin_amdgcn_readlane((int)h, 63);
#pragma unroll
            for (uint32_t c = 0; c < NC; c++) carry[c] = c < n_cols ? wave_read_lane(s[c], 63) : 0;
        }
    }
    if (carry_h != kNoHay && lane == 0) send(carry_h, carry);
}

template <uint32_t NC>
__global__ void __launch_bounds__(kScoreThreads) k_score(RecordsIn in, ScoreOut out)
{
    score_body<false, false, NC>(nullptr, in, out);
}

// the whole-word form: the workgroup stages the table's 32-byte class in LDS
template <bool IC, uint32_t NC, bool WORDS = true, bool EXACT = false>
__global__ void __launch_bounds__(kScoreThreads) k_score_words(SpansIn in, ScoreOut out)
{
    __shared__ uint32_t words[kWordClassWords];
    if (WORDS && threadIdx.x < kWordClassWords) words[threadIdx.x] = in.words[threadIdx.x];
    __syncthreads();
    score_body<WORDS, IC, NC, SpansIn, EXACT>(words, in, out);
}

template <uint32_t NC>
void score_launch(bool ic, dim3 grid, const SpansIn& in, const ScoreOut& out, hipStream_t st)
{
    const dim3 block(kScoreThreads);
    if (in.exact) {                                          // spellings (include/am.h "exact case"), with a class or without one
        if (in.words) { if (ic) hipLaunchKernelGGL((k_score_words<true, NC, true, true>), grid, block, 0, st, in, out); else hipLaunchKernelGGL((k_score_words<false, NC, true, true>), grid, block, 0, st, in, out); }
        else if (ic) hipLaunchKernelGGL((k_score_words<true, NC, false, true>), grid, block, 0, st, in, out);
        else hipLaunchKernelGGL((k_score_words<false, NC, false, true>), grid, block, 0, st, in, out);
    }
    else if (!in.words) hipLaunchKernelGGL((k_score<NC>), grid, block, 0, st, static_cast<const RecordsIn&>(in), out);
    else if (ic) hipLaunchKernelGGL((k_score_words<true, NC>), grid, block, 0, st, in, out);
    else hipLaunchKernelGGL((k_score_words<false, NC>), grid, block, 0, st, in, out);
}

// ---- top-k and range select over one column

__global__ void __launch_bounds__(kTopkBins) k_topk_init(TopkState* __restrict__ state, unsigned long long* __restrict__ hist, uint64_t k)
{
    hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) { state->prefix = 0; state->k_left = k; }
}

__global__ void __launch_bounds__(kTopkThreads) k_topk_hist(const int64_t* __restrict__ col, uint64_t n, uint32_t largest, uint32_t digit,
                                                            const TopkState* __restrict__ state, unsigned long long* __restrict__ hist)
{
    __shared__ uint32_t bins[kTopkBins];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t prefix = state->prefix;
#pragma unroll
    for (uint32_t u = 0; u < kTopkPerThread; u++) {
        const uint64_t i = (uint64_t)blockIdx.x * kTopkBlock + u * kTopkThreads + threadIdx.x;
        if (i >= n) continue;
        const uint64_t key = score_key(col[i], largest != 0);
        if (!topk_in_prefix(key, prefix, digit)) continue;
        const uint32_t b = topk_digit(key, digit);
        AM_BOUNDS(b < kTopkBins);
        atomicAdd(&bins[b], 1u);                                             // (at most kTopkBlock per bin: no wrap)
    }
    __syncthreads();
    const uint32_t c = bins[threadIdx.x];
    if (c != 0) atomicAdd(&hist[threadIdx.x], (unsigned long long)c);
}

// one wavefront: the digit of this pass from the 256 words, which are cleared for the next pass
__global__ void __launch_bounds__(kWave) k_topk_pick(TopkState* __restrict__ state, unsigned long long* __restrict__ hist)
{
    __shared__ uint64_t h[kTopkBins];
    for (uint32_t i = threadIdx.x; i < kTopkBins; i += kWave) { h[i] = hist[i]; hist[i] = 0; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t k = state->k_left;
        const uint32_t d = topk_pick(h, &k);
        state->prefix = (state->prefix << 8) | d;
        state->k_left = k;
    }
}

// tie[i] = key i is the k-th key (n + 1 entries, the last one 0: the sum's trailing element)
__global__ void __launch_bounds__(kRowThreads) k_topk_ties(const int64_t* __restrict__ col, uint64_t n, uint32_t largest, const TopkState* __restrict__ state,
                                                            uint32_t* __restrict__ tie)
{
    const uint64_t i = global_row();
    if (i > n) return;
    tie[i] = i < n && score_key(col[i], largest != 0) == state->prefix ? 1u : 0u;
}

// with tie_rank = the exclusive sum of tie: the keys above the k-th and the first q of its ties.  flags: n bytes (nullable); keep: n + 1 words, the last one 0 (nullable)
__global__ void __launch_bounds__(kRowThreads) k_topk_flags(const int64_t* __restrict__ col, uint64_t n, uint32_t largest, const TopkState* __restrict__ state,
                                                             const uint64_t* __restrict__ tie_rank, uint8_t* __restrict__ flags, uint32_t* __restrict__ keep)
{
    const uint64_t i = global_row();
    if (i > n) return;
    if (i == n) { if (keep) keep[i] = 0; return; }
    const uint64_t key = score_key(col[i], largest != 0), cut = state->prefix, quota = state->k_left;
    const bool f = key > cut || (key == cut && tie_rank[i] < quota);
    if (flags) flags[i] = f ? 1 : 0;
    if (keep) keep[i] = f ? 1u : 0u;
}

__global__ void __launch_bounds__(kRowThreads) k_score_range(const int64_t* __restrict__ col, uint64_t n, int64_t lo, int64_t hi, uint8_t* __restrict__ flags)
{
    const uint64_t i = global_row();
    if (i >= n) return;
    const int64_t s = col[i];
    flags[i] = lo <= s && s <= hi ? 1 : 0;
}

// with pos = the exclusive sum of keep: the winners in ascending haystack order
__global__ void __launch_bounds__(kRowThreads) k_topk_gather(const int64_t* __restrict__ col, uint64_t n, const uint32_t* __restrict__ keep, const uint64_t* __restrict__ pos,
                                                              Scored* __restrict__ out, uint64_t n_out)
{
    const uint64_t i = global_row();
    if (i >= n || !keep[i]) return;
    const uint64_t p = pos[i];
    AM_BOUNDS(p < n_out);
    if (p >= n_out) return;
    Scored x;
    x.score = col[i]; x.haystack = (uint32_t)i; x.reserved = 0;
    out[p] = x;
}

}  // namespace

void score_geometry(uint32_t* tile_records, uint32_t* topk_block_items)
{
    if (tile_records) *tile_records = kScoreTile;
    if (topk_block_items) *topk_block_items = kTopkBlock;
}

hipError_t launch_score(bool ic, const SpansIn& in, const ScoreOut& out, int n_cu, hipStream_t st)
{
    if (in.n_rec == 0 || in.n_needles == 0 || in.n_hay == 0) return hipSuccess;
    if (out.n_cols == 0 || out.n_cols > kScoreMaxColumns || out.stride < in.n_hay) return hipErrorInvalidValue;
    const uint64_t n_tiles = (in.n_rec + kScoreTile - 1) / kScoreTile;
    const dim3 grid((uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)(n_cu > 0 ? n_cu : 1) * kScoreGroupsPerCu));
    if (out.n_cols == 1) score_launch<1>(ic, grid, in, out, st);
    else if (out.n_cols <= 4) score_launch<4>(ic, grid, in, out, st);
    else score_launch<8>(ic, grid, in, out, st);
    return hipGetLastError();
}

hipError_t launch_topk_flags(const int64_t* col, uint64_t n, uint64_t k, bool largest, const TopkWork& w, uint8_t* flags, uint32_t* keep, hipStream_t st)
{
    if (n == 0 || k == 0 || k > n) return hipErrorInvalidValue;          // (the callers answer k == 0 themselves and cap k at n)
    const uint32_t lg = largest ? 1u : 0u;
    const dim3 hist_grid((uint32_t)((n + kTopkBlock - 1) / kTopkBlock));
    hipLaunchKernelGGL(k_topk_init, dim3(1), dim3(kTopkBins), 0, st, w.state, (unsigned long long*)w.hist, k);
    for (uint32_t digit = kTopkDigits; digit-- > 0;) {
        hipLaunchKernelGGL(k_topk_hist, hist_grid, dim3(kTopkThreads), 0, st, col, n, lg, digit, (const TopkState*)w.state, (unsigned long long*)w.hist);
        hipLaunchKernelGGL(k_topk_pick, dim3(1), dim3(kWave), 0, st, w.state, (unsigned long long*)w.hist);
    }
    hipError_t e = launch_rows(k_topk_ties, n + 1, st, col, n, lg, w.state, w.tie);
    if (e == hipSuccess) e = launch_scan(w.scan_tmp, w.scan_tmp_bytes, w.tie, w.tie_rank, n + 1, st);
    return e != hipSuccess ? e : launch_rows(k_topk_flags, n + 1, st, col, n, lg, w.state, w.tie_rank, flags, keep);
}

hipError_t launch_score_range(const int64_t* col, uint64_t n, int64_t lo, int64_t hi, uint8_t* flags, hipStream_t st)
{
    return launch_rows(k_score_range, n, st, col, n, lo, hi, flags);
}

hipError_t launch_topk_gather(const int64_t* col, uint64_t n, const uint32_t* keep, const uint64_t* pos, Scored* out, uint64_t n_out, hipStream_t st)
{
    return launch_rows(k_topk_gather, n_out ? n : 0, st, col, n, keep, pos, out, n_out);
}

}  // namespace dev
}  // namespace am
