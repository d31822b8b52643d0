// am_hist.hip -- per-needle match counts: the fold `Map.insertWith (+) v 1` over every (record, value of machineValues ! record.state)
// (reference: src/Data/Text/AhoCorasick/Automaton.hs:442-553 runWithCase and the folds over it; the count identity sum(counts) == countMatches is
// benchmark/haskell/app/Main.hs:67-76), on the records a scan has left in HBM.  A sibling of k_idset / k_fold_hash (am_records.hip): the same
// expansion of a record through the flat value lists of am_needle_ids (am_records.h), into a histogram uint64[n_needles] instead of a bitmap or a checksum.
//
// Natural text is Zipf-distributed: one global atomic per value would send a large share of all adds to a few dozen addresses, and adders that meet on
// one row run an order of magnitude below adders that are spread.  So the adds of a workgroup to the same id are combined ON CHIP:
//   * a persistent grid (a few workgroups per CU) walks the records in tiles of kHistTile;
//   * every workgroup keeps a direct-mapped table of kHistSlots {id tag, u32 count} in LDS.  A lane claims an empty slot for its id with an LDS
//     compare-and-swap on the tag; a slot that carries the id is an LDS add; a slot that carries another id is a conflict, and that one add goes to HBM
//     as a 64-bit global atomic (tags never change once claimed: no eviction, nothing to re-validate);
//   * at the end the workgroup adds every live slot to HBM with one 64-bit global atomic.
// No LDS counter can wrap: a record adds at most kHistLdsPerRecord times to LDS (the values of a list beyond that go to HBM directly), a tile has kHistTile
// records, and the workgroup flushes (and clears) its counts after at most kHistTilesPerFlush tiles (AM_HIST_FLUSH_TILES lets a test ask for fewer, never more):
// at most 1024 * 1024 * 2048 = 2^31 adds between two flushes, all of them to one slot in the worst case, below 2^32.
// Lane per RECORD, the value list of a record looped by its lane: the states of a dictionary carry one value almost everywhere (a suffix chain like
// tshirt / shirt / hirt a few), so a wave-wide prefix sum to spread values over lanes would be paid by every record for the sake of few.
// k_needle_hist_words is the same walk over the WHOLE-WORD spans of a table with a word class (am_count_spans_by_needle*): a value is added only where span_of
// (am_words.h) keeps the span it gives with its record -- the bincount of the AM_SPANS_ALL rows of that table.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "am_bounds.h"
#include "am_device.h"
#include "am_records.h"
#include "am_words.h"

AM_BOUNDS_TU("am_hist.hip")

namespace am {
namespace dev {

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kHistThreads = 256;
constexpr uint32_t kHistPerThread = 4;                    // records a lane takes per tile: their loads are issued together
constexpr uint32_t kHistTile = kHistThreads * kHistPerThread;
constexpr uint32_t kHistSlotBits = 12;
constexpr uint32_t kHistSlots = 1u << kHistSlotBits;      // 4096 slots = 32 KiB of LDS: four workgroups (16 wavefronts) per CU
constexpr uint32_t kHistLdsPerRecord = 1024;
constexpr uint32_t kHistTilesPerFlush = 2048;
constexpr uint32_t kHistEmpty = 0xFFFFFFFFu;              // no id: ids are < n_needles <= 2^32 - 1
constexpr int kHistGroupsPerCu = 4;
static_assert((uint64_t)kHistTile * kHistLdsPerRecord * kHistTilesPerFlush < (1ull << 32), "an LDS counter could wrap between two flushes");

// ids are handles in the caller's order (alphabetical, by frequency, ...): a multiplicative hash spreads neighbours over the table
__device__ __forceinline__ uint32_t hist_slot(uint32_t id) { return (id * 0x9E3779B1u) >> (32 - kHistSlotBits); }

// The walk over the tiles with the workgroup's LDS table (tag / cnt: kHistSlots words each, declared by the kernel).  WORDS / EXACT (View = SpansIn, otherwise
// RecordsIn): a value is added only where the table keeps the span it gives with its record -- span_of (am_words.h), the function the span expansion decides its rows
// with -- against the class in `words` (LDS) and the table's spellings.
template <bool kTrace, bool WORDS, bool IC, class View, bool EXACT = false>
__device__ __forceinline__ void hist_body(const View& in, uint32_t* tag, uint32_t* cnt, const uint32_t* words, unsigned long long* __restrict__ counts,
                                          unsigned long long* __restrict__ trace, uint32_t tiles_per_flush)
{
    const uint32_t* __restrict__ vals = in.vals;
    const uint32_t n_needles = in.n_needles;
    for (uint32_t i = threadIdx.x; i < kHistSlots; i += kHistThreads) { tag[i] = kHistEmpty; cnt[i] = 0; }
    __syncthreads();
    // every live slot to HBM with one add; `clear`: the counts start again (the tags stay: the hot ids keep their slots)
    auto flush = [&](bool clear) -> uint64_t {
        uint64_t adds = 0;
        for (uint32_t i = threadIdx.x; i < kHistSlots; i += kHistThreads) {
            const uint32_t c = cnt[i];
            if (c == 0) continue;
            const uint32_t id = tag[i];
            AM_BOUNDS(id < n_needles);
            if (id < n_needles) atomicAdd(&counts[id], (unsigned long long)c);
            if (clear) cnt[i] = 0;
            adds++;
        }
        return adds;
    };
    uint64_t in_lds = 0, in_hbm = 0, in_flush = 0;        // (kTrace only)
    const uint64_t n_tiles = (in.n_rec + kHistTile - 1) / kHistTile;
    uint32_t since_flush = 0;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {            // (the same tiles for every lane of the workgroup: the barriers below are uniform)
        uint64_t k[kHistPerThread], ke[kHistPerThread];
        Record rec[kHistPerThread];                                          // (beyond the state, WORDS only: the predicate needs the record's haystack and end)
        load_records<kHistPerThread, false>(in, t * kHistTile + threadIdx.x, kHistThreads, rec, k, ke);
#pragma unroll
        for (uint32_t u = 0; u < kHistPerThread; u++) {
            for (uint64_t j = 0; k[u] + j < ke[u]; j++) {
                const uint32_t id = vals[k[u] + j];
                if (id >= n_needles) continue;                               // a handle beyond the table: skipped, as containsAll skips it (k_idset)
                if constexpr (WORDS || EXACT) {
                    uint64_t ss, sn;
                    if (!span_of<IC, WORDS, EXACT>(in, rec[u], id, words, ss, sn)) continue;      // not kept: no row of the span table, no count
                }
                uint32_t s = 0;
                bool hit = false;
                if (j < kHistLdsPerRecord) {
                    s = hist_slot(id);
                    AM_BOUNDS(s < kHistSlots);
                    uint32_t tg = ((volatile uint32_t*)tag)[s];
                    if (tg == kHistEmpty) { tg = atomicCAS(&tag[s], kHistEmpty, id); if (tg == kHistEmpty) tg = id; }
                    hit = tg == id;
                }
                if (hit) atomicAdd(&cnt[s], 1u);
                else atomicAdd(&counts[id], 1ull);
                if (kTrace) { if (hit) in_lds++; else in_hbm++; }
            }
        }
        if (++since_flush >= tiles_per_flush) {
            __syncthreads();
            in_flush += flush(true);
            __syncthreads();
            since_flush = 0;
        }
    }
    __syncthreads();
    in_flush += flush(false);
    if (kTrace) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { in_lds += __shfl_xor(in_lds, d, kWave); in_hbm += __shfl_xor(in_hbm, d, kWave); in_flush += __shfl_xor(in_flush, d, kWave); }
        if ((threadIdx.x & (kWave - 1)) == 0) { atomicAdd(&trace[0], in_lds); atomicAdd(&trace[1], in_hbm); atomicAdd(&trace[2], in_flush); }
    }
}

template <bool kTrace>
__global__ void __launch_bounds__(kHistThreads) k_needle_hist(RecordsIn in, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ trace,
                                                              uint32_t tiles_per_flush)
{
    __shared__ uint32_t tag[kHistSlots];
    __shared__ uint32_t cnt[kHistSlots];
    hist_body<kTrace, false, false>(in, tag, cnt, nullptr, counts, trace, tiles_per_flush);
}

// the whole-word form: the workgroup stages the table's 32-byte class in LDS beside its tables; the LDS-counter wrap argument is the plain kernel's (a record adds
// at most as often as there)
template <bool kTrace, bool IC, bool WORDS = true, bool EXACT = false>
__global__ void __launch_bounds__(kHistThreads) k_needle_hist_words(SpansIn in, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ trace,
                                                                    uint32_t tiles_per_flush)
{
    __shared__ uint32_t tag[kHistSlots];
    __shared__ uint32_t cnt[kHistSlots];
    __shared__ uint32_t words[kWordClassWords];
    if (WORDS && threadIdx.x < kWordClassWords) words[threadIdx.x] = in.words[threadIdx.x];      // (hist_body's first barrier comes before any read)
    hist_body<kTrace, WORDS, IC, SpansIn, EXACT>(in, tag, cnt, words, counts, trace, tiles_per_flush);
}

// what both launchers decide the same way: the persistent grid, and the flush interval (never more than the bound the wrap argument rests on)
template <class Kernel, class View>
hipError_t hist_run(Kernel kernel, const View& in, uint64_t* counts, uint64_t* trace, uint32_t flush_tiles, int n_cu, hipStream_t st)
{
    const dim3 grid((uint32_t)std::min<uint64_t>((in.n_rec + kHistTile - 1) / kHistTile, (uint64_t)(n_cu > 0 ? n_cu : 1) * kHistGroupsPerCu));
    const uint32_t tiles_per_flush = flush_tiles != 0 && flush_tiles < kHistTilesPerFlush ? flush_tiles : kHistTilesPerFlush;
    hipLaunchKernelGGL(kernel, grid, dim3(kHistThreads), 0, st, in, (unsigned long long*)counts, (unsigned long long*)trace, tiles_per_flush);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_needle_hist(const RecordsIn& in, uint64_t* counts, uint64_t* trace, uint32_t flush_tiles, int n_cu, hipStream_t st)
{
    if (in.n_rec == 0 || in.n_needles == 0) return hipSuccess;
    return hist_run(trace ? k_needle_hist<true> : k_needle_hist<false>, in, counts, trace, flush_tiles, n_cu, st);
}

hipError_t launch_needle_hist_words(bool ic, const SpansIn& in, uint64_t* counts, uint64_t* trace, uint32_t flush_tiles, int n_cu, hipStream_t st)
{
    if (in.n_rec == 0 || in.n_needles == 0) return hipSuccess;
    if (!in.words && !in.exact) return hipErrorInvalidValue;
    if (!in.exact) {
        const auto kernel = trace ? (ic ? k_needle_hist_words<true, true> : k_needle_hist_words<true, false>) : (ic ? k_needle_hist_words<false, true> : k_needle_hist_words<false, false>);
        return hist_run(kernel, in, counts, trace, flush_tiles, n_cu, st);
    }
    // spellings (include/am.h "exact case"), with a class or without one
    const auto kernel = in.words ? (trace ? (ic ? k_needle_hist_words<true, true, true, true> : k_needle_hist_words<true, false, true, true>)
                                          : (ic ? k_needle_hist_words<false, true, true, true> : k_needle_hist_words<false, false, true, true>))
                                 : (trace ? (ic ? k_needle_hist_words<true, true, false, true> : k_needle_hist_words<true, false, false, true>)
                                          : (ic ? k_needle_hist_words<false, true, false, true> : k_needle_hist_words<false, false, false, true>));
    return hist_run(kernel, in, counts, trace, flush_tiles, n_cu, st);
}

}  // namespace dev
}  // namespace am
