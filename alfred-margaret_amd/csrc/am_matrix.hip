// am_matrix.hip -- the term-document matrix: the fold `Map.insertWith (+) v 1` of runWithCase (reference: src/Data/Text/AhoCorasick/Automaton.hs:442-553) run once PER
// HAYSTACK, as a CSR matrix {count, needle, haystack} with one row per haystack, rows sorted by needle, built in HBM from the sorted records a scan has left there.
// A sibling of k_needle_hist (am_hist.hip): the same expansion of a record through the value lists of am_needle_ids (am_records.h), keyed by (haystack, needle).
//
// The two shapes it has to serve pull apart: lines of natural text are millions of rows of a handful of entries (a tile of records spans dozens of rows), and
// `a, aa, aaa` over 16 MiB of `a` is one row of three entries that 48 M adds meet.  One global atomic per value onto a hot key is an order of magnitude too slow, and
// sorting every (haystack, needle) pair before combining pays 48 M keys for three entries.  So, per group of haystacks:
//   1. k_mx_values    sums the lengths of the records' value lists: V >= the distinct keys of the group; the table in HBM gets min(V, rows x needles) * 3 / 2 + 64 slots
//                     and can never fill.
//   2. k_mx_combine   a persistent grid over CHUNKS of kMxChunk consecutive records.  A lane first folds the run of equal ids in its own record's list, then adds to
//                     the workgroup's LDS table of kMxSlots {u64 key, u32 count} (a 64-bit LDS compare-and-swap claims a slot; a slot that carries another key is a
//                     conflict, and that add goes to HBM directly).  After every chunk the live slots are added to the open-addressing table in HBM -- a 64-bit
//                     compare-and-swap on the key, a 64-bit add on the count, the lane that claims a slot adds 1 to row_entries[haystack] -- and the LDS table is
//                     cleared: the records are sorted by haystack, a later chunk brings other keys.  One global atomic pair per distinct (chunk, key) in the common case.
//                     No LDS counter can wrap: a record adds at most kMxLdsPerRecord to LDS, a chunk has kMxChunk records (static_assert below).
//   3. launch_scan    row_entries -> offsets (am_scan.hip).
//   4. k_mx_scatter   one pass over the table: live slots into their rows, row_entries[haystack] counted down as the row's cursor.  The order inside a row is the order
//                     of arrival here, so ...
//   5. k_mx_rows*     ... every row is ordered by needle, out of place (scattered entries -> result): rows of up to kMxWaveRow entries by ranking inside a wavefront (the keys of a
//                     row are distinct: rank = keys below mine), rows of up to kMxLdsRow by a workgroup's bitonic sort of (needle, index) in LDS, longer rows by ranking
//                     through a presence bitmap of n_needles bits (the containsAll row layout) with a popcount prefix: no sort at all.
// Counts are sums of integers and every row ends sorted by a key that is unique in it: the result is bit-identical from run to run whatever the order of the atomics.
// Every barrier below is reached by all lanes of its workgroup: the trip counts around them depend on blockIdx, kernel arguments and values every lane reads from the same address.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "am_bounds.h"
#include "am_device.h"
#include "am_records.h"

AM_BOUNDS_TU("am_matrix.hip")

namespace am {
namespace dev {

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kMxThreads = 256;
constexpr uint32_t kMxPerThread = 4;                      // records a lane takes per tile: their loads are issued together
constexpr uint32_t kMxTile = kMxThreads * kMxPerThread;
constexpr uint32_t kMxTilesPerChunk = 4;
constexpr uint32_t kMxChunk = kMxTile * kMxTilesPerChunk; // records between two flushes of the LDS table
constexpr uint32_t kMxSlotBits = 11;
constexpr uint32_t kMxSlots = 1u << kMxSlotBits;          // 2048 slots = 24 KiB of LDS: four workgroups (16 wavefronts) per CU with room to spare
constexpr uint32_t kMxLdsPerRecord = 1024;
constexpr uint64_t kMxEmpty = ~0ull;                      // no key: haystacks are < 2^32 - 1
constexpr uint32_t kMxNoId = 0xFFFFFFFFu;                 // no id: ids are < n_needles <= 2^32 - 1
constexpr int kMxGroupsPerCu = 4;
static_assert((uint64_t)kMxChunk * kMxLdsPerRecord < (1ull << 32), "an LDS counter could wrap between two flushes");
static_assert(kMxLdsRow % kMxThreads == 0 && (kMxLdsRow & (kMxLdsRow - 1)) == 0, "the bitonic network wants a power of two");
static_assert(kMxWaveRow == kWave, "a short row is ranked by one wavefront");

__device__ __forceinline__ uint64_t mx_mix(uint64_t key) { return key * 0x9E3779B97F4A7C15ull; }     // (the high bits depend on every bit of the key)

// count += c under `key` in the table in HBM; the lane that claims the slot counts the row's new entry
__device__ __forceinline__ void mx_insert(uint64_t key, uint64_t c, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ cnts, uint64_t cap,
                                          uint32_t* __restrict__ row_entries, uint32_t n_rows)
{
    const uint32_t hay = (uint32_t)(key >> 32);
    AM_BOUNDS(hay < n_rows && cap != 0);
    if (hay >= n_rows) return;
    uint64_t h = __umul64hi(mx_mix(key), cap);
    for (uint64_t probes = 0; probes < cap; probes++) {
        AM_BOUNDS(h < cap);
        unsigned long long cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (a key never changes once set: only `empty` can be stale)
        if (cur == kMxEmpty) {
            cur = atomicCAS(&keys[h], (unsigned long long)kMxEmpty, (unsigned long long)key);
            if (cur == kMxEmpty) { atomicAdd(&row_entries[hay], 1u); cur = key; }
        }
        if (cur == key) { atomicAdd(&cnts[h], (unsigned long long)c); return; }
        if (++h == cap) h = 0;
    }
    AM_BOUNDS(false);                                     // the table is larger than the keys it can meet
}

// (every value: the table is sized for the handles beyond n_needles too.  The one fold that reads vals_off itself: through value_range this loop measured 17 % slower
// in two sessions, for no reason the ISA shows -- profiles/r25_record_folds.md -- so it keeps the tests it had: a list that is out of range adds nothing)
__global__ void __launch_bounds__(kMxThreads) k_mx_values(RecordsIn in, unsigned long long* __restrict__ total)
{
    uint64_t v = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kMxThreads + threadIdx.x; r < in.n_rec; r += (uint64_t)gridDim.x * kMxThreads) {
        const uint32_t state = in.recs[r].state;
        AM_BOUNDS(state < in.n_states);
        if (state >= in.n_states) continue;
        const uint64_t k = in.vals_off[state], ke = in.vals_off[state + 1];
        AM_BOUNDS(k <= ke && ke <= in.n_values);
        if (k <= ke && ke <= in.n_values) v += ke - k;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && v) atomicAdd(total, (unsigned long long)v);
}

__global__ void __launch_bounds__(kMxThreads) k_mx_combine(RecordsIn in, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ cnts, uint64_t cap,
                                                           uint32_t* __restrict__ row_entries)
{
    __shared__ unsigned long long tag[kMxSlots];
    __shared__ uint32_t cnt[kMxSlots];
    for (uint32_t i = threadIdx.x; i < kMxSlots; i += kMxThreads) { tag[i] = kMxEmpty; cnt[i] = 0; }
    __syncthreads();
    const uint64_t n_chunks = (in.n_rec + kMxChunk - 1) / kMxChunk;
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {            // (the same chunks for every lane of the workgroup: the barriers below are uniform)
        for (uint32_t t = 0; t < kMxTilesPerChunk; t++) {
            uint64_t k[kMxPerThread], ke[kMxPerThread];
            Record rec[kMxPerThread];
            load_records<kMxPerThread, true>(in, c * kMxChunk + t * kMxTile + threadIdx.x, kMxThreads, rec, k, ke);      // (a record of a haystack beyond the group: emptied)
#pragma unroll
            for (uint32_t u = 0; u < kMxPerThread; u++) {
                uint32_t budget = kMxLdsPerRecord;                          // what this record may still add to LDS counters
                // `n` occurrences of `id` in this record's list: to the workgroup's table, or (slot taken by another key, budget spent) to HBM
                auto emit = [&](uint32_t id, uint64_t n) {
                    const uint64_t key = (uint64_t)rec[u].haystack << 32 | id;
                    if (n <= budget) {
                        const uint32_t s = (uint32_t)(mx_mix(key) >> (64 - kMxSlotBits));
                        AM_BOUNDS(s < kMxSlots);
                        unsigned long long tg = ((volatile unsigned long long*)tag)[s];
                        if (tg == kMxEmpty) { tg = atomicCAS(&tag[s], (unsigned long long)kMxEmpty, (unsigned long long)key); if (tg == kMxEmpty) tg = key; }
                        if (tg == key) { budget -= (uint32_t)n; atomicAdd(&cnt[s], (uint32_t)n); return; }
                    }
                    mx_insert(key, n, keys, cnts, cap, row_entries, in.n_hay);
                };
                uint32_t pend = kMxNoId; uint64_t run = 0;                  // equal neighbours of a list (one needle given many times under one handle) are one add
                for (uint64_t j = k[u]; j < ke[u]; j++) {
                    const uint32_t id = in.vals[j];
                    if (id >= in.n_needles) continue;                       // a handle beyond the table: skipped, as am_count_by_needle skips it
                    if (id == pend) { run++; continue; }
                    if (run) emit(pend, run);
                    pend = id; run = 1;
                }
                if (run) emit(pend, run);
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < kMxSlots; i += kMxThreads) {
            const uint32_t n = cnt[i];
            if (n != 0) { mx_insert(tag[i], n, keys, cnts, cap, row_entries, in.n_hay); cnt[i] = 0; }
            tag[i] = kMxEmpty;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kMxThreads) k_mx_scatter(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ cnts, uint64_t cap,
                                                           const uint64_t* __restrict__ offsets, uint32_t* __restrict__ row_entries, uint32_t n_rows, uint32_t hay0,
                                                           NeedleCount* __restrict__ tmp, uint64_t n_entries)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kMxThreads + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * kMxThreads) {
        const uint64_t key = keys[i];
        if (key == kMxEmpty) continue;
        const uint32_t hay = (uint32_t)(key >> 32);
        AM_BOUNDS(hay < n_rows && cnts[i] != 0);
        if (hay >= n_rows) continue;
        const uint32_t left = atomicSub(&row_entries[hay], 1u);            // (the row's entry count, counted down: its cursor)
        const uint64_t at = offsets[hay] + (left - 1u);
        AM_BOUNDS(left != 0 && at < offsets[hay + 1] && at < n_entries);
        if (left == 0 || at >= n_entries) continue;
        NeedleCount e; e.count = cnts[i]; e.needle = (uint32_t)key; e.haystack = hay0 + hay;
        tmp[at] = e;
    }
}

// a lane per row: rows of one entry are copied, rows of up to kMxWaveRow entries are ranked by the row's wavefront one after the other, longer rows are listed for
// k_mx_rows_lds (from the front of `list`) and k_mx_rows_wide (from its back); ctr[0], ctr[1] = how many of each
__global__ void __launch_bounds__(kMxThreads) k_mx_rows(const NeedleCount* __restrict__ tmp, const uint64_t* __restrict__ offsets, uint32_t n_rows, uint64_t n_entries,
                                                        NeedleCount* __restrict__ out, uint32_t* __restrict__ list, uint32_t* __restrict__ ctr)
{
    const uint64_t r = (uint64_t)blockIdx.x * kMxThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    uint64_t start = 0, len = 0;
    if (r < n_rows) { start = offsets[r]; len = offsets[r + 1] - start; }
    AM_BOUNDS(start + len <= n_entries && start + len >= start);
    if (start + len > n_entries || start + len < start) len = 0;
    if (len == 1) out[start] = tmp[start];
    else if (len > kMxWaveRow) {
        const uint32_t at = len <= kMxLdsRow ? atomicAdd(&ctr[0], 1u) : n_rows - 1u - atomicAdd(&ctr[1], 1u);
        AM_BOUNDS(at < n_rows);
        if (at < n_rows) list[at] = (uint32_t)r;
    }
    uint64_t todo = __ballot(len >= 2 && len <= kMxWaveRow);
    while (todo) {
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t s = __shfl(start, src, kWave);
        const uint32_t n = (uint32_t)__shfl(len, src, kWave);
        NeedleCount e; e.count = 0; e.needle = kMxNoId; e.haystack = 0;
        if (lane < n) e = tmp[s + lane];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; j++) rank += __shfl(e.needle, (int)j, kWave) < e.needle ? 1u : 0u;
        AM_BOUNDS(lane >= n || rank < n);
        if (lane < n && rank < n) out[s + rank] = e;
    }
}

__global__ void __launch_bounds__(kMxThreads) k_mx_rows_lds(const NeedleCount* __restrict__ tmp, const uint64_t* __restrict__ offsets, uint32_t n_rows, uint64_t n_entries,
                                                            const uint32_t* __restrict__ list, const uint32_t* __restrict__ ctr, NeedleCount* __restrict__ out)
{
    __shared__ uint64_t key[kMxLdsRow];                      // needle << 32 | index in the row
    const uint32_t n_list = min(ctr[0], n_rows);
    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        const uint32_t r = list[li];
        AM_BOUNDS(r < n_rows);
        uint64_t start = 0; uint32_t len = 0;
        if (r < n_rows) { start = offsets[r]; const uint64_t l = offsets[r + 1] - start; AM_BOUNDS(l <= kMxLdsRow && start + l <= n_entries); if (l <= kMxLdsRow && start + l <= n_entries) len = (uint32_t)l; }
        uint32_t n2 = 2;
        while (n2 < len) n2 <<= 1;
        for (uint32_t i = threadIdx.x; i < n2; i += kMxThreads) key[i] = i < len ? ((uint64_t)tmp[start + i].needle << 32 | i) : ~0ull;
        __syncthreads();
        for (uint32_t k = 2; k <= n2; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = threadIdx.x; i < n2; i += kMxThreads) {
                    const uint32_t p = i ^ j;
                    if (p > i) {
                        const uint64_t a = key[i], b = key[p];
                        if ((a > b) == ((i & k) == 0)) { key[i] = b; key[p] = a; }
                    }
                }
                __syncthreads();
            }
        }
        for (uint32_t i = threadIdx.x; i < len; i += kMxThreads) {
            const uint32_t from = (uint32_t)key[i];
            AM_BOUNDS(from < len);
            if (from < len) out[start + i] = tmp[start + from];
        }
        __syncthreads();
    }
}

// rows beyond the LDS capacity: every workgroup owns a bitmap of n_needles bits (clear on entry, cleared again on the way out) and the popcount prefix of its words
__global__ void __launch_bounds__(kMxThreads) k_mx_rows_wide(const NeedleCount* __restrict__ tmp, const uint64_t* __restrict__ offsets, uint32_t n_rows, uint64_t n_entries,
                                                             const uint32_t* __restrict__ list, const uint32_t* __restrict__ ctr, uint32_t n_needles, uint32_t words,
                                                             uint32_t* __restrict__ bits_all, uint32_t* __restrict__ pre_all, NeedleCount* __restrict__ out)
{
    __shared__ uint32_t wsum[kMxThreads / kWave];
    uint32_t* const bits = bits_all + (uint64_t)blockIdx.x * words;
    uint32_t* const pre = pre_all + (uint64_t)blockIdx.x * words;
    const uint32_t n_list = min(ctr[1], n_rows);
    const uint32_t per = (words + kMxThreads - 1) / kMxThreads;            // words a lane sums: a contiguous run
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        const uint32_t r = list[n_rows - 1u - li];
        AM_BOUNDS(r < n_rows);
        uint64_t start = 0, len = 0;
        if (r < n_rows) { start = offsets[r]; len = offsets[r + 1] - start; }
        AM_BOUNDS(start + len <= n_entries && len <= n_needles);
        if (start + len > n_entries) len = 0;
        for (uint64_t i = threadIdx.x; i < len; i += kMxThreads) {
            const uint32_t nd = tmp[start + i].needle;
            AM_BOUNDS(nd < n_needles);
            if (nd < n_needles) atomicOr(&bits[nd >> 5], 1u << (nd & 31u));
        }
        __syncthreads();
        const uint64_t w0 = (uint64_t)threadIdx.x * per, w1 = min<uint64_t>(w0 + per, words);
        uint32_t mine = 0;
        for (uint64_t w = w0; w < w1; w++) mine += __popc(__hip_atomic_load(&bits[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(incl, d, kWave); if (lane >= (uint32_t)d) incl += y; }
        if (lane == kWave - 1) wsum[wave] = incl;
        __syncthreads();
        uint32_t run = incl - mine;
        for (uint32_t k = 0; k < wave; k++) run += wsum[k];
        for (uint64_t w = w0; w < w1; w++) { pre[w] = run; run += __popc(__hip_atomic_load(&bits[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
        __syncthreads();
        for (uint64_t i = threadIdx.x; i < len; i += kMxThreads) {
            const NeedleCount e = tmp[start + i];
            if (e.needle >= n_needles) continue;
            const uint32_t w = e.needle >> 5;
            const uint32_t below = __hip_atomic_load(&bits[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ((1u << (e.needle & 31u)) - 1u);
            const uint64_t rank = (uint64_t)__hip_atomic_load(&pre[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + __popc(below);
            AM_BOUNDS(rank < len);
            if (rank < len) out[start + rank] = e;
        }
        __syncthreads();
        for (uint64_t i = threadIdx.x; i < len; i += kMxThreads) {
            const uint32_t nd = tmp[start + i].needle;
            if (nd < n_needles) atomicExch(&bits[nd >> 5], 0u);
        }
        __syncthreads();
    }
}

uint32_t mx_grid(uint64_t items, int n_cu, uint32_t per_cu)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + kMxThreads - 1) / kMxThreads, (uint64_t)(n_cu > 0 ? n_cu : 1) * per_cu));
}

}  // namespace

void mx_limits(uint32_t* out4) { out4[0] = kMxWaveRow; out4[1] = kMxLdsRow; out4[2] = kMxSlots; out4[3] = kMxChunk; }

hipError_t launch_mx_values(const RecordsIn& in, uint64_t* total, int n_cu, hipStream_t st)
{
    if (in.n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mx_values, dim3(mx_grid(in.n_rec, n_cu, 16)), dim3(kMxThreads), 0, st, in, (unsigned long long*)total);
    return hipGetLastError();
}

hipError_t launch_mx_combine(const RecordsIn& in, uint64_t* keys, uint64_t* cnts, uint64_t cap, uint32_t* row_entries, int n_cu, hipStream_t st)
{
    if (in.n_rec == 0 || in.n_needles == 0 || in.n_hay == 0 || cap == 0) return hipSuccess;
    const uint64_t n_chunks = (in.n_rec + kMxChunk - 1) / kMxChunk;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_chunks, (uint64_t)(n_cu > 0 ? n_cu : 1) * kMxGroupsPerCu);
    hipLaunchKernelGGL(k_mx_combine, dim3(grid), dim3(kMxThreads), 0, st, in, (unsigned long long*)keys, (unsigned long long*)cnts, cap, row_entries);
    return hipGetLastError();
}

hipError_t launch_mx_scatter(const uint64_t* keys, const uint64_t* cnts, uint64_t cap, const uint64_t* offsets, uint32_t* row_entries, uint32_t n_rows, uint32_t hay0,
                             NeedleCount* tmp, uint64_t n_entries, int n_cu, hipStream_t st)
{
    if (cap == 0 || n_entries == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mx_scatter, dim3(mx_grid(cap, n_cu, 32)), dim3(kMxThreads), 0, st, (const unsigned long long*)keys, (const unsigned long long*)cnts, cap, offsets,
                       row_entries, n_rows, hay0, tmp, n_entries);
    return hipGetLastError();
}

hipError_t launch_mx_rows(const NeedleCount* tmp, const uint64_t* offsets, uint32_t n_rows, uint64_t n_entries, NeedleCount* out, uint32_t* list, uint32_t* ctr, hipStream_t st)
{
    if (n_rows == 0 || n_entries == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mx_rows, dim3((uint32_t)(((uint64_t)n_rows + kMxThreads - 1) / kMxThreads)), dim3(kMxThreads), 0, st, tmp, offsets, n_rows, n_entries, out, list, ctr);
    return hipGetLastError();
}

hipError_t launch_mx_rows_lds(const NeedleCount* tmp, const uint64_t* offsets, uint32_t n_rows, uint64_t n_entries, const uint32_t* list, const uint32_t* ctr,
                              NeedleCount* out, int n_cu, hipStream_t st)
{
    if (n_rows == 0 || n_entries <= kMxWaveRow) return hipSuccess;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(n_rows, n_entries / kMxWaveRow), (uint64_t)(n_cu > 0 ? n_cu : 1) * 8);
    hipLaunchKernelGGL(k_mx_rows_lds, dim3(grid), dim3(kMxThreads), 0, st, tmp, offsets, n_rows, n_entries, list, ctr, out);
    return hipGetLastError();
}

uint32_t mx_wide_grid(uint32_t n_rows, uint64_t n_entries, uint32_t n_needles, int n_cu)
{
    if (n_needles <= kMxLdsRow || n_entries <= kMxLdsRow || n_rows == 0) return 0;
    const uint64_t words = ((uint64_t)n_needles + 31) / 32;
    const uint64_t by_memory = std::max<uint64_t>(1, (256ull << 20) / (words * 8));      // bitmaps and prefixes: 256 MiB at most, one workgroup's at least
    return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(std::min<uint64_t>(n_rows, n_entries / kMxLdsRow), by_memory), (uint64_t)(n_cu > 0 ? n_cu : 1) * 2);
}

hipError_t launch_mx_rows_wide(const NeedleCount* tmp, const uint64_t* offsets, uint32_t n_rows, uint64_t n_entries, const uint32_t* list, const uint32_t* ctr,
                               uint32_t n_needles, uint32_t* bits, uint32_t* pre, uint32_t grid, NeedleCount* out, hipStream_t st)
{
    if (grid == 0) return hipSuccess;
    const uint32_t words = (uint32_t)(((uint64_t)n_needles + 31) / 32);
    hipLaunchKernelGGL(k_mx_rows_wide, dim3(grid), dim3(kMxThreads), 0, st, tmp, offsets, n_rows, n_entries, list, ctr, n_needles, words, bits, pre, out);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace am
