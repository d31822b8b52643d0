// am_records.hip -- the small folds over the sorted records of a scan, each a direct use of the shared walk (am_records.h): Searcher.containsAll's bitmap rows
// (k_idset, k_idset_all -- also the slot rows of the rule sets), the fold checksum of a held result (k_fold_hash) and the per-haystack "a span is kept" flags of a
// select (k_hay_flags_spans).  The large folds have files of their own: am_hist.hip, am_matrix.hip, am_score.hip, am_spans.hip.
#include <hip/hip_runtime.h>

#include "am_bounds.h"
#include "am_device.h"
#include "am_records.h"
#include "am_wave.h"
#include "am_words.h"

AM_BOUNDS_TU("am_records.hip")

namespace am {
namespace dev {

namespace {
constexpr int kWave = 64;

// ---- a select's predicate over the records: one lane per record, the first of its values whose span the table keeps (span_of, am_words.h) flags the record's
// haystack, the remaining values are skipped (several lanes may store the same 1 into the same byte)
template <bool IC, bool WORDS, bool EXACT>
__global__ void __launch_bounds__(kRowThreads) k_hay_flags_spans(SpansIn in, uint8_t* __restrict__ flags)
{
    const uint64_t i = global_row();
    if (i >= in.n_rec) return;
    const Record r = in.recs[i];
    AM_BOUNDS(r.haystack < in.n_hay);
    if (r.haystack >= in.n_hay) return;
    uint64_t v0, v1;
    value_range(in, r, v0, v1);
    for (uint64_t k = v0; k < v1; k++) {
        const uint32_t v = in.vals[k];
        if (v >= in.n_needles) continue;                               // the am_needle_ids convention: skipped
        uint64_t s, n;
        if (!span_of<IC, WORDS, EXACT>(in, r, v, in.words, s, n)) continue;
        flags[r.haystack] = 1;
        return;
    }
}

}  // namespace

// ---- Searcher.containsAll (Searcher.hs:173-187) on the records: the IntSet of needle ids still missing, as one bitmap of `words` 32-bit words per haystack.
// k_idset sets the bit of every reported id, k_idset_all tests whether all n_needles bits of a haystack are set (IS.null of the final accumulator).
__global__ void __launch_bounds__(kRowThreads) k_idset(RecordsIn in, uint32_t hay0, uint32_t words, uint32_t* __restrict__ bits)
{
    const uint64_t r = global_row();
    if (r >= in.n_rec) return;
    const Record rec = in.recs[r];
    const uint32_t h = rec.haystack - hay0;                      // (a haystack below hay0 wraps to a row beyond in.n_hay)
    AM_BOUNDS(h < in.n_hay);
    if (h >= in.n_hay) return;
    uint32_t* row = bits + (uint64_t)h * words;
    uint64_t k, ke;
    value_range(in, rec, k, ke);
    for (; k < ke; k++) {
        const uint32_t id = in.vals[k];
        if (id >= in.n_needles) continue;                        // IS.delete of an absent key
        AM_BOUNDS((id >> 5) < words);
        const uint32_t m = 1u << (id & 31);
        if (!(row[id >> 5] & m)) atomicOr(row + (id >> 5), m);      // a stale read only costs an extra atomic
    }
}

__global__ void __launch_bounds__(kRowThreads) k_idset_all(const uint32_t* __restrict__ bits, uint32_t words, uint32_t n_needles, uint32_t n_hay, uint8_t* __restrict__ flags)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t h = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    if (h >= n_hay) return;
    const uint32_t* row = bits + (uint64_t)h * words;
    uint64_t c = 0;
    for (uint32_t w = lane; w < words; w += kWave) c += __popc(row[w]);
    c = wave_sum_u64(c);
    if (lane == 0) flags[h] = c == (uint64_t)n_needles ? 1 : 0;
}

hipError_t launch_idset(const RecordsIn& in, uint32_t hay0, uint32_t words, uint32_t* bits, hipStream_t st)
{
    return launch_rows(k_idset, in.n_hay ? in.n_rec : 0, st, in, hay0, words, bits);
}

hipError_t launch_idset_all(const uint32_t* bits, uint32_t words, uint32_t n_needles, uint32_t n_hay, uint8_t* flags, hipStream_t st)
{
    if (n_hay == 0) return hipSuccess;
    hipLaunchKernelGGL(k_idset_all, dim3((n_hay + 3) / 4), dim3(kRowThreads), 0, st, bits, words, n_needles, n_hay, flags);
    return hipGetLastError();
}

// ---- checksum of the fold sequence (SURVEY 8d "parity check at scale"): per haystack, the left fold
//   h' = h * P + mix(matchPos, value)      over every (record, value of machineValues ! record.state) in order
// i.e. exactly what the reference's runWithCase would hand to a fold function, reduced to 64 bits.  One wavefront per haystack: every lane folds a contiguous block of
// the haystack's records, the (hash, count) pairs are combined with (h1, c1) . (h2, c2) = (h1 * P^c2 + h2, c1 + c2).  EVERY value counts: there is no n_needles here.
constexpr uint64_t kFoldP = 0x100000001B3ull;
__device__ __forceinline__ uint64_t fold_mix(uint64_t pos, uint32_t v)
{
    uint64_t x = (pos * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)v + 0x632BE59BD9B4E019ull);
    x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32;
    return x;
}
__device__ __forceinline__ uint64_t fold_pow(uint64_t e)
{
    uint64_t r = 1, b = kFoldP;
    while (e) { if (e & 1) r *= b; b *= b; e >>= 1; }
    return r;
}
__global__ void __launch_bounds__(kRowThreads) k_fold_hash(RecordsIn in, const uint64_t* __restrict__ rec_first, uint64_t* __restrict__ hash_out, uint64_t* __restrict__ count_out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t h = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    if (h >= in.n_hay) return;
    uint64_t r0 = rec_first[h], r1 = rec_first[h + 1];
    AM_BOUNDS(r0 <= r1 && r1 <= in.n_rec);
    if (r1 > in.n_rec) r1 = in.n_rec;
    if (r0 > r1) r0 = r1;
    const uint64_t per = (r1 - r0 + kWave - 1) / kWave;
    uint64_t a = r0 + per * lane, z = a + per;
    if (a > r1) a = r1;
    if (z > r1) z = r1;
    uint64_t hh = 0, cnt = 0;
    for (uint64_t r = a; r < z; r++) {
        const Record rec = in.recs[r];
        uint64_t k, ke;
        value_range(in, rec, k, ke);
        for (; k < ke; k++) { hh = hh * kFoldP + fold_mix(rec.end_pos, in.vals[k]); cnt++; }
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {            // lanes whose index is a multiple of 2d absorb their right neighbour's block
        const uint64_t oh = __shfl_down(hh, d, kWave), oc = __shfl_down(cnt, d, kWave);
        hh = hh * fold_pow(oc) + oh; cnt += oc;
    }
    if (lane == 0) { hash_out[h] = hh; if (count_out) count_out[h] = cnt; }
}

hipError_t launch_fold_hash(const RecordsIn& in, const uint64_t* rec_first, uint64_t* hash_out, uint64_t* count_out, hipStream_t st)
{
    if (in.n_hay == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fold_hash, dim3((in.n_hay + 3) / 4), dim3(kRowThreads), 0, st, in, rec_first, hash_out, count_out);
    return hipGetLastError();
}

hipError_t launch_hay_flags_spans(bool ic, const SpansIn& in, uint8_t* flags, hipStream_t st)
{
    // (no predicate: no start is needed, so no case mode)
    const auto kernel = in.exact ? (in.words ? (ic ? k_hay_flags_spans<true, true, true> : k_hay_flags_spans<false, true, true>)
                                             : (ic ? k_hay_flags_spans<true, false, true> : k_hay_flags_spans<false, false, true>))
                                 : !in.words ? k_hay_flags_spans<false, false, false> : ic ? k_hay_flags_spans<true, true, false> : k_hay_flags_spans<false, true, false>;
    return launch_rows(kernel, in.n_rec, st, in, flags);
}

}  // namespace dev
}  // namespace am
