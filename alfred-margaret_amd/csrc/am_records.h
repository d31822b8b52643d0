// am_records.h -- the walk every fold over the records shares (device side): a record of a scan expanded through machineValues in flat form (RecordsIn, am_device.h),
// i.e. the values vals[vals_off[state] .. vals_off[state + 1]) of the record's state.  Every fold gets its list from value_range, one record at a time or -- load_records
// -- a tile of them with the loads issued together; only k_mx_values (am_matrix.hip), which sums the lists' lengths, reads vals_off itself.  What a fold does with a
// value (skip handles >= n_needles or look at every value, a budget by list index, a haystack that is out of range) stays the fold's own.
#pragma once
#include <hip/hip_runtime.h>

#include "am_bounds.h"
#include "am_device.h"

namespace am {
namespace dev {

constexpr uint32_t kNoHay = 0xFFFFFFFFu;                  // no haystack: indices are < n_hay <= 2^32 - 2

// the value list of record r as [v0, v1) of in.vals: v0 <= v1 <= in.n_values; empty when the state is out of range, or -- live = false -- for a record the caller
// has given up (nothing of the table is read).  Of r only the state is read, and before `live` is looked at: a caller that decides `live` from the record's
// haystack gets both fields with one 8-byte load, as the tile loaders did before they were one (profiles/r25_record_folds.md, Codegen: why `live` and HAY exist).
__device__ __forceinline__ void value_range(const RecordsIn& in, const Record& r, uint64_t& v0, uint64_t& v1, bool live = true)
{
    const uint32_t state = r.state;
    AM_BOUNDS(!live || state < in.n_states);
    v0 = v1 = 0;
    if ((state < in.n_states) & live) { v0 = in.vals_off[state]; v1 = in.vals_off[state + 1]; }
    AM_BOUNDS(v0 <= v1 && v1 <= in.n_values);
    if (v1 > in.n_values) v1 = in.n_values;
    if (v0 > v1) v0 = v1;
}

// PER records of a tile per lane -- first, first + stride, ... -- and their lists [k[u], ke[u]).  Unrolled: the PER record loads go out before the first list bounds
// are read.  An index beyond in.n_rec gives an empty list and a record of haystack kNoHay; with HAY so does a record whose haystack is not below in.n_hay.
template <uint32_t PER, bool HAY>
__device__ __forceinline__ void load_records(const RecordsIn& in, uint64_t first, uint64_t stride, Record (&rec)[PER], uint64_t (&k)[PER], uint64_t (&ke)[PER])
{
#pragma unroll
    for (uint32_t u = 0; u < PER; u++) {
        const uint64_t r = first + u * stride;
        k[u] = ke[u] = 0;
        rec[u].end_pos = 0; rec[u].haystack = kNoHay; rec[u].state = 0;
        if (r < in.n_rec) {
            rec[u] = in.recs[r];
            const bool live = !HAY || rec[u].haystack < in.n_hay;
            AM_BOUNDS(live);
            if (!live) rec[u].haystack = kNoHay;
            value_range(in, rec[u], k[u], ke[u], live);
        }
    }
}

}  // namespace dev
}  // namespace am
