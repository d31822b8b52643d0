// near.hpp -- host mirror of am_near_spans (include/am.h "proximity"): the sequential definition.  Over the leftmost-longest rows of a haystack (ascending, disjoint)
// every span of group_a is an anchor; a plain loop looks left and right for the nearest member of group_b in the same row, the smaller gap wins, a tie goes left,
// and a pair comes out where the gap is at most max_gap.  nearFold takes the spans as they are and touches no device.
#pragma once
#include <vector>

#include "spans.hpp"

namespace alfred_margaret {

struct NearHits {
    std::vector<uint64_t> offsets;                          // nHay + 1
    std::vector<am_near_pair> pairs;                        // rows ascending by (haystack, a, query); a and b index sp.spans
    uint64_t hayWords = 0;
    std::vector<uint64_t> fired;                            // [nQueries][hayWords], bit h % 64 of word h / 64; bits beyond nHay are zero
    std::vector<uint64_t> counts;                           // nQueries
};

inline void checkNearQueries(const std::vector<am_near_query>& queries)
{
    if (queries.size() > AM_NEAR_MAX_QUERIES) throw AmError(AM_ERR_INVALID, "nearFold: more queries than AM_NEAR_MAX_QUERIES");
    for (const am_near_query& q : queries) {
        if (q.group_a >= AM_NEAR_MAX_GROUPS || q.group_b >= AM_NEAR_MAX_GROUPS) throw AmError(AM_ERR_INVALID, "nearFold: a group index is not below AM_NEAR_MAX_GROUPS");
        if ((q.flags & ~AM_NEAR_ORDERED) != 0 || q.reserved != 0) throw AmError(AM_ERR_INVALID, "nearFold: unknown flags, or reserved is not 0");
    }
}

// sp: CSR rows of leftmost-longest spans; groupMask: one mask per needle handle (a span whose handle lies beyond it is in no group)
inline NearHits nearFold(const Spans& sp, const std::vector<uint32_t>& groupMask, const std::vector<am_near_query>& queries)
{
    checkNearQueries(queries);
    if (sp.offsets.empty() || sp.offsets[0] != 0 || sp.offsets.back() != sp.spans.size()) throw AmError(AM_ERR_INVALID, "nearFold: the offsets are not those of the spans");
    const size_t nHay = sp.offsets.size() - 1, nQ = queries.size();
    NearHits out;
    out.hayWords = (nHay + 63) / 64;
    out.fired.assign(nQ * out.hayWords, 0);
    out.counts.assign(nQ, 0);
    out.offsets.assign(nHay + 1, 0);
    auto inGroup = [&](uint64_t i, uint32_t g) { const uint32_t v = sp.spans[i].needle; return v < groupMask.size() && (groupMask[v] >> g & 1u) != 0; };
    for (size_t h = 0; h < nHay; h++) {
        const uint64_t lo = sp.offsets[h], hi = sp.offsets[h + 1];
        if (hi < lo) throw AmError(AM_ERR_INVALID, "nearFold: the offsets descend");
        for (uint64_t i = lo; i < hi; i++) {
            const am_span& a = sp.spans[i];
            for (size_t q = 0; q < nQ; q++) {
                const am_near_query& Q = queries[q];
                if (!inGroup(i, Q.group_a)) continue;
                bool hasP = false, hasN = false;
                uint64_t p = 0, n = 0;
                if (!(Q.flags & AM_NEAR_ORDERED))
                    for (uint64_t j = i; j-- > lo;)
                        if (inGroup(j, Q.group_b)) { hasP = true; p = j; break; }
                for (uint64_t j = i + 1; j < hi; j++)
                    if (inGroup(j, Q.group_b)) { hasN = true; n = j; break; }
                if (!hasP && !hasN) continue;
                const uint64_t gapP = hasP ? a.start - (sp.spans[p].start + sp.spans[p].len) : 0;
                const uint64_t gapN = hasN ? sp.spans[n].start - (a.start + a.len) : 0;
                const bool left = hasP && (!hasN || gapP <= gapN);
                const uint64_t gap = left ? gapP : gapN;
                if (gap > Q.max_gap) continue;
                out.pairs.push_back(am_near_pair{i, left ? p : n, gap, (uint32_t)h, (uint32_t)q});
                out.fired[q * out.hayWords + h / 64] |= 1ull << (h % 64);
                out.counts[q]++;
            }
        }
        out.offsets[h + 1] = out.pairs.size();
    }
    return out;
}

}  // namespace alfred_margaret
