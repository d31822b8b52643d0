// am_near_host.h -- the result handle of include/am.h "proximity" that am_near.cpp makes and am_select.cpp (am_select_near) reads, with the shared host / device
// definitions of am_near.h.  Internal: nothing here is part of the C ABI.
#pragma once
#include "am_near.h"
#include "am_spans.h"

// what am_near* leaves in HBM (am_near.cpp; am_select_near, am_select.cpp, reads it): the pairs as a CSR result, and -- am_rule_hits' layout -- query-major bitmaps
// and per-query counts; the host copies are made once, on first use.  Remembers the batch its spans were made from as am_selection does.
struct am_near_hits : am::host::CsrResult<am_near_pair> {
    uint64_t n_queries = 0, hay_words = 0, src_total = 0;
    am::host::DevBuf fired, counts;                         // uint64[n_queries][hay_words], uint64[n_queries] (none when there is no haystack or no query)
    std::vector<uint64_t> h_fired, h_counts;
    bool fired_fetched = false, counts_fetched = false;
};
