// am_spans.h -- the two handles of include/am.h "match spans" that am_spans.cpp makes and am_subst.cpp reads: the needles' lengths beside machineValues, and the
// CSR result of a spans call with what the splice checks it against.  Internal: nothing here is part of the C ABI.
#pragma once
#include "am_host.h"

struct am_span_table {
    const am_needle_ids* ids = nullptr;
    am::host::DevBuf len_bytes, len_cps;                    // uint32[n_needles] each, on the automaton's device
    bool has_words = false;                                 // am_span_table_create_words: every consumer of the table sees the whole-word spans only
    uint8_t word_bytes[256] = {};                           // the class as the caller gave it, 0 / 1
    am::host::DevBuf words;                                 // ... and as the kernels read it: 8 dwords beside the lengths (am_words.h)
    const uint32_t* d_words() const { return has_words ? (const uint32_t*)words.p : nullptr; }
    bool has_exact = false;                                 // am_span_table_create_cased with a spelling: a handle that has one is a row only where the text spells it so
    std::vector<uint64_t> exact_off;                        // the spellings as the caller gave them (am_span_table_exact): n_needles + 1 offsets into exact_bytes
    std::vector<uint8_t> exact_bytes;
    am::host::DevBuf exact_refs, exact_pool;                // ... and as the kernels read them: ExactRef[n_needles], and the pool in groups of 16 bytes (am_cased.h)
    const am::dev::ExactRef* d_exact() const { return has_exact ? (const am::dev::ExactRef*)exact_refs.p : nullptr; }
    bool has_predicate() const { return has_words || has_exact; }      // no predicate: every span is a row, and the folds over the values alone say the same
};

namespace am {
namespace host {
// what the kernels that turn records into spans read: records [0, n_rec) of a scan of `scanned`, whose haystacks count from 0 there, under table t
inline am::dev::SpansIn spans_in(const am_span_table* t, const am::dev::Record* recs, uint64_t n_rec, const am_batch* scanned, uint32_t n_hay)
{
    return {records_in(t->ids, recs, n_rec, n_hay), (const uint32_t*)t->len_bytes.p, (const uint32_t*)t->len_cps.p, (const uint8_t*)scanned->d_text, scanned->d_offsets,
            scanned->total, t->d_words(), t->d_exact(), t->has_exact ? (const uint8_t*)t->exact_pool.p : nullptr};
}
// d_flags[h] = 1 iff row h of am_spans_batch(t, case_mode, AM_SPANS_ALL, b) is not empty, in bounded record memory (am_contains_all.cpp, beside the whole-word counts)
int spans_flags(const am_span_table* t, int case_mode, am_batch* b, uint8_t* d_flags);
}  // namespace host
}  // namespace am

struct am_spans : am::host::CsrResult<am_span> {
    uint32_t rounds = 0;                                    // pointer-doubling rounds of the call
    int mode = AM_SPANS_ALL;                                // what am_batch_substitute holds a result to: the selection, the table's handles and the batch it was made from
    uint32_t n_needles = 0;
    uint64_t src_total = 0;
    int unit = AM_UNIT_BYTES;                               // what start / len are in; anything else: made by am_coords_spans, refused by the stages that read byte spans
};
