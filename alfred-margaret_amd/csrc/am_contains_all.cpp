// am_contains_all.cpp -- what is folded over the records with machineValues in flat form (am_needle_ids), on the device: Searcher.containsAll
// (Searcher.hs:167-187), the fold checksum of a result, the per-needle match counts (am_count_by_needle*) and the per-haystack needle counts (am_count_matrix*).
// The argument checks, the segment loop of the one-shot entry points (fold_slices) and the matrix's result handle are am_fold.h's, shared with the other folds.
#include "am_host.h"
#include "am_spans.h"

#include <memory>
#include <string>
#include <thread>
#include <vector>

using namespace am;
using namespace am::dev;
using namespace am::host;

// ------------------------------------------------------------------ Searcher.containsAll (Searcher.hs:167-187)

extern "C" int am_needle_ids_create(const am_automaton* a, const uint64_t* values_offsets, const uint32_t* values, uint32_t n_needles, am_needle_ids** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!a) return fail(AM_ERR_INVALID, "null automaton");
    AM_TRY(ensure_runtime());
    ON_DEVICE(a->dev);
    // a handle attached to a received image (multi-GPU ranks) has no reference arrays: the state count comes from the image
    uint64_t n_states = 0;
    if (a->has_ref) n_states = a->offsets.size() - 1;
    else {
        std::lock_guard<std::mutex> lk(const_cast<am_automaton*>(a)->mu);
        for (const Flavor& f : a->fl) if (f.ready) n_states = f.h.n_states;
        if (!n_states) return fail(AM_ERR_INVALID, "automaton handle has no image");
    }
    if (!values_offsets || values_offsets[0] != 0) return fail(AM_ERR_INVALID, "values_offsets[0] must be 0");
    for (uint64_t s = 0; s < n_states; s++)
        if (values_offsets[s + 1] < values_offsets[s] || (a->has_ref && values_offsets[s + 1] - values_offsets[s] != a->values_len[s]))
            return fail(AM_ERR_INVALID, "values_offsets disagrees with the values_len given to am_automaton_create");
    const uint64_t n_values = values_offsets[n_states];
    if (n_values && !values) return fail(AM_ERR_INVALID, "values is null");
    am_needle_ids* ids = new am_needle_ids();
    ids->a = a; ids->n_needles = n_needles; ids->n_states = n_states; ids->n_values = n_values;
    int rc = ids->vals_off.ensure((n_states + 1) * 8);
    if (rc == AM_OK) rc = ids->vals.ensure(n_values * 4 + 4);
    if (rc == AM_OK && hipMemcpy(ids->vals_off.p, values_offsets, (n_states + 1) * 8, hipMemcpyHostToDevice) != hipSuccess) rc = fail(AM_ERR_HIP, "upload failed");
    if (rc == AM_OK && n_values && hipMemcpy(ids->vals.p, values, n_values * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail(AM_ERR_HIP, "upload failed");
    if (rc != AM_OK) { delete ids; return rc; }
    *out = ids;
    return AM_OK;
}

extern "C" void am_needle_ids_destroy(am_needle_ids* ids) { delete ids; }

// The slot rows of a batch by the direct route (round 5): the scan itself sets the bit of every needle id it reports -- no record is written -- and a haystack whose
// row is full is not looked at any further (`Done`, Searcher.hs:181; a full row cannot grow).  The per-haystack "row is full" flags go to the sink.  *taken = false:
// the call did not go this way (the general kernel, the empty needle's dense pass, nothing to scan) and the caller folds the records instead.
static int direct_rows(const am_needle_ids* ids, int case_mode, am_batch* b, uint32_t* d_bits, uint32_t words, uint32_t* d_missing, FlagSink& sink, bool* taken)
{
    *taken = false;
    return scan_needle_ids(ids->a, case_mode, b, (const uint64_t*)ids->vals_off.p, (const uint32_t*)ids->vals.p, ids->n_needles, d_bits, words, d_missing, sink, taken);
}

// containsAll with the flags left in HBM: the sink decides what becomes of them (am_contains_all_batch: the copy to the caller; a select: the compaction)
int am::host::contains_all_flags(const am_needle_ids* ids, int case_mode, am_batch* b, FlagSink& sink)
{
    const uint32_t n_hay = b->n_hay;
    AM_TRY(sink.begin(b));
    if (ids->n_needles == 0) return n_hay ? sink.constant(1) : AM_OK;      // IS.null of the empty set (Searcher.hs:176,184)
    if (n_hay == 0) return AM_OK;
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    DevBuf records, rec_first, bits, flags;
    const uint32_t words = (ids->n_needles + 31) / 32;
    // The direct route (direct_rows): one bitmap row per haystack, up to 8 GiB of them; wider batches, the general kernel and automata with the empty needle fold
    // the records (below).
    if ((uint64_t)n_hay * words * 4 <= (8ull << 30) && !cfg::on(cfg::kNoIdsScan)) {
        AM_TRY(bits.ensure((uint64_t)n_hay * words * 4 + 64));
        AM_TRY(flags.ensure((size_t)n_hay * 4 + 64));                  // (here: the haystacks' missing-id counters)
        bool taken = false;
        AM_TRY(direct_rows(ids, case_mode, b, (uint32_t*)bits.p, words, (uint32_t*)flags.p, sink, &taken));
        if (taken) return AM_OK;
    }
    uint64_t n_rec = 0;
    AM_TRY(run_records(ids->a, case_mode, b, records_into(records), &n_rec));
    if (n_rec == 0) return sink.constant(0);
    // one bitmap row per haystack; very wide batches go through in groups of haystacks (records are sorted by haystack)
    const uint64_t budget = 1ull << 30;
    const uint32_t group = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_hay, budget / ((uint64_t)words * 4)));
    AM_TRY(rec_first.ensure(((uint64_t)n_hay + 1) * 8));
    AM_TRY(bits.ensure((uint64_t)group * words * 4));
    AM_TRY(flags.ensure(n_hay));
    HIP_TRY(launch_rp_ranges((const Record*)records.p, n_rec, (uint64_t*)rec_first.p, kNoRoute, n_hay, st));
    std::vector<uint64_t> first;
    if (group < n_hay) {
        first.resize((size_t)n_hay + 1);
        HIP_TRY(hipMemcpyAsync(first.data(), rec_first.p, first.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (uint32_t h0 = 0; h0 < n_hay; h0 += group) {
        const uint32_t h1 = std::min<uint64_t>(n_hay, (uint64_t)h0 + group);
        const uint64_t r0 = first.empty() ? 0 : first[h0], r1 = first.empty() ? n_rec : first[h1];
        HIP_TRY(hipMemsetAsync(bits.p, 0, (uint64_t)(h1 - h0) * words * 4, st));
        { Prof pr("idset", st);
          HIP_TRY(launch_idset(records_in(ids, (const Record*)records.p + r0, r1 - r0, h1 - h0), h0, words, (uint32_t*)bits.p, st));
          HIP_TRY(launch_idset_all((const uint32_t*)bits.p, words, ids->n_needles, h1 - h0, (uint8_t*)flags.p + h0, st)); }
    }
    return sink.device((const uint8_t*)flags.p, st);       // (returns when the copy or the compaction has finished: the workspaces are freed)
}

extern "C" int am_contains_all_batch(const am_needle_ids* ids, int case_mode, const am_batch* cb, uint8_t* flags_out)
{
    if (!ids || !cb) return fail(AM_ERR_INVALID, "null needle ids or batch");
    HostFlagSink sink(flags_out, false);
    return contains_all_flags(ids, case_mode, const_cast<am_batch*>(cb), sink);
}

extern "C" int am_matches_fold_hash(const am_matches* m, const am_needle_ids* ids, size_t n_hay, uint64_t* hash_out, uint64_t* count_out)
{
    if (!m || !ids) return fail(AM_ERR_INVALID, "null matches or values table");
    if (n_hay && !hash_out) return fail(AM_ERR_INVALID, "hash_out is null");
    if (n_hay >= 0xFFFFFFFFull) return fail(AM_ERR_INVALID, "too many haystacks");
    if (n_hay == 0) return AM_OK;
    AM_TRY(matches_in_hbm(m, ids, "am_matches_fold_hash"));
    AM_TRY(ensure_runtime());
    ON_DEVICE(m->dev);
    hipStream_t st; AM_TRY(get_stream(m->dev, &st));
    DevBuf rec_first, out, dummy;
    AM_TRY(rec_first.ensure((n_hay + 1) * 8));
    AM_TRY(out.ensure(n_hay * 16));
    AM_TRY(dummy.ensure(sizeof(Record)));
    const Record* recs = m->n ? m->d_records + m->first : (const Record*)dummy.p;
    HIP_TRY(launch_rp_ranges(recs, m->n, (uint64_t*)rec_first.p, kNoRoute, (uint32_t)n_hay, st));
    { Prof pr("fold_hash", st);
      HIP_TRY(launch_fold_hash(records_in(ids, recs, m->n, (uint32_t)n_hay), (const uint64_t*)rec_first.p, (uint64_t*)out.p, (uint64_t*)out.p + n_hay, st)); }
    HIP_TRY(hipMemcpyAsync(hash_out, out.p, n_hay * 8, hipMemcpyDeviceToHost, st));
    if (count_out) HIP_TRY(hipMemcpyAsync(count_out, (uint64_t*)out.p + n_hay, n_hay * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return AM_OK;
}

extern "C" int am_contains_all(const am_needle_ids* ids, int case_mode, const am_slice* hay, size_t n_hay, uint8_t* flags_out)
{
    if (!ids) return fail(AM_ERR_INVALID, "null needle ids");
    ON_DEVICE(ids->a->dev);
    am_batch* b = nullptr;
    AM_TRY(am_batch_upload(hay, n_hay, &b));
    const int rc = am_contains_all_batch(ids, case_mode, b, flags_out);
    am_batch_destroy(b);
    return rc;
}

// ------------------------------------------------------------------ per-needle match counts (term frequencies)
// counts[v] = how often runWithCase (Automaton.hs:442-553) hands `Match _ v` to the fold function, over the whole batch: the records of a scan are expanded
// through the value lists and summed into uint64[n_needles] in HBM by k_needle_hist (am_hist.hip).  No record crosses the wire; the record array of a scan
// is bounded: a batch whose records would exceed the budget is scanned in groups of whole consecutive haystacks, each group folded before the next (integer
// adds commute: the same counts).

namespace {

constexpr uint64_t kHistRecordBudget = 1ull << 30;       // bytes of records in HBM at a time (64 Mi records; natural text: ~400 MiB of haystacks a group)
uint64_t hist_budget() { const long v = cfg::get(cfg::kHistRecordsMiB); return v > 0 ? (uint64_t)v << 20 : kHistRecordBudget; }

std::atomic<uint64_t> g_hist_trace[3];                   // AM_HIST_TRACE: sums of the launches' trace words (am_debug_hist_adds)
uint32_t hist_flush_tiles() { const long v = cfg::get(cfg::kHistFlushTiles); return v > 0 ? (uint32_t)std::min<long>(v, 1L << 30) : 0u; }      // (0: the kernels' own interval)

int needle_hist(const RecordsIn& in, uint64_t* d_counts, uint64_t* d_trace, int dev, hipStream_t st)
{
    Prof pr("needle_hist", st);
    HIP_TRY(launch_needle_hist(in, d_counts, d_trace, hist_flush_tiles(), g_rt.dev[dev].n_cu, st));
    return AM_OK;
}

// one scan of `b` (haystacks h0 ... of the caller's batch), its records handed to `fold`; returns when the fold has finished (the record array is free again)
int fold_scan(const am_needle_ids* ids, int case_mode, am_batch* b, RecordArray& ra, uint32_t h0, const RecordFold& fold)
{
    uint64_t n_rec = 0;
    AM_TRY(run_records(ids->a, case_mode, b, records_into(ra), &n_rec));
    if (n_rec == 0) return AM_OK;
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    AM_TRY(fold((const Record*)ra.p, n_rec, h0, b->n_hay, b, b->dev, st));
    HIP_TRY(hipStreamSynchronize(st));
    return AM_OK;
}

}  // namespace

// a device-resident batch scanned and folded in bounded record memory (am_host.h): in one piece, or in groups of whole consecutive haystacks (am_count_by_needle*,
// am_count_matrix*, the slot rows, the whole-word flags and am_score* share this loop)
int am::host::fold_batch(const am_needle_ids* ids, int case_mode, am_batch* b, const RecordFold& fold)
{
    if (b->n_hay == 0 || b->total == 0) return AM_OK;
    ON_DEVICE(b->dev);                                     // (segments are folded on threads of their own)
    RecordArray ra(b->dev);
    const uint64_t budget = hist_budget();
    // a record per end position at most (and one more per haystack where the empty needle reports position 0): small batches need no count pass
    if ((b->total + b->n_hay) * sizeof(Record) <= budget || b->n_hay == 1) return fold_scan(ids, case_mode, b, ra, 0, fold);
    // the count pass: values per haystack (>= its records: every record carries at least one value)
    std::vector<uint64_t> per(b->n_hay);
    uint64_t total_values = 0;
    AM_TRY(am_count_batch(ids->a, case_mode, b, per.data(), &total_values));
    if (total_values == 0) return AM_OK;
    if (total_values * sizeof(Record) <= budget) return fold_scan(ids, case_mode, b, ra, 0, fold);
    // groups of whole consecutive haystacks, each a batch of its own (sub_batch, am_fold.h)
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    std::vector<uint64_t> offs((size_t)b->n_hay + 1);
    HIP_TRY(hipMemcpyAsync(offs.data(), b->d_offsets, offs.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    DerivedBatch sub;                                       // ONE batch: its buffers serve group after group
    sub.begin(b->dev);
    for (uint32_t h0 = 0; h0 < b->n_hay;) {
        uint32_t h1 = h0; uint64_t values = 0;
        while (h1 < b->n_hay && (h1 == h0 || (values + per[h1]) * sizeof(Record) <= budget)) values += per[h1++];      // (a haystack beyond the budget by itself: a group of one)
        const uint64_t bytes = offs[h1] - offs[h0];
        if (values != 0 && bytes != 0) {
            AM_TRY(sub_batch(b, h0, h1, offs[h0], offs[h1], sub, st));
            AM_TRY(fold_scan(ids, case_mode, sub.b.get(), ra, h0, fold));
        }
        h0 = h1;
    }
    return AM_OK;
}

namespace {

// the counts of a device-resident batch into d_counts (accumulating)
int hist_batch(const am_needle_ids* ids, int case_mode, am_batch* b, uint64_t* d_counts, uint64_t* d_trace)
{
    return fold_batch(ids, case_mode, b, [&](const Record* recs, uint64_t n_rec, uint32_t, uint32_t n_hay, const am_batch*, int dev, hipStream_t st) {
        return needle_hist(records_in(ids, recs, n_rec, n_hay), d_counts, d_trace, dev, st);
    });
}

// the same over the whole-word spans of a table with a word class (am_count_spans_by_needle*): the predicate reads the text and the offsets of the batch the records
// index, which is the group's sub-batch where fold_batch made groups
int hist_words_batch(const am_span_table* t, int case_mode, am_batch* b, uint64_t* d_counts, uint64_t* d_trace)
{
    return fold_batch(t->ids, case_mode, b, [&](const Record* recs, uint64_t n_rec, uint32_t, uint32_t n_hay, const am_batch* scanned, int dev, hipStream_t st) {
        Prof pr("needle_hist_words", st);
        HIP_TRY(launch_needle_hist_words(case_mode == AM_IGNORE_CASE, spans_in(t, recs, n_rec, scanned, n_hay), d_counts, d_trace, hist_flush_tiles(), g_rt.dev[dev].n_cu, st));
        return AM_OK;
    });
}

// the histogram of a call in HBM: n_needles counts + the three trace words, cleared; read back at the end
struct HistOut {
    DevBuf buf; uint32_t n = 0; bool trace = false;
    int begin(uint32_t n_needles, hipStream_t st)
    {
        n = n_needles; trace = cfg::on(cfg::kHistTrace);
        AM_TRY(buf.ensure(((size_t)n + 4) * 8));
        HIP_TRY(hipMemsetAsync(buf.p, 0, ((size_t)n + 4) * 8, st));
        HIP_TRY(hipStreamSynchronize(st));                   // (segments are folded on other threads' streams)
        return AM_OK;
    }
    uint64_t* counts() { return (uint64_t*)buf.p; }
    uint64_t* trace_words() { return trace ? (uint64_t*)buf.p + n : nullptr; }
    int finish(uint64_t* counts_out, hipStream_t st)
    {
        uint64_t tw[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(counts_out, buf.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        if (trace) HIP_TRY(hipMemcpyAsync(tw, (uint64_t*)buf.p + n, sizeof(tw), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < 3; i++) g_hist_trace[i].fetch_add(tw[i], std::memory_order_relaxed);
        return AM_OK;
    }
};

}  // namespace

// the slot rows of a batch (am_host.h): what am_rules_eval_batch evaluates.  The direct route keeps its flags to itself here; the record route is k_idset under
// fold_batch, a group's records into the rows of the group's haystacks
int am::host::slot_rows(const am_needle_ids* ids, int case_mode, am_batch* b, uint32_t* d_bits, uint32_t words, uint32_t* d_missing)
{
    if (b->n_hay == 0 || words == 0) return AM_OK;
    struct NoSink : FlagSink {
        int begin(const am_batch*) override { return AM_OK; }
        // called with b->mu held: the scan writes the batch's scratch (its flags, its unit ticket), so it has finished before the lock goes -- another thread's
        // call on the same batch clears that scratch on a stream of its own
        int device(const uint8_t*, hipStream_t st) override { HIP_TRY(hipStreamSynchronize(st)); return AM_OK; }
        int constant(uint8_t) override { return AM_OK; }
    } none;
    bool taken = false;
    if (!cfg::on(cfg::kNoIdsScan)) AM_TRY(direct_rows(ids, case_mode, b, d_bits, words, d_missing, none, &taken));
    if (taken) return AM_OK;
    {
        ON_DEVICE(b->dev);
        hipStream_t st; AM_TRY(get_stream(b->dev, &st));
        HIP_TRY(hipMemsetAsync(d_bits, 0, (uint64_t)b->n_hay * words * 4, st));
        HIP_TRY(hipStreamSynchronize(st));                  // (as HistOut::begin: the folds follow on this thread's stream, the scans synchronise in between)
    }
    return fold_batch(ids, case_mode, b, [&](const Record* recs, uint64_t n_rec, uint32_t h0, uint32_t n_hay, const am_batch*, int, hipStream_t st) {
        Prof pr("idset", st);
        HIP_TRY(launch_idset(records_in(ids, recs, n_rec, n_hay), 0, words, d_bits + (uint64_t)h0 * words, st));
        return AM_OK;
    });
}

// am_select_spans_batch's predicate (am_select.cpp): d_flags[h] = 1 for every haystack whose AM_SPANS_ALL row under table t is not empty; d_flags = b->n_hay bytes in
// HBM that this call clears.  Scanned and folded in bounded record memory like the whole-word counts above: k_hay_flags_spans reads the text and the offsets of the
// batch the records index, which is the group's sub-batch where fold_batch made groups, and flags the group's haystacks at d_flags + h0.
int am::host::spans_flags(const am_span_table* t, int case_mode, am_batch* b, uint8_t* d_flags)
{
    const am_needle_ids* ids = t->ids;
    if (b->n_hay == 0) return AM_OK;
    {
        ON_DEVICE(b->dev);
        hipStream_t st; AM_TRY(get_stream(b->dev, &st));
        HIP_TRY(hipMemsetAsync(d_flags, 0, b->n_hay, st));
        HIP_TRY(hipStreamSynchronize(st));                  // (as HistOut::begin: the folds follow on this thread's stream, the scans synchronise in between)
    }
    if (ids->n_needles == 0) return AM_OK;
    return fold_batch(ids, case_mode, b, [&](const Record* recs, uint64_t n_rec, uint32_t h0, uint32_t n_hay, const am_batch* scanned, int, hipStream_t st) {
        Prof pr("hay_flags_spans", st);
        HIP_TRY(launch_hay_flags_spans(case_mode == AM_IGNORE_CASE, spans_in(t, recs, n_rec, scanned, n_hay), d_flags + h0, st));
        return AM_OK;
    });
}

extern "C" int am_debug_hist_adds(uint64_t* out3)
{
    for (int i = 0; i < 3; i++) { const uint64_t v = g_hist_trace[i].exchange(0, std::memory_order_relaxed); if (out3) out3[i] = v; }
    return AM_OK;
}

// the counts of a device-resident batch to the caller, behind the checks both *_batch entry points make once their handles are known not to be null; handle: what the
// entry point's message calls its own ("needle ids"); fold(b, d_counts, d_trace): hist_batch or hist_words_batch
template <class Fold>
static int count_batch(const am_needle_ids* ids, const char* handle, int case_mode, const am_batch* cb, uint64_t* counts_out, Fold&& fold)
{
    if (ids->n_needles && !counts_out) return fail(AM_ERR_INVALID, "counts_out is null");
    AM_TRY(check_case(case_mode));
    if (ids->a->dev != cb->dev) return fail(AM_ERR_INVALID, std::string(handle) + " and batch live on different devices");
    if (ids->n_needles == 0) return AM_OK;
    AM_TRY(ensure_runtime());
    am_batch* b = const_cast<am_batch*>(cb);
    if (b->n_hay == 0 || b->total == 0) { std::memset(counts_out, 0, (size_t)ids->n_needles * 8); return AM_OK; }
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    HistOut out;
    AM_TRY(out.begin(ids->n_needles, st));
    AM_TRY(fold(b, out.counts(), out.trace_words()));
    return out.finish(counts_out, st);
}

extern "C" int am_count_by_needle_batch(const am_needle_ids* ids, int case_mode, const am_batch* cb, uint64_t* counts_out)
{
    if (!ids || !cb) return fail(AM_ERR_INVALID, "null needle ids or batch");
    return count_batch(ids, "needle ids", case_mode, cb, counts_out, [&](am_batch* b, uint64_t* d_counts, uint64_t* d_trace) { return hist_batch(ids, case_mode, b, d_counts, d_trace); });
}

extern "C" int am_count_spans_by_needle_batch(const am_span_table* t, int case_mode, const am_batch* cb, uint64_t* counts_out)
{
    if (!t || !cb) return fail(AM_ERR_INVALID, "null span table or batch");
    if (!t->has_predicate()) return am_count_by_needle_batch(t->ids, case_mode, cb, counts_out);      // no class, no spelling: every span is a row, the rows are the values
    return count_batch(t->ids, "span table", case_mode, cb, counts_out, [&](am_batch* b, uint64_t* d_counts, uint64_t* d_trace) { return hist_words_batch(t, case_mode, b, d_counts, d_trace); });
}

extern "C" int am_count_spans_by_needle(const am_span_table* t, int case_mode, const am_slice* hay, size_t n_hay, uint64_t* counts_out)
{
    uint64_t total = 0;
    AM_TRY(check_slices(hay, n_hay, &total));
    AM_TRY(check_case(case_mode));
    if (!t) return fail(AM_ERR_INVALID, "null span table");      // (last of the checks a caller without a device can see; n_needles is the table's)
    const am_needle_ids* ids = t->ids;
    if (ids->n_needles && !counts_out) return fail(AM_ERR_INVALID, "counts_out is null");
    if (!t->has_predicate()) return am_count_by_needle(ids, case_mode, hay, n_hay, counts_out);
    if (ids->n_needles == 0) return AM_OK;
    AM_TRY(ensure_runtime());
    if (total == 0) { std::memset(counts_out, 0, (size_t)ids->n_needles * 8); return AM_OK; }
    return with_oneshot_batch(ids->a->dev, hay, n_hay, [&](am_batch* b) { return am_count_spans_by_needle_batch(t, case_mode, b, counts_out); });
}

extern "C" int am_matches_count_by_needle(const am_matches* m, const am_needle_ids* ids, uint64_t* counts_out)
{
    if (!m || !ids) return fail(AM_ERR_INVALID, "null matches or values table");
    if (ids->n_needles && !counts_out) return fail(AM_ERR_INVALID, "counts_out is null");
    if (ids->n_needles == 0) return AM_OK;
    AM_TRY(matches_in_hbm(m, ids, "am_matches_count_by_needle"));
    AM_TRY(ensure_runtime());
    if (m->n == 0) { std::memset(counts_out, 0, (size_t)ids->n_needles * 8); return AM_OK; }
    ON_DEVICE(m->dev);
    hipStream_t st; AM_TRY(get_stream(m->dev, &st));
    HistOut out;
    AM_TRY(out.begin(ids->n_needles, st));
    // (a held result does not know how many haystacks its batch had: no bound on the haystack fields, which the histogram does not look at)
    AM_TRY(needle_hist(records_in(ids, m->d_records + m->first, m->n, UINT32_MAX), out.counts(), out.trace_words(), m->dev, st));
    return out.finish(counts_out, st);
}

extern "C" int am_count_by_needle(const am_needle_ids* ids, int case_mode, const am_slice* hay, size_t n_hay, uint64_t* counts_out)
{
    if (!ids) return fail(AM_ERR_INVALID, "null needle ids");
    uint64_t total = 0;
    AM_TRY(check_slices(hay, n_hay, &total));
    if (ids->n_needles && !counts_out) return fail(AM_ERR_INVALID, "counts_out is null");
    AM_TRY(check_case(case_mode));
    if (ids->n_needles == 0) return AM_OK;
    AM_TRY(ensure_runtime());
    if (total == 0) { std::memset(counts_out, 0, (size_t)ids->n_needles * 8); return AM_OK; }
    const int dev = ids->a->dev;
    ON_DEVICE(dev);
    hipStream_t st; AM_TRY(get_stream(dev, &st));
    // What the wire carries is the text, once (in one piece or in segments: fold_slices), and n_needles counts at the end.
    HistOut out;
    AM_TRY(out.begin(ids->n_needles, st));
    AM_TRY(fold_slices(dev, hay, n_hay, total, [&](am_batch* b, size_t) { return hist_batch(ids, case_mode, b, out.counts(), out.trace_words()); }));
    return out.finish(counts_out, st);
}

// ------------------------------------------------------------------ per-haystack needle counts: the term-document matrix (am_count_matrix*)
// The fold of am_count_by_needle run once PER HAYSTACK (Automaton.hs:442-553), as a CSR matrix in HBM: row i = the (needle, count) pairs of haystack i in ascending
// needle order.  The kernels are am_matrix.hip; the scans, the record budget and its groups of whole haystacks are fold_batch's, above.  Rows belong to
// haystacks and a group is whole haystacks: every group leaves a part {local offsets, entries with the batch's haystack index}, and the parts are appended at the end.

struct am_needle_matrix : CsrResult<am_needle_count> {};

static_assert(sizeof(am_needle_count) == sizeof(NeedleCount) && sizeof(NeedleCount) == 16, "am_needle_count and the kernels' NeedleCount are one layout");
static_assert(offsetof(am_needle_count, count) == 0 && offsetof(am_needle_count, needle) == 8 && offsetof(am_needle_count, haystack) == 12, "am_needle_count: offsets 0, 8, 12");

namespace {

struct MatrixBuild {
    struct Part { DevBuf offsets, data; uint32_t h0 = 0, n = 0; uint64_t entries = 0; };
    const am_needle_ids* ids;
    std::vector<std::unique_ptr<Part>> parts;             // in haystack order: groups and segments arrive one after the other
    explicit MatrixBuild(const am_needle_ids* i) : ids(i) {}

    // the rows of haystacks [h0, h0 + n) from their records (haystack fields relative to h0)
    int fold(const Record* recs, uint64_t n_rec, uint32_t h0, uint32_t n, int dev, hipStream_t st)
    {
        if (n_rec == 0 || n == 0 || ids->n_needles == 0) return AM_OK;
        const int n_cu = g_rt.dev[dev].n_cu;
        const RecordsIn in = records_in(ids, recs, n_rec, n);
        DevBuf ctr, row_entries, scan_tmp, keys, cnts, tmp, list, bits, pre;
        AM_TRY(ctr.ensure(64));                             // [0] u64: values of the group; words 2, 3: rows for k_mx_rows_lds / k_mx_rows_wide
        AM_TRY(row_entries.ensure(((size_t)n + 1) * 4));
        HIP_TRY(hipMemsetAsync(ctr.p, 0, 64, st));
        HIP_TRY(hipMemsetAsync(row_entries.p, 0, ((size_t)n + 1) * 4, st));
        { Prof pr("mx_values", st);
          HIP_TRY(launch_mx_values(in, (uint64_t*)ctr.p, n_cu, st)); }
        uint64_t values = 0;
        HIP_TRY(hipMemcpyAsync(&values, ctr.p, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (values == 0) return AM_OK;
        // distinct keys <= values, and <= rows x needles (`a, aa, aaa` over one haystack: three)
        const uint64_t keys_max = (uint64_t)n <= values / ids->n_needles ? (uint64_t)n * ids->n_needles : values;
        const uint64_t cap = keys_max + keys_max / 2 + 64;
        AM_TRY(keys.ensure(cap * 8));
        AM_TRY(cnts.ensure(cap * 8));
        HIP_TRY(hipMemsetAsync(keys.p, 0xFF, cap * 8, st));
        HIP_TRY(hipMemsetAsync(cnts.p, 0, cap * 8, st));
        { Prof pr("mx_combine", st);
          HIP_TRY(launch_mx_combine(in, (uint64_t*)keys.p, (uint64_t*)cnts.p, cap, (uint32_t*)row_entries.p, n_cu, st)); }
        std::unique_ptr<Part> part(new Part());
        part->h0 = h0; part->n = n;
        AM_TRY(part->offsets.ensure(((size_t)n + 1) * 8));
        AM_TRY(exclusive_sum(scan_tmp, (const uint32_t*)row_entries.p, (uint64_t*)part->offsets.p, (uint64_t)n + 1, st, &part->entries));
        const uint64_t n_ent = part->entries;
        if (n_ent == 0) return AM_OK;                       // (every handle was beyond the table)
        if (n_ent > keys_max) return fail(AM_ERR_HIP, "am_count_matrix: more entries than the group's table was sized for");
        AM_TRY(tmp.ensure(n_ent * sizeof(NeedleCount)));
        AM_TRY(part->data.ensure(n_ent * sizeof(NeedleCount)));
        AM_TRY(list.ensure((size_t)n * 4));
        uint32_t* const rows_ctr = (uint32_t*)ctr.p + 2;
        { Prof pr("mx_scatter", st);
          HIP_TRY(launch_mx_scatter((const uint64_t*)keys.p, (const uint64_t*)cnts.p, cap, (const uint64_t*)part->offsets.p, (uint32_t*)row_entries.p, n, h0,
                                    (NeedleCount*)tmp.p, n_ent, n_cu, st)); }
        { Prof pr("mx_rows", st);
          HIP_TRY(launch_mx_rows((const NeedleCount*)tmp.p, (const uint64_t*)part->offsets.p, n, n_ent, (NeedleCount*)part->data.p, (uint32_t*)list.p, rows_ctr, st)); }
        if (ids->n_needles > kMxWaveRow) {                  // (a row has at most n_needles entries)
            Prof pr("mx_rows_lds", st);
            HIP_TRY(launch_mx_rows_lds((const NeedleCount*)tmp.p, (const uint64_t*)part->offsets.p, n, n_ent, (const uint32_t*)list.p, rows_ctr, (NeedleCount*)part->data.p, n_cu, st));
        }
        if (const uint32_t grid = mx_wide_grid(n, n_ent, ids->n_needles, n_cu)) {
            const size_t words = ((size_t)ids->n_needles + 31) / 32;
            AM_TRY(bits.ensure(words * 4 * grid));
            AM_TRY(pre.ensure(words * 4 * grid));
            HIP_TRY(hipMemsetAsync(bits.p, 0, words * 4 * grid, st));
            Prof pr("mx_rows_wide", st);
            HIP_TRY(launch_mx_rows_wide((const NeedleCount*)tmp.p, (const uint64_t*)part->offsets.p, n, n_ent, (const uint32_t*)list.p, rows_ctr, ids->n_needles,
                                        (uint32_t*)bits.p, (uint32_t*)pre.p, grid, (NeedleCount*)part->data.p, st));
        }
        HIP_TRY(hipStreamSynchronize(st));                  // (the workspaces are freed, the records go back)
        parts.push_back(std::move(part));
        return AM_OK;
    }

    // the parts appended: offsets rebased by the entries before them, haystacks no part covers (nothing matched there) get empty rows
    int finish(int dev, uint64_t n_hay, hipStream_t st, am_needle_matrix** out)
    {
        if (n_hay == 0) return empty_result(dev, out);
        std::unique_ptr<am_needle_matrix, void (*)(am_needle_matrix*)> x(new am_needle_matrix(), am_needle_matrix_free);
        x->dev = dev; x->n_hay = n_hay;
        if (parts.size() == 1 && parts[0]->h0 == 0 && parts[0]->n == n_hay) {
            Part& p = *parts[0];
            std::swap(x->offsets.p, p.offsets.p); std::swap(x->offsets.cap, p.offsets.cap);
            std::swap(x->data.p, p.data.p); std::swap(x->data.cap, p.data.cap);
            x->n_items = p.entries;
            *out = x.release();
            return AM_OK;
        }
        uint64_t total = 0;
        for (const auto& p : parts) total += p->entries;
        AM_TRY(x->offsets.ensure((n_hay + 1) * 8));
        AM_TRY(x->data.ensure(total * sizeof(NeedleCount)));
        uint64_t* const offs = (uint64_t*)x->offsets.p;
        uint64_t h = 0, base = 0;
        for (const auto& p : parts) {
            if (p->h0 < h || (uint64_t)p->h0 + p->n > n_hay) return fail(AM_ERR_HIP, "am_count_matrix: the groups of haystacks are out of order");
            HIP_TRY(launch_offsets_rebase(nullptr, p->h0 - h, base, offs + h, st));
            HIP_TRY(launch_offsets_rebase((const uint64_t*)p->offsets.p, p->n, base, offs + p->h0, st));
            HIP_TRY(hipMemcpyAsync((NeedleCount*)x->data.p + base, p->data.p, p->entries * sizeof(NeedleCount), hipMemcpyDeviceToDevice, st));
            base += p->entries; h = (uint64_t)p->h0 + p->n;
        }
        HIP_TRY(launch_offsets_rebase(nullptr, n_hay + 1 - h, base, offs + h, st));
        HIP_TRY(hipStreamSynchronize(st));
        x->n_items = total;
        *out = x.release();
        return AM_OK;
    }
};

// the rows of batch `b`, whose first haystack is haystack `base` of the call, into mb
int matrix_batch(MatrixBuild& mb, const am_needle_ids* ids, int case_mode, am_batch* b, uint64_t base)
{
    if (ids->n_needles == 0) return AM_OK;
    return fold_batch(ids, case_mode, b, [&mb, base](const Record* recs, uint64_t n_rec, uint32_t h0, uint32_t n, const am_batch*, int dev, hipStream_t st) {
        return mb.fold(recs, n_rec, (uint32_t)(base + h0), n, dev, st);
    });
}

}  // namespace

extern "C" int am_debug_needle_matrix_limits(uint32_t* out4)
{
    if (!out4) return fail(AM_ERR_INVALID, "out4 is null");
    mx_limits(out4);
    return AM_OK;
}

extern "C" int am_count_matrix_batch(const am_needle_ids* ids, int case_mode, const am_batch* cb, am_needle_matrix** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!ids || !cb) return fail(AM_ERR_INVALID, "null needle ids or batch");
    AM_TRY(check_case(case_mode));
    if (ids->a->dev != cb->dev) return fail(AM_ERR_INVALID, "needle ids and batch live on different devices");
    AM_TRY(ensure_runtime());
    am_batch* b = const_cast<am_batch*>(cb);
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    MatrixBuild mb(ids);
    AM_TRY(matrix_batch(mb, ids, case_mode, b, 0));
    return mb.finish(b->dev, b->n_hay, st, out);
}

extern "C" int am_matches_count_matrix(const am_matches* m, const am_needle_ids* ids, size_t n_hay, am_needle_matrix** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!m || !ids) return fail(AM_ERR_INVALID, "null matches or values table");
    if (n_hay >= 0xFFFFFFFFull) return fail(AM_ERR_INVALID, "too many haystacks");
    AM_TRY(matches_in_hbm(m, ids, "am_matches_count_matrix"));
    AM_TRY(ensure_runtime());
    ON_DEVICE(m->dev);
    hipStream_t st; AM_TRY(get_stream(m->dev, &st));
    MatrixBuild mb(ids);
    AM_TRY(matches_below(m, n_hay, "am_matches_count_matrix", st));
    if (m->n) AM_TRY(mb.fold(m->d_records + m->first, m->n, 0, (uint32_t)n_hay, m->dev, st));
    return mb.finish(m->dev, n_hay, st, out);
}

extern "C" int am_count_matrix(const am_needle_ids* ids, int case_mode, const am_slice* hay, size_t n_hay, am_needle_matrix** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!ids) return fail(AM_ERR_INVALID, "null needle ids");
    uint64_t total = 0;
    AM_TRY(check_slices(hay, n_hay, &total));
    AM_TRY(check_case(case_mode));
    AM_TRY(ensure_runtime());
    const int dev = ids->a->dev;
    ON_DEVICE(dev);
    hipStream_t st; AM_TRY(get_stream(dev, &st));
    MatrixBuild mb(ids);
    // a segment's rows are built in HBM while the next segment goes up (fold_slices), and appended in order
    if (total != 0 && ids->n_needles != 0)
        AM_TRY(fold_slices(dev, hay, n_hay, total, [&](am_batch* b, size_t first) { return matrix_batch(mb, ids, case_mode, b, first); }));
    return mb.finish(dev, n_hay, st, out);
}

extern "C" uint64_t am_needle_matrix_size(const am_needle_matrix* x) { return x ? x->n_items : 0; }
extern "C" uint64_t am_needle_matrix_haystacks(const am_needle_matrix* x) { return x ? x->n_hay : 0; }
extern "C" const void* am_needle_matrix_device_offsets(const am_needle_matrix* x) { return x ? x->offsets.p : nullptr; }
extern "C" const void* am_needle_matrix_device_data(const am_needle_matrix* x) { return x ? x->data.p : nullptr; }

extern "C" const uint64_t* am_needle_matrix_offsets(am_needle_matrix* x)
{
    if (!x) { fail(AM_ERR_INVALID, "null matrix"); return nullptr; }
    return x->fetch_offsets("the matrix");
}

extern "C" const am_needle_count* am_needle_matrix_data(am_needle_matrix* x)
{
    if (!x) { fail(AM_ERR_INVALID, "null matrix"); return nullptr; }
    return x->fetch_data("the matrix");
}

extern "C" void am_needle_matrix_free(am_needle_matrix* x) { delete x; }
