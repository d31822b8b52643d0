// am_select.cpp -- select on the device (include/am.h "select"): keep the haystacks of a batch that a predicate holds for, drop the rest, and hand the kept ones on
// as a batch of their own -- `grep -F -f needles`, `grep -v`, `grep -w` and "the lines that mention all of these terms" between two stages of a pipeline in HBM.
// The predicates are the library's own: the flags of the containsAny / containsAll scans, taken where the scans leave them (FlagSink, am_host.h), and the non-empty
// rows of AM_SPANS_ALL (spans_flags, am_contains_all.cpp), one rule of a rule-set result (am_select_rule over am_rules.cpp's am_rule_hits), and the best k or a range
// of one column of a scores result (am_select_top_k / am_select_score over am_score.cpp's am_scores; the flags are am_score.hip's).  The compaction by
// runs is am_select.hip's; the bytes move with am_split.hip's gather.  What crosses to the host during a *_batch select: the kept count, the run count and the kept
// bytes (one copy of three words), and whatever the scans read back themselves.
// Every argument is checked before any device work.
#include "am_near_host.h"

using namespace am;
using namespace am::dev;
using namespace am::host;

// which haystacks of a batch were kept: ascending source indices, their new offsets, and the runs the gather copies.  (Holds DevBufs: on the heap only.)
struct am_selection {
    int dev = 0;
    uint64_t n_src = 0, src_total = 0;                      // the batch it was made from (am_batch_from_selection checks both)
    uint64_t n_kept = 0, n_runs = 0, total = 0;
    DevBuf indices, new_off, run_src, run_dst;              // uint32[n_kept], uint64[n_kept + 1], uint64[n_runs + 1] each (none when n_src == 0)
    std::vector<uint32_t> h_indices; bool fetched = false;
};

namespace {

using SelectionPtr = std::unique_ptr<am_selection, void (*)(am_selection*)>;

constexpr uint64_t kOneLaunchSums = 1ull << 16;             // up to here the three exclusive sums take one launch (launch_scan_jobs), beyond it three launches each

// the compaction of n = b->n_hay > 0 flags in HBM (d_flags null: every flag is `constant`) into s; returns when the device has finished with the flags
int compact(const am_batch* b, const uint8_t* d_flags, uint8_t constant, int invert, hipStream_t st, am_selection* s)
{
    const uint64_t n = b->n_hay;
    DevBuf keep, run_head, klen, rank, run_rank, koff, scan_tmp;
    AM_TRY(keep.ensure((n + 1) * 4));
    AM_TRY(run_head.ensure((n + 1) * 4));
    AM_TRY(klen.ensure((n + 1) * 8));
    AM_TRY(rank.ensure((n + 1) * 8));
    AM_TRY(run_rank.ensure((n + 1) * 8));
    AM_TRY(koff.ensure((n + 1) * 8));
    { Prof pr("select_plan", st);
      HIP_TRY(launch_select_plan(d_flags, constant, invert ? 1u : 0u, b->d_offsets, n, b->total, (uint32_t*)keep.p, (uint32_t*)run_head.p, (uint64_t*)klen.p, st)); }
    if (n + 1 <= kOneLaunchSums) {
        ScanJobs jobs{}; jobs.n_jobs = 3;
        jobs.j[0] = ScanJob{(const uint32_t*)keep.p, nullptr, (uint64_t*)rank.p, n + 1, nullptr};
        jobs.j[1] = ScanJob{(const uint32_t*)run_head.p, nullptr, (uint64_t*)run_rank.p, n + 1, nullptr};
        jobs.j[2] = ScanJob{nullptr, (const uint64_t*)klen.p, (uint64_t*)koff.p, n + 1, nullptr};
        HIP_TRY(launch_scan_jobs(jobs, st));
    } else {
        AM_TRY(exclusive_sum(scan_tmp, (const uint32_t*)keep.p, (uint64_t*)rank.p, n + 1, st));      // (one temporary: its size depends on n + 1 alone)
        AM_TRY(exclusive_sum(scan_tmp, (const uint32_t*)run_head.p, (uint64_t*)run_rank.p, n + 1, st));
        AM_TRY(exclusive_sum64(scan_tmp, (const uint64_t*)klen.p, (uint64_t*)koff.p, n + 1, st));
    }
    uint64_t tail[3] = {0, 0, 0};                           // the three scalars that cross
    HIP_TRY(hipMemcpyAsync(&tail[0], (const uint64_t*)rank.p + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&tail[1], (const uint64_t*)run_rank.p + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&tail[2], (const uint64_t*)koff.p + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                      // (the flags have been read: the batch's scratch is free again)
    s->n_kept = tail[0]; s->n_runs = tail[1]; s->total = tail[2];
    if (s->n_kept > n || s->n_runs > s->n_kept || s->total > b->total) return fail(AM_ERR_HIP, "select: the compaction's sums are out of range");
    AM_TRY(s->indices.ensure(s->n_kept * 4));
    AM_TRY(s->new_off.ensure((s->n_kept + 1) * 8));
    AM_TRY(s->run_src.ensure((s->n_runs + 1) * 8));
    AM_TRY(s->run_dst.ensure((s->n_runs + 1) * 8));
    { Prof pr("select_emit", st);
      HIP_TRY(launch_select_emit((const uint32_t*)keep.p, (const uint32_t*)run_head.p, (const uint64_t*)rank.p, (const uint64_t*)run_rank.p, (const uint64_t*)koff.p,
                                 b->d_offsets, n, s->n_kept, s->n_runs, (uint32_t*)s->indices.p, (uint64_t*)s->new_off.p, (uint64_t*)s->run_src.p, (uint64_t*)s->run_dst.p, st)); }
    HIP_TRY(hipStreamSynchronize(st));                      // (the workspaces are freed; a selection may be used from any thread and stream afterwards)
    return AM_OK;
}

// the sink of a containsAny / containsAll scan that compacts the flags where the scan left them
struct SelectSink : FlagSink {
    const am_batch* b; int invert; am_selection* s;
    SelectSink(const am_batch* batch, int inv, am_selection* sel) : b(batch), invert(inv), s(sel) {}
    int begin(const am_batch*) override { return AM_OK; }
    int device(const uint8_t* d_flags, hipStream_t st) override { return compact(b, d_flags, 0, invert, st, s); }
    int constant(uint8_t v) override
    {
        ON_DEVICE(b->dev);
        hipStream_t st; AM_TRY(get_stream(b->dev, &st));
        return compact(b, nullptr, v, invert, st, s);
    }
};

SelectionPtr new_selection(const am_batch* b)
{
    SelectionPtr s(new am_selection(), am_selection_free);
    s->dev = b->dev; s->n_src = b->n_hay; s->src_total = b->total;
    if (b->n_hay == 0) { s->h_indices.assign(1, 0); s->fetched = true; }      // nothing to select from: nothing in HBM
    return s;
}

// the frame of the four *_batch selects: the checks in the order every one of them makes them, the selection, and fill(b, s) where there is a haystack to select from.
// handle: the entry point's own, looked at -- handle_dev() -- only once it and the batch are known not to be null; case_mode: null where the entry point takes none
// (am_select_flags)
template <class DevOf, class Fill>
int select_with(const void* handle, DevOf&& handle_dev, const int* case_mode, const am_batch* cb, am_selection** out, const char* null_msg, const char* dev_msg, Fill&& fill)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (case_mode) AM_TRY(check_case(*case_mode));
    if (!handle || !cb) return fail(AM_ERR_INVALID, null_msg);
    if (handle_dev() != cb->dev) return fail(AM_ERR_INVALID, dev_msg);
    AM_TRY(ensure_runtime());
    am_batch* b = const_cast<am_batch*>(cb);
    SelectionPtr s = new_selection(b);
    if (b->n_hay != 0) AM_TRY(fill(b, s.get()));
    *out = s.release();
    return AM_OK;
}

// a fill: the flags that write(d_flags, st) puts into n_hay bytes of the call's own (the scans of the groups use the batch's scratch), compacted
template <class Write>
int compact_written(const am_batch* b, int invert, am_selection* s, Write&& write)
{
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    DevBuf flags;
    AM_TRY(flags.ensure(b->n_hay));
    AM_TRY(write((uint8_t*)flags.p, st));
    return compact(b, (const uint8_t*)flags.p, 0, invert, st, s);
}

}  // namespace

extern "C" int am_select_any_batch(const am_automaton* a, int case_mode, int invert, const am_batch* cb, am_selection** out)
{
    return select_with(a, [&] { return a->dev; }, &case_mode, cb, out, "null automaton or batch", "automaton and batch live on different devices", [&](am_batch* b, am_selection* s) {
        SelectSink sink(b, invert, s);
        return contains_any_flags(a, case_mode, b, sink);
    });
}

extern "C" int am_select_all_batch(const am_needle_ids* ids, int case_mode, int invert, const am_batch* cb, am_selection** out)
{
    return select_with(ids, [&] { return ids->a->dev; }, &case_mode, cb, out, "null needle ids or batch", "needle ids and batch live on different devices", [&](am_batch* b, am_selection* s) {
        SelectSink sink(b, invert, s);
        return contains_all_flags(ids, case_mode, b, sink);
    });
}

extern "C" int am_select_spans_batch(const am_span_table* t, int case_mode, int invert, const am_batch* cb, am_selection** out)
{
    return select_with(t, [&] { return t->ids->a->dev; }, &case_mode, cb, out, "null span table or batch", "span table and batch live on different devices", [&](am_batch* b, am_selection* s) {
        return compact_written(b, invert, s, [&](uint8_t* d_flags, hipStream_t) { return spans_flags(t, case_mode, b, d_flags); });
    });
}

extern "C" int am_select_flags(const am_batch* cb, const uint8_t* host_flags, int invert, am_selection** out)
{
    // (the batch is its own handle; a batch with haystacks was made on a device, so the flags' check, made where there is a haystack, is behind no other failure)
    return select_with(cb, [&] { return cb->dev; }, nullptr, cb, out, "null batch", "", [&](am_batch* b, am_selection* s) -> int {
        if (!host_flags) return fail(AM_ERR_INVALID, "flags is null");
        return compact_written(b, invert, s, [&](uint8_t* d_flags, hipStream_t st) -> int {
            HIP_TRY(hipMemcpyAsync(d_flags, host_flags, b->n_hay, hipMemcpyHostToDevice, st));
            return AM_OK;
        });
    });
}

// the haystacks of one rule of a rule-set result (am_rules.cpp): its row of `fired`, or labels == rule, as byte flags (k_rule_flags), then the compaction every select
// shares.  src must be the batch the hits were made from: the hits remember haystack count, total bytes and device, as a selection does.
extern "C" int am_select_rule(const am_rule_hits* x, uint32_t rule, int which, int invert, const am_batch* src, am_selection** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (which != AM_RULE_FIRED && which != AM_RULE_FIRST) return fail(AM_ERR_INVALID, "which must be AM_RULE_FIRED or AM_RULE_FIRST");
    if (!x || !src) return fail(AM_ERR_INVALID, "null rule hits or batch");
    if (rule >= x->n_rules) return fail(AM_ERR_INVALID, "rule is not below the number of rules");
    if (x->n_hay != src->n_hay || x->src_total != src->total || x->dev != src->dev)
        return fail(AM_ERR_INVALID, "the rule hits were not made from a batch with this haystack count and size");
    AM_TRY(ensure_runtime());
    SelectionPtr s = new_selection(src);
    if (src->n_hay != 0)
        AM_TRY(compact_written(src, invert, s.get(), [&](uint8_t* d_flags, hipStream_t st) -> int {
            Prof pr("rule_flags", st);
            HIP_TRY(launch_rule_flags(which == AM_RULE_FIRED ? (const uint64_t*)x->fired.p + (uint64_t)rule * x->hay_words : nullptr, (const uint32_t*)x->labels.p, rule,
                                      x->n_hay, x->hay_words, d_flags, st));
            return AM_OK;
        }));
    *out = s.release();
    return AM_OK;
}

// the haystacks in which one query of a proximity result (am_near.cpp) has a pair: its row of `fired` as byte flags (k_rule_flags: the layout is am_rule_hits'),
// then the compaction.  src must be the batch the spans of the hits were made from.
extern "C" int am_select_near(const am_near_hits* x, uint32_t query, int invert, const am_batch* src, am_selection** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!x || !src) return fail(AM_ERR_INVALID, "null proximity hits or batch");
    if (query >= x->n_queries) return fail(AM_ERR_INVALID, "query is not below the number of queries");
    if (x->n_hay != src->n_hay || x->src_total != src->total || x->dev != src->dev)
        return fail(AM_ERR_INVALID, "the proximity hits were not made from a batch with this haystack count and size");
    AM_TRY(ensure_runtime());
    SelectionPtr s = new_selection(src);
    if (src->n_hay != 0)
        AM_TRY(compact_written(src, invert, s.get(), [&](uint8_t* d_flags, hipStream_t st) -> int {
            Prof pr("rule_flags", st);
            HIP_TRY(launch_rule_flags((const uint64_t*)x->fired.p + (uint64_t)query * x->hay_words, nullptr, query, x->n_hay, x->hay_words, d_flags, st));
            return AM_OK;
        }));
    *out = s.release();
    return AM_OK;
}

// the two selects over one column of a scores result (am_score.cpp): the checks both make, the selection, and -- where there is a haystack -- fill(s).  src must be
// the batch the scores were made from: the scores remember haystack count, total bytes and device, as a selection does.
template <class Fill>
static int select_scores(const am_scores* x, uint32_t column, const am_batch* src, am_selection** out, Fill&& fill)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!x || !src) return fail(AM_ERR_INVALID, "null scores or batch");
    if (column >= x->n_cols) return fail(AM_ERR_INVALID, "column is not below the number of columns");
    if (x->n_hay != src->n_hay || (x->src_total_known && x->src_total != src->total) || x->dev != src->dev)
        return fail(AM_ERR_INVALID, "the scores were not made from a batch with this haystack count and size");
    AM_TRY(ensure_runtime());
    SelectionPtr s = new_selection(src);
    if (src->n_hay != 0) AM_TRY(fill(s.get()));
    *out = s.release();
    return AM_OK;
}

// every flag of the selection is `v`
static int compact_constant(const am_batch* b, uint8_t v, am_selection* s)
{
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    return compact(b, nullptr, v, 0, st, s);
}

// the min(k, n_hay) best haystacks of a column: the radix select's flags (topk_flags, am_score.cpp: key > T, or key == T and among the first q ties), compacted
extern "C" int am_select_top_k(const am_scores* x, uint32_t column, uint64_t k, int largest, const am_batch* src, am_selection** out)
{
    return select_scores(x, column, src, out, [&](am_selection* s) -> int {
        if (k == 0 || k >= x->n_hay) return compact_constant(src, k == 0 ? 0 : 1, s);      // nothing, or everything: no key is looked at
        TopkBuffers work;                                   // (lives until the compaction has waited for the stream)
        return compact_written(src, 0, s, [&](uint8_t* d_flags, hipStream_t st) { return topk_flags(x, column, k, largest, work, d_flags, nullptr, st); });
    });
}

// lo <= score <= hi (lo > hi keeps nothing), or -- invert -- the others
extern "C" int am_select_score(const am_scores* x, uint32_t column, int64_t lo, int64_t hi, int invert, const am_batch* src, am_selection** out)
{
    return select_scores(x, column, src, out, [&](am_selection* s) -> int {
        return compact_written(src, invert, s, [&](uint8_t* d_flags, hipStream_t st) -> int {
            Prof pr("score_range", st);
            HIP_TRY(launch_score_range(x->column(column), x->n_hay, lo, hi, d_flags, st));
            return AM_OK;
        });
    });
}

extern "C" int am_select_any(const am_automaton* a, int case_mode, int invert, const am_slice* hay, size_t n_hay, am_selection** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_slices(hay, n_hay));
    AM_TRY(check_case(case_mode));
    if (!a) return fail(AM_ERR_INVALID, "null automaton");      // (last: a caller without a device can see every other check)
    AM_TRY(ensure_runtime());                               // (the last of what a caller without a device can see; the handle is not looked at before)
    return with_oneshot_batch(a->dev, hay, n_hay, [&](am_batch* b) { return am_select_any_batch(a, case_mode, invert, b, out); });
}

extern "C" int am_select_all(const am_needle_ids* ids, int case_mode, int invert, const am_slice* hay, size_t n_hay, am_selection** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_slices(hay, n_hay));
    AM_TRY(check_case(case_mode));
    if (!ids) return fail(AM_ERR_INVALID, "null needle ids");
    AM_TRY(ensure_runtime());
    return with_oneshot_batch(ids->a->dev, hay, n_hay, [&](am_batch* b) { return am_select_all_batch(ids, case_mode, invert, b, out); });
}

extern "C" uint64_t am_selection_size(const am_selection* s) { return s ? s->n_kept : 0; }
extern "C" uint64_t am_selection_source_haystacks(const am_selection* s) { return s ? s->n_src : 0; }
extern "C" uint64_t am_selection_total_bytes(const am_selection* s) { return s ? s->total : 0; }
extern "C" const void* am_selection_device_indices(const am_selection* s) { return s && s->n_kept ? s->indices.p : nullptr; }

extern "C" const uint32_t* am_selection_indices(am_selection* s)
{
    if (!s) { fail(AM_ERR_INVALID, "null selection"); return nullptr; }
    return fetch_once(s->h_indices, s->fetched, s->dev, s->indices, s->n_kept, "the selection's indices");
}

extern "C" void am_selection_free(am_selection* s)
{
    if (!s) return;
    OnDevice od(s->dev);
    delete s;
}

extern "C" int am_batch_from_selection(const am_batch* src, const am_selection* s, am_batch** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!src || !s) return fail(AM_ERR_INVALID, "null batch or selection");
    if (s->n_src != src->n_hay || s->src_total != src->total || s->dev != src->dev)
        return fail(AM_ERR_INVALID, "the selection was not made from a batch with this haystack count and size");
    AM_TRY(ensure_runtime());
    if (s->n_kept == 0) return DerivedBatch::empty(src->dev, out);
    ON_DEVICE(src->dev);
    hipStream_t st; AM_TRY(get_stream(src->dev, &st));
    DerivedBatch nb;
    nb.begin(src->dev);
    uint64_t* new_off; uint8_t* new_text;
    AM_TRY(nb.offsets(s->n_kept, &new_off));
    HIP_TRY(hipMemcpyAsync(new_off, s->new_off.p, (s->n_kept + 1) * 8, hipMemcpyDeviceToDevice, st));
    AM_TRY(nb.text(s->total, st, &new_text));
    { Prof pr("select_gather", st);
      HIP_TRY(launch_split_gather((const uint8_t*)src->d_text, src->total, (const uint64_t*)s->run_src.p, (const uint64_t*)s->run_dst.p, s->n_runs, s->total, new_text,
                                  g_rt.dev[src->dev].n_cu, st)); }
    HIP_TRY(hipStreamSynchronize(st));                      // a batch object may be used from any thread and stream afterwards
    return nb.publish(s->total, s->n_kept, out);
}

extern "C" void am_select_geometry(uint32_t* tile_bytes, uint32_t* scan_block_items)
{
    if (tile_bytes) *tile_bytes = split_gather_tile_bytes();
    if (scan_block_items) *scan_block_items = scan_tile_items();
}
