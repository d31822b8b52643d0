// am_score.cpp -- scores on the device (include/am.h "scores"): a number per match, added up per haystack.  The fold `acc + weight v` of runWithCase (reference:
// src/Data/Text/AhoCorasick/Automaton.hs:442-553) over every haystack of a batch and up to AM_SCORE_MAX_COLUMNS weight columns at once: the records of a scan stay
// in HBM, k_score (am_score.hip) sums them by haystack -- they are sorted by haystack, so this is a segmented sum -- into int64[n_cols][n_hay], which stays in HBM
// until asked for.  The scans, the record budget and its groups of whole haystacks are fold_batch's (am_contains_all.cpp), the segments of the one-shot form are
// fold_slices' (am_fold.h): a group's or a segment's records add into the rows of its own haystacks, scores + h0.  am_scores_top_k is here; the two selects over a
// result, am_select_top_k and am_select_score, are am_select.cpp's and share topk_flags below.
// Every argument is checked before any device work.
#include "am_score.h"
#include "am_spans.h"

using namespace am;
using namespace am::dev;
using namespace am::host;

static_assert(sizeof(am_scored) == sizeof(Scored) && sizeof(Scored) == 16, "am_scored and the kernels' Scored are one layout");
static_assert(offsetof(am_scored, score) == 0 && offsetof(am_scored, haystack) == 8 && offsetof(am_scored, reserved) == 12, "am_scored: offsets 0, 8, 12");
static_assert(AM_SCORE_MAX_COLUMNS == kScoreMaxColumns, "AM_SCORE_MAX_COLUMNS is the kernels' limit");

namespace {

using ScoresPtr = std::unique_ptr<am_scores, void (*)(am_scores*)>;

// the result of a call over n_hay haystacks, every score zero; returns when the zeros are in place (segments are folded on other threads' streams)
int new_scores(const am_weights* w, uint64_t n_hay, uint64_t src_total, hipStream_t st, ScoresPtr& x)
{
    x.reset(new am_scores());
    x->dev = w->dev; x->n_hay = n_hay; x->src_total = src_total; x->n_cols = w->n_cols;
    const uint64_t n = (uint64_t)w->n_cols * n_hay;
    if (n == 0) { x->h_scores.assign(1, 0); x->fetched = true; return AM_OK; }      // no haystacks: nothing in HBM
    AM_TRY(x->scores.ensure(n * 8));
    HIP_TRY(hipMemsetAsync(x->scores.p, 0, n * 8, st));
    HIP_TRY(hipStreamSynchronize(st));
    return AM_OK;
}

// records [0, n_rec) of a scan of `scanned`, whose n_hay haystacks are haystacks first ... of the result.  t: a span table with a word class, or null
int score_records(const am_weights* w, const am_span_table* t, int case_mode, const Record* recs, uint64_t n_rec, uint64_t first, uint32_t n_hay, const am_batch* scanned,
                  am_scores* x, int dev, hipStream_t st)
{
    if (first + n_hay > x->n_hay) return fail(AM_ERR_HIP, "am_score: a group of haystacks lies beyond the result");
    const SpansIn in = t ? spans_in(t, recs, n_rec, scanned, n_hay) : SpansIn{records_in(w->ids, recs, n_rec, n_hay)};      // (no table: no class, only the records part is read)
    ScoreOut out{(const int64_t*)w->w.p, w->n_cols, w->n_needles, (unsigned long long*)x->scores.p + first, x->n_hay};
    Prof pr(t ? "score_words" : "score", st);
    HIP_TRY(launch_score(case_mode == AM_IGNORE_CASE, in, out, g_rt.dev[dev].n_cu, st));
    return AM_OK;
}

// batch b, whose haystack 0 is haystack `first` of the result, scanned and scored in bounded record memory
int score_batch_into(const am_weights* w, const am_span_table* t, int case_mode, am_batch* b, uint64_t first, am_scores* x)
{
    return fold_batch(w->ids, case_mode, b, [&](const Record* recs, uint64_t n_rec, uint32_t h0, uint32_t n_hay, const am_batch* scanned, int dev, hipStream_t st) {
        return score_records(w, t, case_mode, recs, n_rec, first + h0, n_hay, scanned, x, dev, st);
    });
}

// what am_score_batch and am_score_spans_batch do once their checks are made
int score_batch(const am_weights* w, const am_span_table* t, int case_mode, const am_batch* cb, am_scores** out)
{
    AM_TRY(ensure_runtime());
    am_batch* b = const_cast<am_batch*>(cb);
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    ScoresPtr x(nullptr, am_scores_free);
    AM_TRY(new_scores(w, b->n_hay, b->total, st, x));
    if (b->n_hay != 0 && w->n_needles != 0) AM_TRY(score_batch_into(w, t, case_mode, b, 0, x.get()));
    HIP_TRY(hipStreamSynchronize(st));                      // (a result may be used from any thread and stream afterwards)
    *out = x.release();
    return AM_OK;
}

}  // namespace

extern "C" int am_weights_create(const am_needle_ids* ids, const int64_t* weights, uint32_t n_cols, am_weights** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (n_cols == 0 || n_cols > AM_SCORE_MAX_COLUMNS) return fail(AM_ERR_INVALID, "n_cols must be 1 .. AM_SCORE_MAX_COLUMNS");
    if (!ids) return fail(AM_ERR_INVALID, "null needle ids");
    AM_TRY(ensure_runtime());                               // (the last of what a caller without a device can see; the table is not looked at before)
    const uint64_t n = (uint64_t)n_cols * ids->n_needles;
    if (n && !weights) return fail(AM_ERR_INVALID, "weights is null");
    const int dev = ids->a->dev;
    ON_DEVICE(dev);
    std::unique_ptr<am_weights> w(new am_weights());
    w->ids = ids; w->dev = dev; w->n_cols = n_cols; w->n_needles = ids->n_needles;
    AM_TRY(w->w.ensure(n * 8 + 8));
    if (n) HIP_TRY(hipMemcpy(w->w.p, weights, n * 8, hipMemcpyHostToDevice));
    *out = w.release();
    return AM_OK;
}

extern "C" void am_weights_destroy(am_weights* w)
{
    if (!w) return;
    OnDevice od(w->dev);
    delete w;
}

extern "C" int am_score_batch(const am_weights* w, int case_mode, const am_batch* cb, am_scores** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_case(case_mode));
    if (!w || !cb) return fail(AM_ERR_INVALID, "null weights or batch");
    if (w->dev != cb->dev) return fail(AM_ERR_INVALID, "weights and batch live on different devices");
    return score_batch(w, nullptr, case_mode, cb, out);
}

extern "C" int am_score_spans_batch(const am_span_table* t, const am_weights* w, int case_mode, const am_batch* cb, am_scores** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_case(case_mode));
    if (!t || !w || !cb) return fail(AM_ERR_INVALID, "null span table, weights or batch");
    if (t->ids != w->ids) return fail(AM_ERR_INVALID, "the span table and the weights were not made over the same needle ids");
    if (w->dev != cb->dev) return fail(AM_ERR_INVALID, "weights and batch live on different devices");
    return score_batch(w, t->has_predicate() ? t : nullptr, case_mode, cb, out);      // no class, no spelling: every span is a row, the rows are the values
}

extern "C" int am_score(const am_weights* w, int case_mode, const am_slice* hay, size_t n_hay, am_scores** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    uint64_t total = 0;
    AM_TRY(check_slices(hay, n_hay, &total));
    AM_TRY(check_case(case_mode));
    if (!w) return fail(AM_ERR_INVALID, "null weights");       // (last: a caller without a device can see every other check)
    AM_TRY(ensure_runtime());
    const int dev = w->dev;
    ON_DEVICE(dev);
    hipStream_t st; AM_TRY(get_stream(dev, &st));
    ScoresPtr x(nullptr, am_scores_free);
    AM_TRY(new_scores(w, n_hay, total, st, x));
    // what the wire carries is the text, once (in one piece or in segments: fold_slices); a segment's records add into the rows of its own haystacks
    if (total != 0 && w->n_needles != 0)
        AM_TRY(fold_slices(dev, hay, n_hay, total, [&](am_batch* b, size_t first) { return score_batch_into(w, nullptr, case_mode, b, first, x.get()); }));
    HIP_TRY(hipStreamSynchronize(st));
    *out = x.release();
    return AM_OK;
}

extern "C" int am_matches_score(const am_matches* m, const am_weights* w, size_t n_hay, am_scores** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!m || !w) return fail(AM_ERR_INVALID, "null matches or weights");
    if (n_hay >= 0xFFFFFFFFull) return fail(AM_ERR_INVALID, "too many haystacks");
    AM_TRY(matches_in_hbm(m, w->ids, "am_matches_score"));
    AM_TRY(ensure_runtime());
    ON_DEVICE(m->dev);
    hipStream_t st; AM_TRY(get_stream(m->dev, &st));
    AM_TRY(matches_below(m, n_hay, "am_matches_score", st));
    ScoresPtr x(nullptr, am_scores_free);
    AM_TRY(new_scores(w, n_hay, 0, st, x));
    x->src_total_known = false;                             // (a result does not remember the bytes of its batch: the selects hold such scores to the haystack count)
    if (m->n && n_hay && w->n_needles) AM_TRY(score_records(w, nullptr, AM_CASE_SENSITIVE, m->d_records + m->first, m->n, 0, (uint32_t)n_hay, nullptr, x.get(), m->dev, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out = x.release();
    return AM_OK;
}

extern "C" uint64_t am_scores_haystacks(const am_scores* x) { return x ? x->n_hay : 0; }
extern "C" uint64_t am_scores_columns(const am_scores* x) { return x ? x->n_cols : 0; }
extern "C" const void* am_scores_device_data(const am_scores* x) { return x && x->n_hay ? x->scores.p : nullptr; }

extern "C" const int64_t* am_scores_data(am_scores* x)
{
    if (!x) { fail(AM_ERR_INVALID, "null scores"); return nullptr; }
    return fetch_once(x->h_scores, x->fetched, x->dev, x->scores, (uint64_t)x->n_cols * x->n_hay, "the scores");
}

extern "C" void am_scores_free(am_scores* x)
{
    if (!x) return;
    OnDevice od(x->dev);
    delete x;
}

int am::host::topk_flags(const am_scores* x, uint32_t column, uint64_t k, int largest, TopkBuffers& work, uint8_t* d_flags, uint32_t* d_keep, hipStream_t st)
{
    const uint64_t n = x->n_hay;
    size_t tmp_bytes = 0;
    HIP_TRY(scan_temp_bytes(n + 1, &tmp_bytes));
    AM_TRY(work.state.ensure(sizeof(TopkState) + kTopkBins * 8));
    AM_TRY(work.tie.ensure((n + 1) * 4));
    AM_TRY(work.tie_rank.ensure((n + 1) * 8));
    AM_TRY(work.scan_tmp.ensure(tmp_bytes));
    static_assert(sizeof(TopkState) % 8 == 0, "the histogram follows the state");
    const TopkWork w{(TopkState*)work.state.p, (uint64_t*)((uint8_t*)work.state.p + sizeof(TopkState)), (uint32_t*)work.tie.p, (uint64_t*)work.tie_rank.p,
                     work.scan_tmp.p, work.scan_tmp.cap};
    Prof pr("topk_flags", st);
    HIP_TRY(launch_topk_flags(x->column(column), n, k, largest != 0, w, d_flags, d_keep, st));
    return AM_OK;
}

extern "C" int am_scores_top_k(am_scores* x, uint32_t column, uint64_t k, int largest, am_scored* out, uint64_t* n_out)
{
    if (!n_out) return fail(AM_ERR_INVALID, "n_out is null");
    *n_out = 0;
    if (!x) return fail(AM_ERR_INVALID, "null scores");
    if (column >= x->n_cols) return fail(AM_ERR_INVALID, "column is not below the number of columns");
    const uint64_t n = x->n_hay, kk = std::min<uint64_t>(k, n);
    if (kk == 0) return AM_OK;
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    AM_TRY(ensure_runtime());
    ON_DEVICE(x->dev);
    hipStream_t st; AM_TRY(get_stream(x->dev, &st));
    if (kk == n) {
        // every haystack is a winner: the column itself is what crosses (half of what the caller asked for)
        std::vector<int64_t> col;
        try { col.resize((size_t)n); } catch (const std::exception&) { return fail(AM_ERR_OOM, "no host memory for the column"); }
        HIP_TRY(hipMemcpyAsync(col.data(), x->column(column), n * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint64_t i = 0; i < n; i++) out[i] = am_scored{col[i], (uint32_t)i, 0};
    } else {
        TopkBuffers work;
        DevBuf keep, pos, winners;
        AM_TRY(keep.ensure((n + 1) * 4));
        AM_TRY(pos.ensure((n + 1) * 8));
        AM_TRY(winners.ensure(kk * sizeof(Scored)));
        AM_TRY(topk_flags(x, column, kk, largest, work, nullptr, (uint32_t*)keep.p, st));
        AM_TRY(exclusive_sum(work.scan_tmp, (const uint32_t*)keep.p, (uint64_t*)pos.p, n + 1, st));      // (after the ties' sum on the stream, which sized the temporary for n + 1)
        { Prof pr("topk_gather", st);
          HIP_TRY(launch_topk_gather(x->column(column), n, (const uint32_t*)keep.p, (const uint64_t*)pos.p, (Scored*)winners.p, kk, st)); }
        uint64_t kept = 0;
        HIP_TRY(hipMemcpyAsync(&kept, (const uint64_t*)pos.p + n, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out, winners.p, kk * sizeof(Scored), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (kept != kk) return fail(AM_ERR_HIP, "am_scores_top_k: the selection did not keep k haystacks");
    }
    // the winners cross the wire anyway: their final order is made here
    const bool lg = largest != 0;
    std::sort(out, out + kk, [lg](const am_scored& a, const am_scored& b) {
        const uint64_t ka = score_key(a.score, lg), kb = score_key(b.score, lg);
        return ka != kb ? ka > kb : a.haystack < b.haystack;
    });
    *n_out = kk;
    return AM_OK;
}

extern "C" void am_score_geometry(uint32_t* tile_records, uint32_t* topk_block_items) { score_geometry(tile_records, topk_block_items); }
