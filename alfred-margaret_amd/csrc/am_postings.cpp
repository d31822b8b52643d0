// am_postings.cpp -- postings on the device (include/am.h "postings"): the rows of a spans result ordered by needle, their row offsets per needle, the row each came
// from and the document frequencies; and one needle's row as a spans result of its own.  A stage over the rows of any am_spans result where they lie in HBM
// (am_postings.hip): the needle column and the identity into (key, index) pairs, per pass of the plan (am_postings.h) a count table, the library's exclusive sum
// over it and a stable scatter, then the gather of the 24-byte rows, the offsets and the document frequencies.  The result is CSR by NEEDLE -- CsrResult's rows are
// the N needles here, not the haystacks -- with two arrays beside it, and stays in HBM until asked for; its handle, the one-shot form and the argument checks are
// am_fold.h's.
// WORKSPACE of a call, freed when it returns: 16 bytes per span (two key and two index arrays that take turns) and per pass 12 bytes per digit value and tile (the
// uint32 counts and their uint64 bases).  What crosses to the host: nothing; am_spans_of_needle reads the two offsets of its row.
// Every argument is checked before any device work.
#include "am_postings.h"
#include "am_spans.h"

using namespace am;
using namespace am::dev;
using namespace am::host;

using SpansResult = struct am_spans;                        // (am_spans alone names the one-shot entry point)
using Postings = struct am_postings;                        // (as am_postings does)

// CsrResult's n_hay is the ROW count of this result: n_needles.  The haystack count of the spans it was made from is src_hay.
struct am_postings : am::host::CsrResult<am_span> {
    uint64_t src_hay = 0, src_total = 0;
    uint32_t n_needles = 0;
    int mode = AM_SPANS_ALL, unit = AM_UNIT_BYTES;
    DevBuf source, doc_freq;                                // uint64[n_items], uint64[n_needles] (none when there is no row)
    std::vector<uint64_t> h_source, h_doc_freq;
    bool source_fetched = false, doc_freq_fetched = false;
};

namespace {

using PostingsPtr = std::unique_ptr<Postings, void (*)(Postings*)>;
using SpansPtr = std::unique_ptr<SpansResult, void (*)(SpansResult*)>;

int check_modes(int case_mode, int spans_mode)
{
    AM_TRY(check_case(case_mode));
    if (spans_mode != AM_SPANS_ALL && spans_mode != AM_SPANS_LEFTMOST_LONGEST) return fail(AM_ERR_INVALID, "spans_mode must be AM_SPANS_ALL or AM_SPANS_LEFTMOST_LONGEST");
    return AM_OK;
}

// what the result remembers of the spans it was made from
void describe(Postings* p, int dev, uint64_t src_hay, uint64_t src_total, uint32_t n_needles, int mode, int unit)
{
    p->dev = dev; p->n_hay = n_needles; p->n_needles = n_needles;
    p->src_hay = src_hay; p->src_total = src_total; p->mode = mode; p->unit = unit;
}

// a result without rows: N + 1 zero offsets, N zero document frequencies, nothing in HBM
int no_rows(Postings* p)
{
    try {
        p->h_offsets.assign((size_t)p->n_needles + 1, 0);
        p->h_doc_freq.assign(std::max<size_t>(p->n_needles, 1), 0);
    } catch (const std::exception&) { return fail(AM_ERR_OOM, "no host memory for the postings' offsets"); }
    p->h_data.assign(1, am_span{}); p->h_source.assign(1, 0);
    p->n_items = 0;
    p->offsets_fetched = p->data_fetched = p->source_fetched = p->doc_freq_fetched = true;
    return AM_OK;
}

int check_spans(const SpansResult* s)
{
    if (s->n_items >= kPostMaxSpans) return fail(AM_ERR_UNSUPPORTED, "am_postings_from_spans: 2^32 - 1 spans and more (the sort carries 32-bit row indices)");
    if (s->n_items && !s->data.p) return fail(AM_ERR_UNSUPPORTED, "am_postings_from_spans: the spans were assembled on the host and have no rows in HBM");
    return AM_OK;
}

// the stage; every argument has been checked
int sort_by_needle(const SpansResult* s, Postings** out)
{
    AM_TRY(ensure_runtime());
    PostingsPtr p(new Postings(), am_postings_free);
    describe(p.get(), s->dev, s->n_hay, s->src_total, s->n_needles, s->mode, s->unit);
    const uint64_t n = s->n_items, N = s->n_needles;
    if (n == 0) { AM_TRY(no_rows(p.get())); *out = p.release(); return AM_OK; }
    ON_DEVICE(s->dev);
    hipStream_t st; AM_TRY(get_stream(s->dev, &st));
    const PostPlan plan = post_plan(N);
    const uint64_t n_tiles = post_tiles(n);
    uint64_t cells = 0;
    for (uint32_t k = 0; k < plan.passes; k++) cells = std::max<uint64_t>(cells, (uint64_t)post_digits(plan, k) * n_tiles);
    DevBuf keys[2], idx[2], counts, base, scan_tmp;
    AM_TRY(keys[0].ensure(n * 4));
    AM_TRY(idx[0].ensure(n * 4));
    if (plan.passes) {
        AM_TRY(keys[1].ensure(n * 4));
        AM_TRY(idx[1].ensure(n * 4));
        AM_TRY(counts.ensure(cells * 4));
        AM_TRY(base.ensure(cells * 8));
    }
    AM_TRY(p->data.ensure(n * sizeof(Span)));
    AM_TRY(p->source.ensure(n * 8));
    AM_TRY(p->offsets.ensure((N + 1) * 8));
    AM_TRY(p->doc_freq.ensure(N * 8));
    p->n_items = n;
    const Span* spans = (const Span*)s->data.p;
    { Prof pr("post_keys", st);
      HIP_TRY(launch_post_keys(spans, n, (uint32_t*)keys[0].p, (uint32_t*)idx[0].p, st)); }
    uint32_t cur = 0;
    for (uint32_t k = 0; k < plan.passes; k++, cur ^= 1u) {
        const uint64_t pass_cells = (uint64_t)post_digits(plan, k) * n_tiles;
        { Prof pr("post_hist", st);
          HIP_TRY(launch_post_hist(plan, k, (const uint32_t*)keys[cur].p, n, (uint32_t*)counts.p, st)); }
        { Prof pr("post_scan", st);
          AM_TRY(exclusive_sum(scan_tmp, (const uint32_t*)counts.p, (uint64_t*)base.p, pass_cells, st)); }      // (pass 0 has the most cells: the temporary never moves)
        { Prof pr("post_scatter", st);
          HIP_TRY(launch_post_scatter(plan, k, (const uint32_t*)keys[cur].p, (const uint32_t*)idx[cur].p, n, (const uint64_t*)base.p, (uint32_t*)keys[cur ^ 1u].p,
                                      (uint32_t*)idx[cur ^ 1u].p, st)); }
    }
    { Prof pr("post_gather", st);
      HIP_TRY(launch_post_gather(spans, (const uint32_t*)idx[cur].p, n, (Span*)p->data.p, (uint64_t*)p->source.p, st)); }
    { Prof pr("post_offsets", st);
      HIP_TRY(launch_post_offsets((const uint32_t*)keys[cur].p, n, N, (uint64_t*)p->offsets.p, st)); }
    HIP_TRY(hipMemsetAsync(p->doc_freq.p, 0, N * 8, st));
    { Prof pr("post_df", st);
      HIP_TRY(launch_post_df((const Span*)p->data.p, (const uint32_t*)keys[cur].p, n, N, (uint64_t*)p->doc_freq.p, st)); }
    HIP_TRY(hipStreamSynchronize(st));                      // (the workspaces are freed; a result may be used from any thread and stream afterwards)
    *out = p.release();
    return AM_OK;
}

}  // namespace

extern "C" int am_postings_from_spans(const SpansResult* s, Postings** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!s) return fail(AM_ERR_INVALID, "null spans");
    AM_TRY(check_spans(s));
    return sort_by_needle(s, out);
}

extern "C" int am_postings_batch(const am_span_table* t, int case_mode, int spans_mode, const am_batch* b, Postings** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_modes(case_mode, spans_mode));
    if (!t || !b) return fail(AM_ERR_INVALID, "null span table or batch");
    if (t->ids->a->dev != b->dev) return fail(AM_ERR_INVALID, "span table and batch live on different devices");
    SpansResult* raw = nullptr;
    AM_TRY(am_spans_batch(t, case_mode, spans_mode, b, &raw));
    SpansPtr s(raw, am_spans_free);
    AM_TRY(check_spans(s.get()));
    return sort_by_needle(s.get(), out);
}

extern "C" int am_postings(const am_span_table* t, int case_mode, int spans_mode, const am_slice* hay, size_t n_hay, Postings** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_slices(hay, n_hay));
    AM_TRY(check_modes(case_mode, spans_mode));
    if (!t) return fail(AM_ERR_INVALID, "null span table");      // (last: a caller without a device can see every other check)
    AM_TRY(ensure_runtime());                               // (the table is not looked at before)
    if (n_hay == 0) {
        PostingsPtr p(new Postings(), am_postings_free);
        describe(p.get(), t->ids->a->dev, 0, 0, t->ids->n_needles, spans_mode, AM_UNIT_BYTES);
        AM_TRY(no_rows(p.get()));
        *out = p.release();
        return AM_OK;
    }
    return with_oneshot_batch(t->ids->a->dev, hay, n_hay, [&](am_batch* b) { return am_postings_batch(t, case_mode, spans_mode, b, out); });
}

extern "C" uint64_t am_postings_size(const Postings* p) { return p ? p->n_items : 0; }
extern "C" uint64_t am_postings_needles(const Postings* p) { return p ? p->n_needles : 0; }
extern "C" uint64_t am_postings_haystacks(const Postings* p) { return p ? p->src_hay : 0; }
extern "C" const void* am_postings_device_offsets(const Postings* p) { return p && p->n_items ? p->offsets.p : nullptr; }
extern "C" const void* am_postings_device_data(const Postings* p) { return p && p->n_items ? p->data.p : nullptr; }
extern "C" const void* am_postings_device_source(const Postings* p) { return p && p->n_items ? p->source.p : nullptr; }
extern "C" const void* am_postings_device_doc_freq(const Postings* p) { return p && p->n_items ? p->doc_freq.p : nullptr; }

extern "C" const uint64_t* am_postings_offsets(Postings* p)
{
    if (!p) { fail(AM_ERR_INVALID, "null postings"); return nullptr; }
    return p->fetch_offsets("the postings' offsets");
}

extern "C" const am_span* am_postings_data(Postings* p)
{
    if (!p) { fail(AM_ERR_INVALID, "null postings"); return nullptr; }
    return p->fetch_data("the postings");
}

extern "C" const uint64_t* am_postings_source(Postings* p)
{
    if (!p) { fail(AM_ERR_INVALID, "null postings"); return nullptr; }
    return fetch_once(p->h_source, p->source_fetched, p->dev, p->source, p->n_items, "the postings' source rows");
}

extern "C" const uint64_t* am_postings_doc_freq(Postings* p)
{
    if (!p) { fail(AM_ERR_INVALID, "null postings"); return nullptr; }
    return fetch_once(p->h_doc_freq, p->doc_freq_fetched, p->dev, p->doc_freq, p->n_needles, "the document frequencies");
}

extern "C" void am_postings_free(Postings* p)
{
    if (!p) return;
    OnDevice od(p->dev);
    delete p;
}

extern "C" int am_spans_of_needle(const Postings* p, uint32_t needle, SpansResult** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!p) return fail(AM_ERR_INVALID, "null postings");
    if (needle >= p->n_needles) return fail(AM_ERR_INVALID, "am_spans_of_needle: needle is not below the postings' needle count");
    AM_TRY(ensure_runtime());
    SpansPtr r(new SpansResult(), am_spans_free);
    r->mode = p->mode; r->n_needles = p->n_needles; r->src_total = p->src_total; r->unit = p->unit;
    if (p->src_hay == 0) { r->make_empty(p->dev); *out = r.release(); return AM_OK; }
    r->dev = p->dev; r->n_hay = p->src_hay;
    ON_DEVICE(p->dev);
    hipStream_t st; AM_TRY(get_stream(p->dev, &st));
    AM_TRY(r->offsets.ensure((p->src_hay + 1) * 8));
    uint64_t row[2] = {0, 0};                               // the two words that cross
    if (p->n_items) {
        HIP_TRY(hipMemcpyAsync(row, (const uint64_t*)p->offsets.p + needle, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (row[0] > row[1] || row[1] > p->n_items) return fail(AM_ERR_HIP, "am_spans_of_needle: the row's offsets are out of range");
    }
    const uint64_t n_row = row[1] - row[0];
    if (n_row == 0) {
        HIP_TRY(hipMemsetAsync(r->offsets.p, 0, (p->src_hay + 1) * 8, st));
    } else {
        AM_TRY(r->data.ensure(n_row * sizeof(Span)));
        r->n_items = n_row;
        HIP_TRY(hipMemcpyAsync(r->data.p, (const Span*)p->data.p + row[0], n_row * sizeof(Span), hipMemcpyDeviceToDevice, st));
        Prof pr("post_row_offsets", st);
        HIP_TRY(launch_post_row_offsets((const Span*)r->data.p, n_row, p->src_hay, (uint64_t*)r->offsets.p, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    *out = r.release();
    return AM_OK;
}

extern "C" void am_postings_geometry(uint64_t n_needles, uint32_t* tile_spans, uint32_t* wave_spans, uint32_t* passes, uint32_t* bits)
{
    const PostPlan plan = post_plan(n_needles > 0xFFFFFFFFull ? 0xFFFFFFFFull : n_needles);
    if (tile_spans) *tile_spans = kPostTileSpans;
    if (wave_spans) *wave_spans = kPostWaveSpans;
    if (passes) *passes = plan.passes;
    if (bits) for (uint32_t k = 0; k < kPostMaxPasses; k++) bits[k] = k < plan.passes ? plan.bits[k] : 0;
}
