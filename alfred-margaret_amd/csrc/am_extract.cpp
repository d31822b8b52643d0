// am_extract.cpp -- extract on the device (include/am.h "extract"): the matched text with some characters around it, handed on as a batch -- `grep -o`, a keyword-in-
// context concordance, the snippets of a search front end.  am_fragments_from_spans is the stage alone, between am_spans and am_fragments (am_extract.hip: the window
// of every span by a walk over aligned 16-byte groups, and the union of overlapping windows); am_extract_batch / am_extract put am_spans_batch in front of it and
// am_batch_from_fragments behind it.  A window is a fragment of its haystack, so the result type and the gather are the Splitter's.  What crosses to the host during
// the stage: the piece count (AM_EXTRACT_MERGED only).  Every argument is checked before any device work.
#include "am_spans.h"

using namespace am;
using namespace am::dev;
using namespace am::host;

namespace {

using FragmentsPtr = std::unique_ptr<am_fragments, void (*)(am_fragments*)>;
using SpansPtr = std::unique_ptr<struct am_spans, void (*)(struct am_spans*)>;

constexpr uint64_t kOneLaunchSum = 1ull << 16;              // up to here the exclusive sum of the heads takes one launch (launch_scan_jobs)

int check_extract_mode(int mode)
{
    return mode == AM_EXTRACT_EACH || mode == AM_EXTRACT_MERGED ? AM_OK : fail(AM_ERR_INVALID, "mode must be AM_EXTRACT_EACH or AM_EXTRACT_MERGED");
}

// what the two entry points in front of am_spans_batch check of their modes before they look at a handle
int check_route(int case_mode, int spans_mode, int mode)
{
    AM_TRY(check_case(case_mode));
    if (spans_mode != AM_SPANS_ALL && spans_mode != AM_SPANS_LEFTMOST_LONGEST) return fail(AM_ERR_INVALID, "spans_mode must be AM_SPANS_ALL or AM_SPANS_LEFTMOST_LONGEST");
    AM_TRY(check_extract_mode(mode));
    if (mode == AM_EXTRACT_MERGED && spans_mode != AM_SPANS_LEFTMOST_LONGEST)
        return fail(AM_ERR_INVALID, "AM_EXTRACT_MERGED takes AM_SPANS_LEFTMOST_LONGEST spans only (overlapping spans do not ascend by window)");
    return AM_OK;
}

int check_stage(const am_batch* src, const struct am_spans* s, int mode)
{
    AM_TRY(check_extract_mode(mode));
    if (!src || !s) return fail(AM_ERR_INVALID, "null batch or spans");
    if (s->unit != AM_UNIT_BYTES) return fail(AM_ERR_INVALID, "am_fragments_from_spans: the spans are in converted units (am_coords_spans); the windows are cut from byte spans");
    if (mode == AM_EXTRACT_MERGED && s->mode != AM_SPANS_LEFTMOST_LONGEST)
        return fail(AM_ERR_INVALID, "am_fragments_from_spans: AM_EXTRACT_MERGED takes an AM_SPANS_LEFTMOST_LONGEST result only (overlapping spans do not ascend by window)");
    if (s->n_hay != src->n_hay || s->src_total != src->total || s->dev != src->dev)
        return fail(AM_ERR_INVALID, "the spans were not produced from a batch with this haystack count and size");
    return AM_OK;
}

// the stage; every argument has been checked
int windows(const am_batch* src, const struct am_spans* s, uint32_t before, uint32_t after, int mode, am_fragments** out)
{
    AM_TRY(ensure_runtime());
    if (src->n_hay == 0) return empty_result(src->dev, out);
    FragmentsPtr f(new am_fragments(), am_fragments_free);
    f->dev = src->dev; f->n_hay = src->n_hay; f->src_total = src->total;
    ON_DEVICE(src->dev);
    hipStream_t st; AM_TRY(get_stream(src->dev, &st));
    const uint64_t n_span = s->n_items, n_hay = src->n_hay;
    const Span* spans = (const Span*)s->data.p;
    const uint64_t* span_off = (const uint64_t*)s->offsets.p;
    DevBuf ws, we, head, rank, scan_tmp;                    // AM_EXTRACT_MERGED's workspace: 28 bytes per span, freed on return
    AM_TRY(f->offsets.ensure((n_hay + 1) * 8));
    if (n_span == 0) {                                      // n_hay empty rows
        HIP_TRY(hipMemsetAsync(f->offsets.p, 0, (n_hay + 1) * 8, st));
    } else if (mode == AM_EXTRACT_EACH) {                   // fragment k belongs to span k: the spans' own rows
        f->n_items = n_span;
        AM_TRY(f->data.ensure(n_span * sizeof(Fragment)));
        { Prof pr("extract_windows", st);
          HIP_TRY(launch_extract_windows(spans, n_span, (const uint8_t*)src->d_text, src->d_offsets, src->n_hay, src->total, before, after, (Fragment*)f->data.p, nullptr, nullptr, st)); }
        HIP_TRY(hipMemcpyAsync(f->offsets.p, span_off, (n_hay + 1) * 8, hipMemcpyDeviceToDevice, st));
    } else {
        AM_TRY(ws.ensure(n_span * 8));
        AM_TRY(we.ensure(n_span * 8));
        AM_TRY(head.ensure((n_span + 1) * 4));
        AM_TRY(rank.ensure((n_span + 1) * 8));
        { Prof pr("extract_windows", st);
          HIP_TRY(launch_extract_windows(spans, n_span, (const uint8_t*)src->d_text, src->d_offsets, src->n_hay, src->total, before, after, nullptr, (uint64_t*)ws.p, (uint64_t*)we.p, st)); }
        { Prof pr("extract_heads", st);
          HIP_TRY(launch_extract_heads(spans, n_span, (const uint64_t*)ws.p, (const uint64_t*)we.p, (uint32_t*)head.p, st)); }
        if (n_span + 1 <= kOneLaunchSum) {
            ScanJobs jobs{}; jobs.n_jobs = 1;
            jobs.j[0] = ScanJob{(const uint32_t*)head.p, nullptr, (uint64_t*)rank.p, n_span + 1, nullptr};
            HIP_TRY(launch_scan_jobs(jobs, st));
        } else {
            AM_TRY(exclusive_sum(scan_tmp, (const uint32_t*)head.p, (uint64_t*)rank.p, n_span + 1, st));
        }
        uint64_t n_pieces = 0;                              // the one word that crosses
        AM_TRY(read_u64((const uint64_t*)rank.p + n_span, &n_pieces, st));
        if (n_pieces == 0 || n_pieces > n_span) return fail(AM_ERR_HIP, "extract: the piece count is out of range");
        f->n_items = n_pieces;
        AM_TRY(f->data.ensure(n_pieces * sizeof(Fragment)));
        { Prof pr("extract_emit", st);
          HIP_TRY(launch_extract_emit((const uint32_t*)head.p, (const uint64_t*)rank.p, (const uint64_t*)ws.p, (const uint64_t*)we.p, n_span, n_pieces, span_off, n_hay,
                                      (Fragment*)f->data.p, (uint64_t*)f->offsets.p, st)); }
    }
    HIP_TRY(hipStreamSynchronize(st));                      // (the workspaces are freed; a result may be used from any thread and stream afterwards)
    *out = f.release();
    return AM_OK;
}

}  // namespace

extern "C" int am_fragments_from_spans(const am_batch* src, const struct am_spans* s, uint32_t before, uint32_t after, int mode, am_fragments** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_stage(src, s, mode));
    return windows(src, s, before, after, mode, out);
}

extern "C" int am_extract_batch(const am_span_table* t, int case_mode, int spans_mode, uint32_t before, uint32_t after, int mode, const am_batch* b, am_batch** out,
                                am_fragments** frags_out)
{
    if (frags_out) *frags_out = nullptr;
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_route(case_mode, spans_mode, mode));
    if (!t || !b) return fail(AM_ERR_INVALID, "null span table or batch");
    if (t->ids->a->dev != b->dev) return fail(AM_ERR_INVALID, "span table and batch live on different devices");
    struct am_spans* raw = nullptr;
    AM_TRY(am_spans_batch(t, case_mode, spans_mode, b, &raw));
    SpansPtr s(raw, am_spans_free);
    AM_TRY(check_stage(b, s.get(), mode));
    am_fragments* fraw = nullptr;
    AM_TRY(windows(b, s.get(), before, after, mode, &fraw));
    FragmentsPtr f(fraw, am_fragments_free);
    AM_TRY(am_batch_from_fragments(b, f.get(), out));       // (AM_ERR_UNSUPPORTED from 2^32 - 1 fragments on)
    if (frags_out) *frags_out = f.release();
    return AM_OK;
}

extern "C" int am_extract(const am_span_table* t, int case_mode, int spans_mode, uint32_t before, uint32_t after, int mode, const am_slice* hay, size_t n_hay, am_batch** out,
                          am_fragments** frags_out)
{
    if (frags_out) *frags_out = nullptr;
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_slices(hay, n_hay));
    AM_TRY(check_route(case_mode, spans_mode, mode));
    if (!t) return fail(AM_ERR_INVALID, "null span table");      // (last: a caller without a device can see every other check)
    AM_TRY(ensure_runtime());
    // (no haystacks take the same way: a batch without haystacks, spans and fragments with offsets [0], a new batch without haystacks)
    return with_oneshot_batch(t->ids->a->dev, hay, n_hay, [&](am_batch* b) { return am_extract_batch(t, case_mode, spans_mode, before, after, mode, b, out, frags_out); });
}
