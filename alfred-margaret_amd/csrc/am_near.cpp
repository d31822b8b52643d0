// am_near.cpp -- proximity on the device (include/am.h "proximity"): which matches of one group lie within max_gap bytes of a match of another, from one scan.  A stage
// over the rows of an AM_SPANS_LEFTMOST_LONGEST result where they lie in HBM (am_near.hip): group bitmaps over the span indices, the word links, a lane per span that
// picks its partner per query (near_pick, am_near.h), one exclusive sum that places the pairs, the emit.  The result is CSR like am_spans with am_rule_hits' bitmaps
// and counts beside it, and stays in HBM until asked for; its handle, the one-shot form and the argument checks are am_fold.h's.  am_select_near is am_select.cpp's.
// WORKSPACE of a call, freed when it returns: 20 bytes per span (the hit masks, their counts, the pairs' places) and 0.25 bytes per span and bitmap row (one row per
// group a query names: 8 bytes per span at the most).  What crosses to the host: the pair count.
// Every argument is checked before any device work, but for am_near_create's null group_mask: whether a mask is needed is the table's needle count, and the table is
// not looked at before the runtime is up.  am_near_spans holds a spans result to the table by what the result remembers of it: n_needles and the device.
#include "am_near_host.h"

#include <cstddef>

using namespace am;
using namespace am::dev;
using namespace am::host;

using SpansResult = struct am_spans;                        // (am_spans alone names the one-shot entry point)
using NearCall = struct am_near;                            // (as am_near does)

static_assert(sizeof(am_near_query) == sizeof(NearQuery) && sizeof(am_near_query) == 24, "am_near_query and the kernels' NearQuery are one layout");
static_assert(offsetof(am_near_query, group_b) == 4 && offsetof(am_near_query, flags) == 8 && offsetof(am_near_query, reserved) == 12 && offsetof(am_near_query, max_gap) == 16,
              "am_near_query: 0, 4, 8, 12, 16");
static_assert(sizeof(am_near_pair) == sizeof(NearPair) && sizeof(am_near_pair) == 32, "am_near_pair and the kernels' NearPair are one layout");
static_assert(offsetof(am_near_pair, b) == 8 && offsetof(am_near_pair, gap) == 16 && offsetof(am_near_pair, haystack) == 24 && offsetof(am_near_pair, query) == 28, "am_near_pair: 0, 8, 16, 24, 28");
static_assert(AM_NEAR_MAX_GROUPS == kNearMaxGroups && AM_NEAR_MAX_QUERIES == kNearMaxQueries && AM_NEAR_ORDERED == kNearOrdered, "the header's limits are the kernels'");

// the groups and queries of a proximity call in HBM beside the span table they index.  (Holds DevBufs: on the heap only.)
struct am_near {
    const am_span_table* t = nullptr;                       // must outlive the handle
    int dev = 0;
    uint32_t n_needles = 0;
    NearPlan plan{};
    DevBuf masks, dq;                                       // uint32[n_needles], NearQueryDev[n_queries]
};

namespace {

using HitsPtr = std::unique_ptr<am_near_hits, void (*)(am_near_hits*)>;

// the result of a call without haystacks: no pairs, offsets = [0], no word of fired, every count zero; nothing in HBM
int empty_hits(const NearCall* p, am_near_hits** out)
{
    AM_TRY(empty_result(p->dev, out));
    (*out)->n_queries = p->plan.n_queries;
    (*out)->h_fired.assign(1, 0); (*out)->h_counts.assign(std::max<size_t>(p->plan.n_queries, 1), 0);
    (*out)->fired_fetched = (*out)->counts_fetched = true;
    return AM_OK;
}

// the spans of a call without haystacks
int empty_spans(const NearCall* p, SpansResult** out)
{
    AM_TRY(empty_result(p->dev, out));
    (*out)->mode = AM_SPANS_LEFTMOST_LONGEST; (*out)->n_needles = p->n_needles;
    return AM_OK;
}

}  // namespace

extern "C" int am_near_create(const am_span_table* t, const uint32_t* group_mask, const am_near_query* queries, uint32_t n_queries, NearCall** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (n_queries > AM_NEAR_MAX_QUERIES) return fail(AM_ERR_INVALID, "n_queries must not exceed AM_NEAR_MAX_QUERIES");
    if (n_queries && !queries) return fail(AM_ERR_INVALID, "queries is null");
    for (uint32_t q = 0; q < n_queries; q++) {
        if (queries[q].group_a >= AM_NEAR_MAX_GROUPS || queries[q].group_b >= AM_NEAR_MAX_GROUPS)
            return fail(AM_ERR_INVALID, "am_near_create: a group index of query " + std::to_string(q) + " is not below AM_NEAR_MAX_GROUPS");
        if (queries[q].flags & ~AM_NEAR_ORDERED) return fail(AM_ERR_INVALID, "am_near_create: unknown flags in query " + std::to_string(q));
        if (queries[q].reserved != 0) return fail(AM_ERR_INVALID, "am_near_create: reserved must be 0 in query " + std::to_string(q));
    }
    if (!t) return fail(AM_ERR_INVALID, "null span table");      // (last: a caller without a device can see every other check)
    AM_TRY(ensure_runtime());                               // (the table is not looked at before)
    const uint32_t n = t->ids->n_needles;
    if (n && !group_mask) return fail(AM_ERR_INVALID, "group_mask is null");
    const int dev = t->ids->a->dev;
    ON_DEVICE(dev);
    std::unique_ptr<NearCall, void (*)(NearCall*)> p(new NearCall(), am_near_destroy);
    p->t = t; p->dev = dev; p->n_needles = n;
    p->plan = near_plan((const NearQuery*)queries, n_queries);
    std::vector<NearQueryDev> dq(n_queries);
    for (uint32_t q = 0; q < n_queries; q++) dq[q] = NearQueryDev{queries[q].group_a, p->plan.row_of[queries[q].group_b], queries[q].flags, 0, queries[q].max_gap};
    AM_TRY(p->masks.ensure((size_t)n * 4 + 4));
    AM_TRY(p->dq.ensure((size_t)n_queries * sizeof(NearQueryDev) + 8));
    if (n) HIP_TRY(hipMemcpy(p->masks.p, group_mask, (size_t)n * 4, hipMemcpyHostToDevice));
    if (n_queries) HIP_TRY(hipMemcpy(p->dq.p, dq.data(), (size_t)n_queries * sizeof(NearQueryDev), hipMemcpyHostToDevice));
    *out = p.release();
    return AM_OK;
}

extern "C" void am_near_destroy(NearCall* p)
{
    if (!p) return;
    OnDevice od(p->dev);
    delete p;
}

extern "C" int am_near_spans(const NearCall* p, const SpansResult* s, am_near_hits** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!p || !s) return fail(AM_ERR_INVALID, "null proximity handle or spans");
    if (s->unit != AM_UNIT_BYTES) return fail(AM_ERR_INVALID, "am_near_spans: the spans are in converted units (am_coords_spans); the gaps are measured between byte spans");
    if (s->mode != AM_SPANS_LEFTMOST_LONGEST) return fail(AM_ERR_INVALID, "am_near_spans takes an AM_SPANS_LEFTMOST_LONGEST result (rows that ascend and do not overlap)");
    if (s->n_needles != p->n_needles) return fail(AM_ERR_INVALID, "the spans were not made under a table with this number of needles");
    if (s->dev != p->dev) return fail(AM_ERR_INVALID, "proximity handle and spans live on different devices");
    AM_TRY(ensure_runtime());
    if (s->n_hay == 0) return empty_hits(p, out);
    const uint64_t n = s->n_items, n_hay = s->n_hay, nq = p->plan.n_queries, hay_words = (n_hay + 63) / 64;
    const uint64_t n_words = (n + 63) / 64;
    if (n_words >= 0xFFFF0000ull) return fail(AM_ERR_UNSUPPORTED, "am_near_spans: 2^38 spans and more (a word link is 32 bits)");
    ON_DEVICE(p->dev);
    hipStream_t st; AM_TRY(get_stream(p->dev, &st));
    HitsPtr x(new am_near_hits(), am_near_hits_free);
    x->dev = p->dev; x->n_hay = n_hay; x->n_queries = nq; x->hay_words = hay_words; x->src_total = s->src_total;
    AM_TRY(x->offsets.ensure((n_hay + 1) * 8));
    AM_TRY(x->fired.ensure(nq * hay_words * 8 + 8));
    AM_TRY(x->counts.ensure(nq * 8 + 8));
    HIP_TRY(hipMemsetAsync(x->fired.p, 0, nq * hay_words * 8 + 8, st));
    HIP_TRY(hipMemsetAsync(x->counts.p, 0, nq * 8 + 8, st));
    const uint64_t rows = p->plan.n_rows;
    if (n == 0 || nq == 0) {                                // no span or no query: empty rows
        HIP_TRY(hipMemsetAsync(x->offsets.p, 0, (n_hay + 1) * 8, st));
        HIP_TRY(hipStreamSynchronize(st));
        *out = x.release();
        return AM_OK;
    }
    DevBuf bits, prev_nz, next_nz, hit_mask, hit_count, pos, scan_tmp;
    AM_TRY(bits.ensure(rows * n_words * 8));
    AM_TRY(prev_nz.ensure(rows * n_words * 4));
    AM_TRY(next_nz.ensure(rows * n_words * 4));
    AM_TRY(hit_mask.ensure(n * 8));
    AM_TRY(hit_count.ensure((n + 1) * 4));
    AM_TRY(pos.ensure((n + 1) * 8));
    NearIn in{};
    in.spans = (const Span*)s->data.p; in.n_span = n; in.n_words = (uint32_t)n_words;
    in.span_off = (const uint64_t*)s->offsets.p; in.n_hay = n_hay;
    in.group_mask = (const uint32_t*)p->masks.p; in.n_needles = p->n_needles;
    in.dq = (const NearQueryDev*)p->dq.p; in.plan = p->plan;
    in.bits = (uint64_t*)bits.p; in.prev_nz = (uint32_t*)prev_nz.p; in.next_nz = (uint32_t*)next_nz.p;
    in.hit_mask = (uint64_t*)hit_mask.p; in.hit_count = (uint32_t*)hit_count.p; in.pos = (const uint64_t*)pos.p;
    in.fired = (uint64_t*)x->fired.p; in.hay_words = hay_words; in.counts = (uint64_t*)x->counts.p;
    in.out_off = (uint64_t*)x->offsets.p;
    const int n_cu = g_rt.dev[p->dev].n_cu;
    HIP_TRY(hipMemsetAsync((uint32_t*)hit_count.p + n, 0, 4, st));      // (the sum's trailing element)
    { Prof pr("near_bits", st);
      HIP_TRY(launch_near_bits(in, n_cu, st)); }
    { Prof pr("near_words", st);
      HIP_TRY(launch_near_words(in, st)); }
    { Prof pr("near_count", st);
      HIP_TRY(launch_near_count(in, n_cu, st)); }
    uint64_t n_pairs = 0;
    { Prof pr("near_place", st);
      AM_TRY(exclusive_sum(scan_tmp, (const uint32_t*)hit_count.p, (uint64_t*)pos.p, n + 1, st, &n_pairs)); }
    if (n_pairs > n * nq) return fail(AM_ERR_HIP, "am_near_spans: the pairs' sum is out of range");
    AM_TRY(x->data.ensure(n_pairs * sizeof(NearPair)));
    x->n_items = n_pairs;
    in.pairs = (NearPair*)x->data.p; in.n_pairs = n_pairs;
    { Prof pr("near_emit", st);
      HIP_TRY(launch_near_emit(in, n_cu, st)); }
    HIP_TRY(hipStreamSynchronize(st));                      // (the workspaces are freed; a result may be used from any thread and stream afterwards)
    *out = x.release();
    return AM_OK;
}

extern "C" int am_near_batch(const NearCall* p, int case_mode, const am_batch* b, am_near_hits** out, SpansResult** spans_out)
{
    if (out) *out = nullptr;
    if (spans_out) *spans_out = nullptr;
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    AM_TRY(check_case(case_mode));
    if (!p || !b) return fail(AM_ERR_INVALID, "null proximity handle or batch");
    if (p->dev != b->dev) return fail(AM_ERR_INVALID, "proximity handle and batch live on different devices");
    SpansResult* raw = nullptr;
    AM_TRY(am_spans_batch(p->t, case_mode, AM_SPANS_LEFTMOST_LONGEST, b, &raw));
    std::unique_ptr<SpansResult, void (*)(SpansResult*)> s(raw, am_spans_free);
    AM_TRY(am_near_spans(p, s.get(), out));
    if (spans_out) *spans_out = s.release();
    return AM_OK;
}

extern "C" int am_near(const NearCall* p, int case_mode, const am_slice* hay, size_t n_hay, am_near_hits** out, SpansResult** spans_out)
{
    if (out) *out = nullptr;
    if (spans_out) *spans_out = nullptr;
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    AM_TRY(check_slices(hay, n_hay));
    AM_TRY(check_case(case_mode));
    if (!p) return fail(AM_ERR_INVALID, "null proximity handle");      // (last: a caller without a device can see every other check)
    AM_TRY(ensure_runtime());                               // (the handle is not looked at before)
    if (n_hay == 0) {
        if (spans_out) AM_TRY(empty_spans(p, spans_out));
        return empty_hits(p, out);
    }
    return with_oneshot_batch(p->dev, hay, n_hay, [&](am_batch* b) { return am_near_batch(p, case_mode, b, out, spans_out); });
}

extern "C" uint64_t am_near_hits_size(const am_near_hits* x) { return x ? x->n_items : 0; }
extern "C" uint64_t am_near_hits_haystacks(const am_near_hits* x) { return x ? x->n_hay : 0; }
extern "C" uint64_t am_near_hits_queries(const am_near_hits* x) { return x ? x->n_queries : 0; }
extern "C" uint64_t am_near_hits_hay_words(const am_near_hits* x) { return x ? x->hay_words : 0; }
extern "C" const void* am_near_hits_device_offsets(const am_near_hits* x) { return x ? x->offsets.p : nullptr; }
extern "C" const void* am_near_hits_device_data(const am_near_hits* x) { return x && x->n_items ? x->data.p : nullptr; }
extern "C" const void* am_near_hits_device_fired(const am_near_hits* x) { return x && x->n_queries * x->hay_words ? x->fired.p : nullptr; }
extern "C" const void* am_near_hits_device_counts(const am_near_hits* x) { return x && x->n_queries && x->n_hay ? x->counts.p : nullptr; }

extern "C" const uint64_t* am_near_hits_offsets(am_near_hits* x)
{
    if (!x) { fail(AM_ERR_INVALID, "null proximity hits"); return nullptr; }
    return x->fetch_offsets("the proximity pairs");
}

extern "C" const am_near_pair* am_near_hits_data(am_near_hits* x)
{
    if (!x) { fail(AM_ERR_INVALID, "null proximity hits"); return nullptr; }
    return x->fetch_data("the proximity pairs");
}

extern "C" const uint64_t* am_near_hits_fired(am_near_hits* x)
{
    if (!x) { fail(AM_ERR_INVALID, "null proximity hits"); return nullptr; }
    return fetch_once(x->h_fired, x->fired_fetched, x->dev, x->fired, x->n_queries * x->hay_words, "the proximity bitmaps");
}

extern "C" const uint64_t* am_near_hits_counts(am_near_hits* x)
{
    if (!x) { fail(AM_ERR_INVALID, "null proximity hits"); return nullptr; }
    return fetch_once(x->h_counts, x->counts_fetched, x->dev, x->counts, x->n_queries, "the proximity counts");
}

extern "C" void am_near_hits_free(am_near_hits* x)
{
    if (!x) return;
    OnDevice od(x->dev);
    delete x;
}

extern "C" void am_near_geometry(uint32_t* tile_spans, uint32_t* word_spans) { near_geometry(tile_spans, word_spans); }
