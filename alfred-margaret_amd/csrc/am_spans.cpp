// am_spans.cpp -- match spans on the device (include/am.h "match spans"): one scan of the batch, then the records a scan leaves in HBM are expanded through the value
// lists and the needles' own lengths into (start, len, haystack, needle), all of them in fold order or the leftmost-longest non-overlapping selection
// (am_spans.hip).  The result is CSR like am_fragments and stays in HBM until asked for: its handle, the chain selector's host sequence and the argument checks are
// am_fold.h's, shared with the other folds.
// A span table may carry a word class (am_span_table_create_words, include/am.h "whole words"): 8 dwords beside the lengths that the expansion filters with.
// It may also carry an exact spelling per handle (am_span_table_create_cased, include/am.h "exact case"): a pool beside the lengths, compared by am_cased.h.
#include "am_spans.h"

#include "am_cased.h"

#include <cstddef>
#include <cstring>

using namespace am;
using namespace am::dev;
using namespace am::host;

using SpansResult = struct am_spans;                     // (am_spans alone names the one-shot entry point)

static_assert(sizeof(am_span) == sizeof(Span) && sizeof(am_span) == 24, "am_span and the kernels' Span are one layout");
static_assert(offsetof(am_span, len) == 8 && offsetof(am_span, haystack) == 16 && offsetof(am_span, needle) == 20, "am_span: 0, 8, 16, 20");

namespace {

constexpr uint32_t kSpansChainLimit = 32;                   // candidates the lane of a chain's head looks at before the chain goes to the doubling rounds

int check_modes(int case_mode, int mode)
{
    AM_TRY(check_case(case_mode));
    if (mode != AM_SPANS_ALL && mode != AM_SPANS_LEFTMOST_LONGEST) return fail(AM_ERR_INVALID, "mode must be AM_SPANS_ALL or AM_SPANS_LEFTMOST_LONGEST");
    return AM_OK;
}

// the result of a call without haystacks
int empty_spans(int dev, int mode, uint32_t n_needles, SpansResult** out)
{
    AM_TRY(empty_result(dev, out));
    (*out)->mode = mode; (*out)->n_needles = n_needles;
    return AM_OK;
}

// the leftmost-longest selection over the spans in HBM: s->data, s->n_items, s->rounds and span_off
int select_leftmost_longest(const SpansIn& in, const Span* spans, uint64_t n_span, SpansResult* s, hipStream_t st)
{
    uint64_t* const span_off = (uint64_t*)s->offsets.p;
    const uint64_t n_words = (in.total + 31) / 32;
    DevBuf bits, pc, rank, scan_tmp, best, cand, tile_max, head, kept, kidx;
    uint64_t n_cand = 0;
    if (n_span != 0 && n_words != 0) {
        AM_TRY(bits.ensure((n_words + 1) * 4));
        AM_TRY(pc.ensure((n_words + 1) * 4));
        AM_TRY(rank.ensure((n_words + 1) * 8));
        HIP_TRY(hipMemsetAsync(bits.p, 0, (n_words + 1) * 4, st));
        { Prof pr("spans_mark", st);
          HIP_TRY(launch_spans_mark(spans, n_span, in, (uint32_t*)bits.p, n_words, st)); }
        { Prof pr("spans_rank", st);
          HIP_TRY(launch_spans_popcount((const uint32_t*)bits.p, n_words, (uint32_t*)pc.p, st));
          AM_TRY(exclusive_sum(scan_tmp, (const uint32_t*)pc.p, (uint64_t*)rank.p, n_words + 1, st, &n_cand)); }
    }
    if (n_cand == 0) {                                      // nothing but zero-length spans, or nothing at all: empty rows
        HIP_TRY(hipMemsetAsync(span_off, 0, ((uint64_t)in.n_hay + 1) * 8, st));
        s->n_items = 0;
        return AM_OK;
    }
    AM_TRY(best.ensure(n_cand * 8));
    AM_TRY(cand.ensure(n_cand * 8));
    AM_TRY(tile_max.ensure(((n_cand + 1 + kSpansMaxTile - 1) / kSpansMaxTile) * 8));
    AM_TRY(head.ensure(n_cand + 1));
    AM_TRY(kept.ensure((n_cand + 1) * 4));
    AM_TRY(kidx.ensure((n_cand + 1) * 8));
    uint32_t* const kp = (uint32_t*)kept.p;
    const uint64_t* const cg = (const uint64_t*)cand.p;
    const uint64_t* const bs = (const uint64_t*)best.p;
    HIP_TRY(hipMemsetAsync(best.p, 0, n_cand * 8, st));
    { Prof pr("spans_best", st);
      HIP_TRY(launch_spans_best(spans, n_span, in, (const uint32_t*)bits.p, (const uint64_t*)rank.p, n_words, (uint64_t*)best.p, n_cand, st)); }
    { Prof pr("spans_candidates", st);
      HIP_TRY(launch_spans_candidates((const uint32_t*)bits.p, (const uint64_t*)rank.p, n_words, (uint64_t*)cand.p, n_cand, st)); }
    { Prof pr("spans_heads", st);
      HIP_TRY(launch_spans_heads(cg, bs, n_cand, (uint64_t*)tile_max.p, (uint8_t*)head.p, kp, st)); }
    uint64_t n_out = 0;                                     // (the ranks are final, read back above: the scan's temporary may move)
    AM_TRY(select_chains(SpansChain{cg, bs, n_cand}, (const uint8_t*)head.p, kp, (uint64_t*)kidx.p, scan_tmp, cfg::get(cfg::kSpansChainLimit), kSpansChainLimit,
                         {"spans_walk", "spans_next", "spans_double"}, &n_out, &s->rounds, st));
    AM_TRY(s->data.ensure(n_out * sizeof(Span)));
    s->n_items = n_out;
    { Prof pr("spans_emit", st);
      HIP_TRY(launch_spans_emit(cg, bs, kp, (const uint64_t*)kidx.p, n_cand, in, (Span*)s->data.p, n_out, span_off, st)); }
    HIP_TRY(hipStreamSynchronize(st));                      // (the workspaces are freed)
    return AM_OK;
}

}  // namespace

namespace {

// the spellings of am_span_table_create_cased, checked on the host before any device work: what span_of's shortcut (am_words.h) rests on
int check_exact(const uint32_t* len_bytes, const uint32_t* len_code_points, uint32_t n, const uint64_t* exact_off, const uint8_t* exact_bytes, bool* any)
{
    *any = false;
    if (exact_off[0] != 0) return fail(AM_ERR_INVALID, "am_span_table_create_cased: exact_off[0] is not 0");
    for (uint32_t v = 0; v < n; v++)
        if (exact_off[v + 1] < exact_off[v]) return fail(AM_ERR_INVALID, "am_span_table_create_cased: exact_off descends at needle " + std::to_string(v));
    if (exact_off[n] != 0 && !exact_bytes) return fail(AM_ERR_INVALID, "am_span_table_create_cased: exact_bytes is null");
    uint64_t groups = 0;
    for (uint32_t v = 0; v < n; v++) {
        const uint64_t e = exact_off[v + 1] - exact_off[v];
        if (e == 0) continue;
        const std::string who = "am_span_table_create_cased: the spelling of needle " + std::to_string(v);
        if (e >= (1ull << 32)) return fail(AM_ERR_INVALID, who + " has 2^32 bytes or more");
        if (len_bytes[v] == 0) return fail(AM_ERR_INVALID, who + " belongs to a needle of length 0");
        const uint8_t* p = exact_bytes + exact_off[v];
        if ((p[0] & 0xC0) == 0x80) return fail(AM_ERR_INVALID, who + " begins with a continuation byte");
        uint64_t starts = 0;
        for (uint64_t i = 0; i < e; i++) starts += (p[i] & 0xC0) != 0x80 ? 1u : 0u;
        if (starts != len_code_points[v]) return fail(AM_ERR_INVALID, who + " has " + std::to_string(starts) + " code points, the needle has " + std::to_string(len_code_points[v]));
        groups += cased_padded(e) / kCasedGroup;
        *any = true;
    }
    if (groups >= (1ull << 32)) return fail(AM_ERR_INVALID, "am_span_table_create_cased: the spellings take 64 GiB or more");      // (ExactRef::at16 is 32 bits)
    return AM_OK;
}

// the spellings to the table's device: the host copy as given, an ExactRef per handle and the pool, every spelling at a multiple of kCasedGroup and zero-filled to
// the next one, kCasedPoolPad zero bytes behind the last (as the replacement pool of am_subst_table_create: a group read at any offset stays inside)
int upload_exact(am_span_table* t, uint32_t n, const uint64_t* exact_off, const uint8_t* exact_bytes)
{
    t->exact_off.assign(exact_off, exact_off + n + 1);
    if (exact_off[n]) t->exact_bytes.assign(exact_bytes, exact_bytes + exact_off[n]);
    std::vector<ExactRef> refs((size_t)n + 1, ExactRef{0, 0});
    uint64_t at = 0;
    for (uint32_t v = 0; v < n; v++) {
        const uint64_t e = exact_off[v + 1] - exact_off[v];
        if (e == 0) continue;
        refs[v] = ExactRef{(uint32_t)(at / kCasedGroup), (uint32_t)e};
        at += cased_padded(e);
    }
    std::vector<uint8_t> pool((size_t)at + kCasedPoolPad, 0);
    for (uint32_t v = 0; v < n; v++)
        if (refs[v].len) std::memcpy(pool.data() + (size_t)refs[v].at16 * kCasedGroup, exact_bytes + exact_off[v], refs[v].len);
    AM_TRY(t->exact_refs.ensure(refs.size() * sizeof(ExactRef)));
    AM_TRY(t->exact_pool.ensure(pool.size()));
    HIP_TRY(hipMemcpy(t->exact_refs.p, refs.data(), refs.size() * sizeof(ExactRef), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t->exact_pool.p, pool.data(), pool.size(), hipMemcpyHostToDevice));
    t->has_exact = true;
    return AM_OK;
}

// am_span_table_create, am_span_table_create_words and am_span_table_create_cased: one set of checks, one set of messages; word_bytes (256 flags, not null) only
// where has_words; exact_off (n_needles + 1 offsets into exact_bytes) nullable: no spelling
int create_table(const am_needle_ids* ids, const uint32_t* len_bytes, const uint32_t* len_code_points, bool has_words, const uint8_t* word_bytes, am_span_table** out,
                 const uint64_t* exact_off = nullptr, const uint8_t* exact_bytes = nullptr)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!ids) return fail(AM_ERR_INVALID, "null needle ids");
    const uint32_t n = ids->n_needles;
    if (n && (!len_bytes || !len_code_points)) return fail(AM_ERR_INVALID, "len_bytes or len_code_points is null");
    for (uint32_t v = 0; v < n; v++) {
        if (len_code_points[v] > len_bytes[v]) return fail(AM_ERR_INVALID, "am_span_table_create: len_code_points exceeds len_bytes for needle " + std::to_string(v));
        if ((len_code_points[v] == 0) != (len_bytes[v] == 0)) return fail(AM_ERR_INVALID, "am_span_table_create: exactly one length of needle " + std::to_string(v) + " is 0");
        if (len_code_points[v] >= (1u << 30)) return fail(AM_ERR_INVALID, "am_span_table_create: 2^30 code points and more (a span length must fit 32 bits)");
    }
    bool any_exact = false;
    if (exact_off) AM_TRY(check_exact(len_bytes, len_code_points, n, exact_off, exact_bytes, &any_exact));
    AM_TRY(ensure_runtime());
    ON_DEVICE(ids->a->dev);
    std::unique_ptr<am_span_table> t(new am_span_table());
    t->ids = ids;
    AM_TRY(t->len_bytes.ensure((size_t)n * 4 + 4));
    AM_TRY(t->len_cps.ensure((size_t)n * 4 + 4));
    if (n) {
        HIP_TRY(hipMemcpy(t->len_bytes.p, len_bytes, (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t->len_cps.p, len_code_points, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    if (has_words) {
        uint32_t packed[kWordClassWords] = {};
        for (uint32_t b = 0; b < 256; b++) {
            t->word_bytes[b] = word_bytes[b] ? 1 : 0;
            if (word_bytes[b]) packed[b >> 5] |= 1u << (b & 31u);
        }
        AM_TRY(t->words.ensure(sizeof(packed)));
        HIP_TRY(hipMemcpy(t->words.p, packed, sizeof(packed), hipMemcpyHostToDevice));
        t->has_words = true;
    }
    if (any_exact) AM_TRY(upload_exact(t.get(), n, exact_off, exact_bytes));      // (no spelling at all: the table of today, byte for byte)
    *out = t.release();
    return AM_OK;
}

}  // namespace

extern "C" int am_span_table_create_cased(const am_needle_ids* ids, const uint32_t* len_bytes, const uint32_t* len_code_points, uint32_t flags, const uint8_t* word_bytes,
                                          const uint64_t* exact_off, const uint8_t* exact_bytes, am_span_table** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (flags & ~AM_SPAN_TABLE_WORDS) return fail(AM_ERR_INVALID, "am_span_table_create_cased: unknown flag bits");
    const bool has_words = (flags & AM_SPAN_TABLE_WORDS) != 0;
    uint8_t dflt[256];
    if (has_words && !word_bytes) am_word_bytes_default(dflt);
    return create_table(ids, len_bytes, len_code_points, has_words, word_bytes ? word_bytes : dflt, out, exact_off, exact_bytes);
}

// the checks of the spellings alone, for a caller that wants them before a device exists (and for the tests of a machine without one)
extern "C" int am_span_table_check_exact(const uint32_t* len_bytes, const uint32_t* len_code_points, uint32_t n_needles, const uint64_t* exact_off, const uint8_t* exact_bytes)
{
    if (!exact_off) return AM_OK;
    if (n_needles && (!len_bytes || !len_code_points)) return fail(AM_ERR_INVALID, "len_bytes or len_code_points is null");
    bool any = false;
    return check_exact(len_bytes, len_code_points, n_needles, exact_off, exact_bytes, &any);
}

extern "C" int am_span_table_exact(const am_span_table* t, uint32_t needle, const uint8_t** bytes, uint64_t* len)
{
    if (bytes) *bytes = nullptr;
    if (len) *len = 0;
    if (!t || !t->has_exact || (uint64_t)needle + 1 >= t->exact_off.size()) return 0;
    const uint64_t e = t->exact_off[needle + 1] - t->exact_off[needle];
    if (e == 0) return 0;
    if (bytes) *bytes = t->exact_bytes.data() + t->exact_off[needle];
    if (len) *len = e;
    return 1;
}

extern "C" int am_span_table_create(const am_needle_ids* ids, const uint32_t* len_bytes, const uint32_t* len_code_points, am_span_table** out)
{
    return create_table(ids, len_bytes, len_code_points, false, nullptr, out);
}

// the default class: 0-9 A-Z a-z _ and every byte of a multi-byte UTF-8 sequence (any code point beyond ASCII is a word character)
extern "C" void am_word_bytes_default(uint8_t out[256])
{
    if (!out) return;
    for (uint32_t b = 0; b < 256; b++)
        out[b] = ((b >= '0' && b <= '9') || (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b == '_' || b >= 0x80) ? 1 : 0;
}

extern "C" int am_span_table_create_words(const am_needle_ids* ids, const uint32_t* len_bytes, const uint32_t* len_code_points, const uint8_t* word_bytes, am_span_table** out)
{
    uint8_t dflt[256];
    if (!word_bytes) am_word_bytes_default(dflt);
    return create_table(ids, len_bytes, len_code_points, true, word_bytes ? word_bytes : dflt, out);
}

extern "C" int am_span_table_word_bytes(const am_span_table* t, uint8_t* out256)
{
    if (!t || !t->has_words) return 0;
    if (out256) std::memcpy(out256, t->word_bytes, 256);
    return 1;
}

extern "C" void am_span_table_destroy(am_span_table* t) { delete t; }

extern "C" int am_spans_batch(const am_span_table* t, int case_mode, int mode, const am_batch* cb, SpansResult** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_modes(case_mode, mode));
    if (!t || !cb) return fail(AM_ERR_INVALID, "null span table or batch");
    const am_needle_ids* ids = t->ids;
    if (ids->a->dev != cb->dev) return fail(AM_ERR_INVALID, "span table and batch live on different devices");
    AM_TRY(ensure_runtime());
    am_batch* b = const_cast<am_batch*>(cb);
    if (b->n_hay == 0) return empty_spans(b->dev, mode, ids->n_needles, out);
    std::unique_ptr<SpansResult, void (*)(SpansResult*)> s(new SpansResult(), am_spans_free);
    s->dev = b->dev; s->n_hay = b->n_hay;
    s->mode = mode; s->n_needles = ids->n_needles; s->src_total = b->total;
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    RecordArray ra(b->dev);
    uint64_t n_rec = 0;
    if (b->total != 0) AM_TRY(run_records(ids->a, case_mode, b, records_into(ra), &n_rec));
    const SpansIn in = spans_in(t, (const Record*)ra.p, n_rec, b, b->n_hay);
    DevBuf cnt, voff, scan_tmp, rec_first, all_spans;
    AM_TRY(cnt.ensure((n_rec + 1) * 4));
    AM_TRY(voff.ensure((n_rec + 1) * 8));
    AM_TRY(rec_first.ensure(((uint64_t)b->n_hay + 1) * 8));
    AM_TRY(s->offsets.ensure(((uint64_t)b->n_hay + 1) * 8));
    uint64_t n_span = 0;
    { Prof pr("spans_count", st);
      HIP_TRY(launch_spans_count(case_mode == AM_IGNORE_CASE, in, (uint32_t*)cnt.p, st));
      AM_TRY(exclusive_sum(scan_tmp, (const uint32_t*)cnt.p, (uint64_t*)voff.p, n_rec + 1, st, &n_span)); }
    DevBuf& spans = mode == AM_SPANS_ALL ? s->data : all_spans;
    AM_TRY(spans.ensure(n_span * sizeof(Span)));
    { Prof pr("spans_write", st);
      HIP_TRY(launch_spans_write(case_mode == AM_IGNORE_CASE, in, (const uint64_t*)voff.p, (Span*)spans.p, n_span, st)); }
    if (mode == AM_SPANS_ALL) {
        HIP_TRY(launch_rp_ranges(in.recs, n_rec, (uint64_t*)rec_first.p, kNoRoute, b->n_hay, st));
        HIP_TRY(launch_spans_offsets((const uint64_t*)rec_first.p, (const uint64_t*)voff.p, n_rec, b->n_hay, (uint64_t*)s->offsets.p, st));
        s->n_items = n_span;
    } else {
        AM_TRY(select_leftmost_longest(in, (const Span*)spans.p, n_span, s.get(), st));
    }
    HIP_TRY(hipStreamSynchronize(st));                      // (the record array goes back to the cache, the workspaces are freed)
    *out = s.release();
    return AM_OK;
}

extern "C" int am_spans(const am_span_table* t, int case_mode, int mode, const am_slice* hay, size_t n_hay, SpansResult** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_slices(hay, n_hay));
    AM_TRY(check_modes(case_mode, mode));
    if (!t) return fail(AM_ERR_INVALID, "null span table");      // (last: a caller without a device can see every other check)
    AM_TRY(ensure_runtime());
    const int dev = t->ids->a->dev;
    if (n_hay == 0) return empty_spans(dev, mode, t->ids->n_needles, out);
    return with_oneshot_batch(dev, hay, n_hay, [&](am_batch* b) { return am_spans_batch(t, case_mode, mode, b, out); });
}

extern "C" uint64_t am_spans_size(const SpansResult* s) { return s ? s->n_items : 0; }
extern "C" uint64_t am_spans_haystacks(const SpansResult* s) { return s ? s->n_hay : 0; }
extern "C" uint32_t am_spans_rounds(const SpansResult* s) { return s ? s->rounds : 0; }
extern "C" const void* am_spans_device_offsets(const SpansResult* s) { return s ? s->offsets.p : nullptr; }
extern "C" const void* am_spans_device_data(const SpansResult* s) { return s && s->n_items ? s->data.p : nullptr; }

extern "C" const uint64_t* am_spans_offsets(SpansResult* s)
{
    if (!s) { fail(AM_ERR_INVALID, "null spans"); return nullptr; }
    return s->fetch_offsets("the spans");
}

extern "C" const am_span* am_spans_data(SpansResult* s)
{
    if (!s) { fail(AM_ERR_INVALID, "null spans"); return nullptr; }
    return s->fetch_data("the spans");
}

extern "C" void am_spans_free(SpansResult* s) { delete s; }
