// am_subst.cpp -- substitute on the device (include/am.h "substitute"): the leftmost-longest spans of a batch (am_spans.cpp) spliced with the replacements of their
// needles into a NEW batch in HBM (am_subst.hip), `replace :: [Match] -> Text -> Text` of the reference (src/Data/Text/AhoCorasick/Replacer.hs:163-180) over matches
// that are never scanned again.  am_batch_substitute is the splice alone -- to am_spans what am_batch_from_fragments is to am_fragments -- and am_substitute_batch /
// am_substitute put the spans call in front of it.  A table of TEMPLATES (am_subst_table_create_templates; csrc/am_subst_tpl.h) is the same table type with another
// piece plan: the splice counts and numbers its pieces first, everything behind the piece kernel is shared.  Every argument is checked before any device work.
#include "am_spans.h"

using namespace am;
using namespace am::dev;
using namespace am::host;

struct am_subst_table {
    const am_span_table* t = nullptr;
    int dev = 0;
    uint32_t n_needles = 0;
    uint64_t pool_bytes = 0;
    DevBuf off, pool;                                       // uint64[n_needles + 1]; the replacements' bytes, padded: a 16-byte group read from any offset stays inside
    bool templates = false;                                 // am_subst_table_create_templates: off = seg_off, pool = the literals' bytes, segs = SubstSeg[n_seg]
    uint64_t n_seg = 0;
    DevBuf segs;
};

namespace {

constexpr size_t kPoolPad = 32;

int check_splice(const am_batch* src, const struct am_spans* s, const am_subst_table* r)
{
    if (!src || !s || !r) return fail(AM_ERR_INVALID, "null batch, spans or substitution table");
    if (s->unit != AM_UNIT_BYTES) return fail(AM_ERR_INVALID, "am_batch_substitute: the spans are in converted units (am_coords_spans); the splice reads byte spans");
    if (s->mode != AM_SPANS_LEFTMOST_LONGEST) return fail(AM_ERR_INVALID, "am_batch_substitute: the spans are not an AM_SPANS_LEFTMOST_LONGEST result (overlapping spans cannot be spliced)");
    if (s->n_hay != src->n_hay || s->src_total != src->total) return fail(AM_ERR_INVALID, "the spans were not produced from a batch with this haystack count and size");
    if (s->dev != src->dev || r->dev != src->dev) return fail(AM_ERR_INVALID, "batch, spans and substitution table live on different devices");
    if (r->n_needles != s->n_needles) return fail(AM_ERR_INVALID, "the substitution table's n_needles differs from that of the span table the spans were made with");
    return AM_OK;
}

// the splice; every argument has been checked
int splice(const am_batch* src, const struct am_spans* s, const am_subst_table* r, am_batch** out)
{
    AM_TRY(ensure_runtime());
    if (src->n_hay == 0) return DerivedBatch::empty(src->dev, out);
    ON_DEVICE(src->dev);
    hipStream_t st; AM_TRY(get_stream(src->dev, &st));
    DerivedBatch nb;
    nb.begin(src->dev);
    const uint64_t n_span = s->n_items, n_hay = src->n_hay;
    uint64_t n_pieces = 2 * n_span + n_hay;
    SubstIn in;
    in.spans = (const Span*)s->data.p; in.n_span = n_span; in.span_off = (const uint64_t*)s->offsets.p;
    in.src_off = src->d_offsets; in.src_total = src->total; in.n_hay = src->n_hay; in.n_needles = r->n_needles;
    in.repl_off = (const uint64_t*)r->off.p; in.pool_bytes = r->pool_bytes;
    DevBuf lens, src_at, live, dst_at, cidx, cdst, csrc, scan_tmp, cnt, pbase, cnt_tmp;
    SubstTpl tpl{(const uint64_t*)r->off.p, (const SubstSeg*)r->segs.p, r->n_seg};
    if (r->templates) {                                     // a span owns 1 + nseg pieces: their exclusive sum numbers them, its total is the one scalar read here
        AM_TRY(cnt.ensure((n_span + 1) * 4));
        AM_TRY(pbase.ensure((n_span + 1) * 8));
        uint64_t owned = 0;
        { Prof pr("subst_tpl_count", st);
          HIP_TRY(launch_subst_tpl_count(in, tpl, (uint32_t*)cnt.p, st));
          AM_TRY(exclusive_sum(cnt_tmp, (const uint32_t*)cnt.p, (uint64_t*)pbase.p, n_span + 1, st, &owned)); }
        n_pieces = owned + n_hay;
    }
    AM_TRY(lens.ensure((n_pieces + 1) * 8));
    AM_TRY(src_at.ensure((n_pieces + 1) * 8));
    AM_TRY(live.ensure((n_pieces + 1) * 4));
    AM_TRY(dst_at.ensure((n_pieces + 1) * 8));
    AM_TRY(cidx.ensure((n_pieces + 1) * 8));
    uint64_t* new_off; uint8_t* new_text;
    AM_TRY(nb.offsets(n_hay, &new_off));
    HIP_TRY(hipMemsetAsync(lens.p, 0, (n_pieces + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(live.p, 0, (n_pieces + 1) * 4, st));
    { Prof pr("subst_pieces", st);
      if (r->templates) HIP_TRY(launch_subst_tpl_pieces(in, tpl, (const uint64_t*)pbase.p, n_pieces, (uint64_t*)lens.p, (uint64_t*)src_at.p, (uint32_t*)live.p, st));
      else HIP_TRY(launch_subst_pieces(in, (uint64_t*)lens.p, (uint64_t*)src_at.p, (uint32_t*)live.p, st)); }
    { Prof pr("subst_scan", st);
      AM_TRY(exclusive_sum64(scan_tmp, (const uint64_t*)lens.p, (uint64_t*)dst_at.p, n_pieces + 1, st));      // (one temporary: its size depends on n_pieces + 1 alone)
      AM_TRY(exclusive_sum(scan_tmp, (const uint32_t*)live.p, (uint64_t*)cidx.p, n_pieces + 1, st)); }
    uint64_t total = 0, n_live = 0;
    HIP_TRY(hipMemcpyAsync(&total, (const uint64_t*)dst_at.p + n_pieces, 8, hipMemcpyDeviceToHost, st));
    AM_TRY(read_u64((const uint64_t*)cidx.p + n_pieces, &n_live, st));
    AM_TRY(cdst.ensure((n_live + 1) * 8));
    AM_TRY(csrc.ensure((n_live + 1) * 8));
    { Prof pr("subst_compact", st);
      HIP_TRY(launch_subst_compact((const uint64_t*)src_at.p, (const uint32_t*)live.p, (const uint64_t*)dst_at.p, (const uint64_t*)cidx.p, n_pieces, (uint64_t*)cdst.p,
                                   (uint64_t*)csrc.p, n_live, in.span_off, r->templates ? (const uint64_t*)pbase.p : nullptr, n_span, n_hay, new_off, st)); }
    AM_TRY(nb.text(total, st, &new_text));
    { Prof pr("subst_gather", st);
      HIP_TRY(launch_subst_gather((const uint8_t*)src->d_text, src->total, (const uint8_t*)r->pool.p, r->pool_bytes, (const uint64_t*)cdst.p, (const uint64_t*)csrc.p, n_live,
                                  total, new_text, g_rt.dev[src->dev].n_cu, st)); }
    HIP_TRY(hipStreamSynchronize(st));                      // a batch object may be used from any thread and stream afterwards; the workspaces are freed
    return nb.publish(total, n_hay, out);
}

}  // namespace

extern "C" int am_subst_table_create(const am_span_table* t, const uint64_t* repl_off, const uint8_t* repl_bytes, am_subst_table** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!t || !repl_off) return fail(AM_ERR_INVALID, "null span table or repl_off");
    const uint32_t n = t->ids->n_needles;
    if (repl_off[0] != 0) return fail(AM_ERR_INVALID, "am_subst_table_create: repl_off[0] must be 0");
    for (uint32_t v = 0; v < n; v++) {
        if (repl_off[v + 1] < repl_off[v]) return fail(AM_ERR_INVALID, "am_subst_table_create: repl_off descends at needle " + std::to_string(v));
        if (repl_off[v + 1] - repl_off[v] >= (1ull << 32)) return fail(AM_ERR_INVALID, "am_subst_table_create: a replacement of 2^32 bytes and more (needle " + std::to_string(v) + ")");
    }
    const uint64_t pool_bytes = repl_off[n];
    if (pool_bytes && !repl_bytes) return fail(AM_ERR_INVALID, "repl_bytes is null");
    AM_TRY(ensure_runtime());
    const int dev = t->ids->a->dev;
    ON_DEVICE(dev);
    std::unique_ptr<am_subst_table> r(new am_subst_table());
    r->t = t; r->dev = dev; r->n_needles = n; r->pool_bytes = pool_bytes;
    const size_t padded = (size_t)((pool_bytes + 15) & ~15ull) + kPoolPad;
    AM_TRY(r->off.ensure(((size_t)n + 1) * 8));
    AM_TRY(r->pool.ensure(padded));
    HIP_TRY(hipMemset(r->pool.p, 0, padded));
    HIP_TRY(hipMemcpy(r->off.p, repl_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    if (pool_bytes) HIP_TRY(hipMemcpy(r->pool.p, repl_bytes, (size_t)pool_bytes, hipMemcpyHostToDevice));
    *out = r.release();
    return AM_OK;
}

// a table of templates: off = seg_off, segs = one SubstSeg per segment, pool = the literals' bytes as given (padded as the replacements are)
extern "C" int am_subst_table_create_templates(const am_span_table* t, const uint64_t* seg_off, const uint8_t* seg_kind, const uint64_t* lit_off, const uint8_t* lit_bytes,
                                               am_subst_table** out)
{
    const std::string fn = "am_subst_table_create_templates: ";
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!t || !seg_off) return fail(AM_ERR_INVALID, "null span table or seg_off");
    const uint32_t n = t->ids->n_needles;
    if (seg_off[0] != 0) return fail(AM_ERR_INVALID, fn + "seg_off[0] must be 0");
    for (uint32_t v = 0; v < n; v++) {
        if (seg_off[v + 1] < seg_off[v]) return fail(AM_ERR_INVALID, fn + "seg_off descends at needle " + std::to_string(v));
        if (seg_off[v + 1] - seg_off[v] > AM_SUBST_MAX_SEGMENTS) return fail(AM_ERR_INVALID, fn + "more than AM_SUBST_MAX_SEGMENTS segments (needle " + std::to_string(v) + ")");
    }
    const uint64_t n_seg = seg_off[n];
    if (n_seg && (!seg_kind || !lit_off)) return fail(AM_ERR_INVALID, "seg_kind or lit_off is null");
    std::vector<SubstSeg> segs((size_t)n_seg);
    if (n_seg && lit_off[0] != 0) return fail(AM_ERR_INVALID, fn + "lit_off[0] must be 0");
    for (uint64_t s = 0; s < n_seg; s++) {
        if (seg_kind[s] != AM_SEG_LITERAL && seg_kind[s] != AM_SEG_MATCH) return fail(AM_ERR_INVALID, fn + "unknown segment kind at segment " + std::to_string(s));
        if (lit_off[s + 1] < lit_off[s]) return fail(AM_ERR_INVALID, fn + "lit_off descends at segment " + std::to_string(s));
        const uint64_t len = lit_off[s + 1] - lit_off[s];
        if (seg_kind[s] == AM_SEG_MATCH && len != 0) return fail(AM_ERR_INVALID, fn + "a MATCH segment with literal bytes (segment " + std::to_string(s) + ")");
        if (len >= (1ull << 32)) return fail(AM_ERR_INVALID, fn + "a literal of 2^32 bytes and more (segment " + std::to_string(s) + ")");
        segs[(size_t)s] = seg_kind[s] == AM_SEG_MATCH ? SubstSeg{0, 0, kSegMatch} : SubstSeg{lit_off[s], (uint32_t)len, kSegLiteral};
    }
    const uint64_t pool_bytes = n_seg ? lit_off[n_seg] : 0;
    if (pool_bytes && !lit_bytes) return fail(AM_ERR_INVALID, "lit_bytes is null");
    AM_TRY(ensure_runtime());
    const int dev = t->ids->a->dev;
    ON_DEVICE(dev);
    std::unique_ptr<am_subst_table> r(new am_subst_table());
    r->t = t; r->dev = dev; r->n_needles = n; r->pool_bytes = pool_bytes; r->templates = true; r->n_seg = n_seg;
    const size_t padded = (size_t)((pool_bytes + 15) & ~15ull) + kPoolPad;
    AM_TRY(r->off.ensure(((size_t)n + 1) * 8));
    AM_TRY(r->segs.ensure(((size_t)n_seg + 1) * sizeof(SubstSeg)));
    AM_TRY(r->pool.ensure(padded));
    HIP_TRY(hipMemset(r->pool.p, 0, padded));
    HIP_TRY(hipMemcpy(r->off.p, seg_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    if (n_seg) HIP_TRY(hipMemcpy(r->segs.p, segs.data(), (size_t)n_seg * sizeof(SubstSeg), hipMemcpyHostToDevice));
    if (pool_bytes) HIP_TRY(hipMemcpy(r->pool.p, lit_bytes, (size_t)pool_bytes, hipMemcpyHostToDevice));
    *out = r.release();
    return AM_OK;
}

extern "C" void am_subst_table_destroy(am_subst_table* r)
{
    if (!r) return;
    OnDevice od(r->dev);
    delete r;
}

extern "C" int am_batch_substitute(const am_batch* src, const struct am_spans* s, const am_subst_table* r, am_batch** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_splice(src, s, r));
    return splice(src, s, r, out);
}

extern "C" int am_substitute_batch(const am_subst_table* r, int case_mode, const am_batch* b, am_batch** out, struct am_spans** spans_out)
{
    if (spans_out) *spans_out = nullptr;
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_case(case_mode));
    if (!r || !b) return fail(AM_ERR_INVALID, "null substitution table or batch");
    if (r->dev != b->dev) return fail(AM_ERR_INVALID, "substitution table and batch live on different devices");
    struct am_spans* raw = nullptr;
    AM_TRY(am_spans_batch(r->t, case_mode, AM_SPANS_LEFTMOST_LONGEST, b, &raw));
    std::unique_ptr<struct am_spans, void (*)(struct am_spans*)> s(raw, am_spans_free);
    AM_TRY(check_splice(b, s.get(), r));
    AM_TRY(splice(b, s.get(), r, out));
    if (spans_out) *spans_out = s.release();
    return AM_OK;
}

extern "C" int am_substitute(const am_subst_table* r, int case_mode, const am_slice* hay, size_t n_hay, am_batch** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_slices(hay, n_hay));
    AM_TRY(check_case(case_mode));
    if (!r) return fail(AM_ERR_INVALID, "null substitution table");      // (last: a caller without a device can see every other check)
    AM_TRY(ensure_runtime());
    if (n_hay == 0) return DerivedBatch::empty(r->dev, out);
    return with_oneshot_batch(r->dev, hay, n_hay, [&](am_batch* b) { return am_substitute_batch(r, case_mode, b, out, nullptr); });      // (the result is a batch of its own)
}

extern "C" void am_substitute_geometry(uint32_t* group_bytes, uint32_t* tile_bytes)
{
    uint32_t g = 0, t = 0;
    subst_geometry(&g, &t);
    if (group_bytes) *group_bytes = g;
    if (tile_bytes) *tile_bytes = t;
}

// ---- batch accessors: what a device stage that PRODUCES text hands back

extern "C" uint64_t am_batch_haystacks(const am_batch* b) { return b ? b->n_hay : 0; }
extern "C" const void* am_batch_device_text(const am_batch* b) { return b ? b->d_text : nullptr; }
extern "C" const void* am_batch_device_offsets(const am_batch* b) { return b ? b->d_offsets : nullptr; }

namespace {
int read_back(const am_batch* b, void* dst, const void* d_src, size_t n)
{
    AM_TRY(ensure_runtime());
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));        // (a one-shot upload of this thread may still be on its way on that stream)
    HIP_TRY(hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return AM_OK;
}
}  // namespace

extern "C" int am_batch_read_offsets(const am_batch* b, uint64_t* out)
{
    if (!b || !out) return fail(AM_ERR_INVALID, "null batch or out");
    return read_back(b, out, b->d_offsets, ((size_t)b->n_hay + 1) * 8);
}

extern "C" int am_batch_read_text(const am_batch* b, uint64_t first_byte, uint64_t n_bytes, uint8_t* dst)
{
    if (!b) return fail(AM_ERR_INVALID, "null batch");
    if (first_byte > b->total || n_bytes > b->total - first_byte) return fail(AM_ERR_INVALID, "am_batch_read_text: the range ends beyond the batch's total bytes");
    if (n_bytes == 0) return AM_OK;
    if (!dst) return fail(AM_ERR_INVALID, "dst is null");
    return read_back(b, dst, (const uint8_t*)b->d_text + first_byte, (size_t)n_bytes);
}
