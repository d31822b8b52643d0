// am_coords.cpp -- match coordinates on the device (include/am.h "coordinates"): positions, spans and fragments in code points or UTF-16 code units, and the line and
// column of every span, converted in HBM.  am_coords_create builds the index of a batch (am_coords.hip: one pass over the text counts the classes per tile of 128
// bytes, one exclusive sum per class makes the uint64 prefixes the index keeps; the uint32 counts are workspace); the four consumers take one lane per row and call
// the lookup of am_coords.h.  What crosses to the host during a call: nothing, except the flag word of am_coords_positions*.  Every argument is checked before any
// device work.
#include "am_coords.h"
#include "am_spans.h"

using namespace am;
using namespace am::dev;
using namespace am::host;

struct am_coords {
    int dev = 0;
    const am_batch* b = nullptr;                            // borrowed: the batch outlives the index
    uint32_t what = 0;
    uint64_t n_tiles = 0, src_total = 0; uint32_t n_hay = 0;
    DevBuf prefix[kCoordsClasses];                          // uint64[n_tiles + 1] per class the index carries
    uint64_t kept_bytes = 0;
    CoordsIn in() const
    {
        CoordsIn x{};
        x.text = (const uint8_t*)b->d_text; x.offsets = b->d_offsets;
        for (uint32_t c = 0; c < kCoordsClasses; c++) x.prefix[c] = (const uint64_t*)prefix[c].p;
        x.total = src_total; x.padded = (src_total + 15) & ~15ull; x.n_hay = n_hay;
        return x;
    }
};

struct am_ranges : am::host::CsrResult<am_span_range> {};
static_assert(sizeof(am_span_range) == sizeof(am::dev::SpanRange) && sizeof(am_span_range) == 32, "am_span_range and the kernels' SpanRange are one layout");

namespace {

using CoordsPtr = std::unique_ptr<am_coords, void (*)(am_coords*)>;
using SpansPtr = std::unique_ptr<struct am_spans, void (*)(struct am_spans*)>;
using FragmentsPtr = std::unique_ptr<am_fragments, void (*)(am_fragments*)>;
using RangesPtr = std::unique_ptr<am_ranges, void (*)(am_ranges*)>;

constexpr uint32_t kClassFlag[kCoordsClasses] = {AM_COORDS_CODE_POINTS, AM_COORDS_UTF16, AM_COORDS_LINES};
constexpr uint32_t kAllFlags = AM_COORDS_CODE_POINTS | AM_COORDS_UTF16 | AM_COORDS_LINES;

int check_unit(int unit)
{
    return unit == AM_UNIT_BYTES || unit == AM_UNIT_CODE_POINTS || unit == AM_UNIT_UTF16 ? AM_OK
                                                                                        : fail(AM_ERR_INVALID, "unit must be AM_UNIT_BYTES, AM_UNIT_CODE_POINTS or AM_UNIT_UTF16");
}

// the index carries what a call in `unit` (and with lines) needs
int check_index(const am_coords* c, int unit, bool lines, const char* entry)
{
    if (unit != AM_UNIT_BYTES && !(c->what & AM_COORDS_CODE_POINTS)) return fail(AM_ERR_INVALID, std::string(entry) + ": the index was built without AM_COORDS_CODE_POINTS");
    if (unit == AM_UNIT_UTF16 && !(c->what & AM_COORDS_UTF16)) return fail(AM_ERR_INVALID, std::string(entry) + ": the index was built without AM_COORDS_UTF16");
    if (lines && !(c->what & AM_COORDS_LINES)) return fail(AM_ERR_INVALID, std::string(entry) + ": the index was built without AM_COORDS_LINES");
    return AM_OK;
}

// a result the index can convert: in bytes, and made from the index's batch (check_stage, am_extract.cpp)
int check_source(const am_coords* c, int res_unit, uint64_t n_hay, uint64_t src_total, int dev, const char* entry, const char* noun)
{
    if (res_unit != AM_UNIT_BYTES) return fail(AM_ERR_INVALID, std::string(entry) + ": the " + noun + " are in converted units already; the index converts byte positions");
    if (n_hay != c->n_hay || src_total != c->src_total || dev != c->dev)
        return fail(AM_ERR_INVALID, std::string("the ") + noun + " were not produced from a batch with this haystack count and size");
    return AM_OK;
}

int check_spans_call(const am_coords* c, const struct am_spans* s, int unit, bool lines, const char* entry)
{
    if (!c || !s) return fail(AM_ERR_INVALID, "null index or spans");
    AM_TRY(check_unit(unit));
    AM_TRY(check_source(c, s->unit, s->n_hay, s->src_total, s->dev, entry, "spans"));
    return check_index(c, unit, lines, entry);
}

// offsets = a copy of the source's, on the stream
template <class Result>
int copy_offsets(Result* r, const DevBuf& src_offsets, uint64_t n_hay, hipStream_t st)
{
    AM_TRY(r->offsets.ensure((n_hay + 1) * 8));
    HIP_TRY(hipMemcpyAsync(r->offsets.p, src_offsets.p, (n_hay + 1) * 8, hipMemcpyDeviceToDevice, st));
    return AM_OK;
}

// the stage of am_coords_positions*: arrays in HBM, the flag word read back
int positions_device(const am_coords* c, const uint32_t* d_hay, const uint64_t* d_pos, uint64_t n, int unit, uint64_t* d_out, hipStream_t st)
{
    DevBuf flag;
    AM_TRY(flag.ensure(8));
    HIP_TRY(hipMemsetAsync(flag.p, 0, 8, st));
    { Prof pr("coords_positions", st);
      HIP_TRY(launch_coords_positions(c->in(), unit, d_hay, d_pos, n, d_out, (uint64_t*)flag.p, st)); }
    uint64_t raised = 0;                                    // the one word that crosses
    AM_TRY(read_u64(flag.p, &raised, st));
    if (raised) return fail(AM_ERR_INVALID, "am_coords_positions: a haystack index is not below the batch's haystack count, or a position lies beyond its haystack");
    return AM_OK;
}

int check_positions_call(const am_coords* c, const void* hay, const void* pos, uint64_t n, int unit, const void* out)
{
    if (!c) return fail(AM_ERR_INVALID, "null index");
    if (n && (!hay || !pos || !out)) return fail(AM_ERR_INVALID, "hay, pos or out is null");
    AM_TRY(check_unit(unit));
    return check_index(c, unit, false, "am_coords_positions");
}

}  // namespace

extern "C" void am_coords_destroy(am_coords* c) { delete c; }
extern "C" uint64_t am_coords_index_bytes(const am_coords* c) { return c ? c->kept_bytes : 0; }

extern "C" int am_coords_create(const am_batch* b, uint32_t what, am_coords** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!b) return fail(AM_ERR_INVALID, "null batch");
    if (what & ~kAllFlags) return fail(AM_ERR_INVALID, "what must be a combination of AM_COORDS_CODE_POINTS, AM_COORDS_UTF16 and AM_COORDS_LINES");
    if (what & AM_COORDS_UTF16) what |= AM_COORDS_CODE_POINTS;
    AM_TRY(ensure_runtime());
    CoordsPtr c(new am_coords(), am_coords_destroy);
    c->dev = b->dev; c->b = b; c->what = what; c->n_hay = b->n_hay; c->src_total = b->total;
    c->n_tiles = (b->total + kCoordsTile - 1) >> kCoordsTileShift;
    if (b->n_hay == 0 || what == 0) { *out = c.release(); return AM_OK; }
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    const uint64_t n = c->n_tiles + 1;
    DevBuf counts[kCoordsClasses], scan_tmp;                // uint32[n_tiles + 1] per class: workspace, freed on return
    uint32_t* d_counts[kCoordsClasses] = {nullptr, nullptr, nullptr};
    for (uint32_t k = 0; k < kCoordsClasses; k++) {
        if (!(what & kClassFlag[k])) continue;
        AM_TRY(counts[k].ensure(n * 4));
        AM_TRY(c->prefix[k].ensure(n * 8));
        c->kept_bytes += n * 8;
        d_counts[k] = (uint32_t*)counts[k].p;
        HIP_TRY(hipMemsetAsync(d_counts[k] + c->n_tiles, 0, 4, st));      // the sum's trailing element
    }
    { Prof pr("coords_tiles", st);
      HIP_TRY(launch_coords_tiles((const uint8_t*)b->d_text, b->total, d_counts, st)); }
    for (uint32_t k = 0; k < kCoordsClasses; k++) {
        if (!d_counts[k]) continue;
        Prof pr("coords_scan", st);
        AM_TRY(exclusive_sum(scan_tmp, d_counts[k], (uint64_t*)c->prefix[k].p, n, st));
    }
    HIP_TRY(hipStreamSynchronize(st));                      // (the workspaces are freed; the index may be used from any thread and stream afterwards)
    *out = c.release();
    return AM_OK;
}

extern "C" int am_coords_spans(const am_coords* c, const struct am_spans* s, int unit, struct am_spans** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_spans_call(c, s, unit, false, "am_coords_spans"));
    AM_TRY(ensure_runtime());
    SpansPtr r(new struct am_spans(), am_spans_free);
    r->rounds = s->rounds; r->mode = s->mode; r->n_needles = s->n_needles; r->src_total = s->src_total; r->unit = unit;
    if (s->n_hay == 0) { r->make_empty(s->dev); *out = r.release(); return AM_OK; }
    r->dev = s->dev; r->n_hay = s->n_hay; r->n_items = s->n_items;
    ON_DEVICE(c->dev);
    hipStream_t st; AM_TRY(get_stream(c->dev, &st));
    AM_TRY(copy_offsets(r.get(), s->offsets, s->n_hay, st));
    if (s->n_items) {
        AM_TRY(r->data.ensure(s->n_items * sizeof(Span)));
        if (unit == AM_UNIT_BYTES) HIP_TRY(hipMemcpyAsync(r->data.p, s->data.p, s->n_items * sizeof(Span), hipMemcpyDeviceToDevice, st));
        else { Prof pr("coords_spans", st);
               HIP_TRY(launch_coords_spans(c->in(), unit, (const Span*)s->data.p, s->n_items, (Span*)r->data.p, st)); }
    }
    HIP_TRY(hipStreamSynchronize(st));
    *out = r.release();
    return AM_OK;
}

extern "C" int am_coords_fragments(const am_coords* c, const am_fragments* f, int unit, am_fragments** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!c || !f) return fail(AM_ERR_INVALID, "null index or fragments");
    AM_TRY(check_unit(unit));
    AM_TRY(check_source(c, f->unit, f->n_hay, f->src_total, f->dev, "am_coords_fragments", "fragments"));
    AM_TRY(check_index(c, unit, false, "am_coords_fragments"));
    AM_TRY(ensure_runtime());
    FragmentsPtr r(new am_fragments(), am_fragments_free);
    r->src_total = f->src_total; r->unit = unit;
    if (f->n_hay == 0) { r->make_empty(f->dev); *out = r.release(); return AM_OK; }
    r->dev = f->dev; r->n_hay = f->n_hay; r->n_items = f->n_items;
    ON_DEVICE(c->dev);
    hipStream_t st; AM_TRY(get_stream(c->dev, &st));
    AM_TRY(copy_offsets(r.get(), f->offsets, f->n_hay, st));
    if (f->n_items) {
        AM_TRY(r->data.ensure(f->n_items * sizeof(Fragment)));
        if (unit == AM_UNIT_BYTES) HIP_TRY(hipMemcpyAsync(r->data.p, f->data.p, f->n_items * sizeof(Fragment), hipMemcpyDeviceToDevice, st));
        else { Prof pr("coords_fragments", st);
               HIP_TRY(launch_coords_fragments(c->in(), unit, (const Fragment*)f->data.p, (const uint64_t*)f->offsets.p, f->n_items, (Fragment*)r->data.p, st)); }
    }
    HIP_TRY(hipStreamSynchronize(st));
    *out = r.release();
    return AM_OK;
}

extern "C" int am_coords_ranges(const am_coords* c, const struct am_spans* s, int unit, am_ranges** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_spans_call(c, s, unit, true, "am_coords_ranges"));
    AM_TRY(ensure_runtime());
    if (s->n_hay == 0) return empty_result(s->dev, out);
    RangesPtr r(new am_ranges(), am_ranges_free);
    r->dev = s->dev; r->n_hay = s->n_hay; r->n_items = s->n_items;
    ON_DEVICE(c->dev);
    hipStream_t st; AM_TRY(get_stream(c->dev, &st));
    AM_TRY(copy_offsets(r.get(), s->offsets, s->n_hay, st));
    if (s->n_items) {
        AM_TRY(r->data.ensure(s->n_items * sizeof(SpanRange)));
        Prof pr("coords_ranges", st);
        HIP_TRY(launch_coords_ranges(c->in(), unit, (const Span*)s->data.p, s->n_items, (SpanRange*)r->data.p, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    *out = r.release();
    return AM_OK;
}

extern "C" int am_coords_positions_device(const am_coords* c, const void* d_hay, const void* d_pos, uint64_t n, int unit, void* d_out)
{
    AM_TRY(check_positions_call(c, d_hay, d_pos, n, unit, d_out));
    if (n == 0) return AM_OK;
    AM_TRY(ensure_runtime());
    ON_DEVICE(c->dev);
    hipStream_t st; AM_TRY(get_stream(c->dev, &st));
    return positions_device(c, (const uint32_t*)d_hay, (const uint64_t*)d_pos, n, unit, (uint64_t*)d_out, st);
}

extern "C" int am_coords_positions(const am_coords* c, const uint32_t* hay, const uint64_t* pos, uint64_t n, int unit, uint64_t* out)
{
    AM_TRY(check_positions_call(c, hay, pos, n, unit, out));
    if (n == 0) return AM_OK;
    AM_TRY(ensure_runtime());
    ON_DEVICE(c->dev);
    hipStream_t st; AM_TRY(get_stream(c->dev, &st));
    DevBuf d_hay, d_pos, d_out;
    AM_TRY(d_hay.ensure(n * 4));
    AM_TRY(d_pos.ensure(n * 8));
    AM_TRY(d_out.ensure(n * 8));
    HIP_TRY(hipMemcpyAsync(d_hay.p, hay, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_pos.p, pos, n * 8, hipMemcpyHostToDevice, st));
    AM_TRY(positions_device(c, (const uint32_t*)d_hay.p, (const uint64_t*)d_pos.p, n, unit, (uint64_t*)d_out.p, st));
    HIP_TRY(hipMemcpyAsync(out, d_out.p, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return AM_OK;
}

extern "C" uint64_t am_ranges_size(const am_ranges* r) { return r ? r->n_items : 0; }
extern "C" uint64_t am_ranges_haystacks(const am_ranges* r) { return r ? r->n_hay : 0; }
extern "C" const void* am_ranges_device_offsets(const am_ranges* r) { return r ? r->offsets.p : nullptr; }
extern "C" const void* am_ranges_device_data(const am_ranges* r) { return r && r->n_items ? r->data.p : nullptr; }

extern "C" const uint64_t* am_ranges_offsets(am_ranges* r)
{
    if (!r) { fail(AM_ERR_INVALID, "null ranges"); return nullptr; }
    return r->fetch_offsets("the ranges");
}

extern "C" const am_span_range* am_ranges_data(am_ranges* r)
{
    if (!r) { fail(AM_ERR_INVALID, "null ranges"); return nullptr; }
    return r->fetch_data("the ranges");
}

extern "C" void am_ranges_free(am_ranges* r) { delete r; }
