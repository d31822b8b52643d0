// am_splitter.cpp -- Data.Text.AhoCorasick.Splitter on the device (reference: src/Data/Text/AhoCorasick/Splitter.hs): one scan of the batch with the one-needle
// automaton, then stepAccum / finalizeAccum (:141-170) over the sorted records in HBM (am_split.hip).  What comes back is a list of (start, length) per haystack that
// stays in HBM until asked for, and am_batch_from_fragments turns it into a batch of its own: document -> lines -> any *_batch entry point, without the host.
// The result handle, the chain selector's host sequence and the argument checks are am_fold.h's, shared with the other folds.
#include "am_host.h"

using namespace am;
using namespace am::dev;
using namespace am::host;

struct am_splitter {
    const am_automaton* a = nullptr;
    uint32_t sep_bytes = 0, sep_cps = 0;
};

namespace {

constexpr uint32_t kSplitChainLimit = 32;                 // records the lane of a chain's head looks at before the chain goes to the doubling rounds
std::atomic<uint32_t> g_split_rounds{0};                  // doubling rounds of the last am_split_batch (am_debug_split_rounds)

struct Bufs {
    DevBuf start, head, kept, kidx, scan_tmp, rec_first;
};

}  // namespace

extern "C" uint32_t am_debug_split_rounds(void) { return g_split_rounds.load(std::memory_order_relaxed); }

extern "C" int am_splitter_create(const am_automaton* a, uint32_t sep_len_bytes, uint32_t sep_len_code_points, am_splitter** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!a) return fail(AM_ERR_INVALID, "null automaton");
    if (sep_len_bytes == 0 || sep_len_code_points == 0) return fail(AM_ERR_INVALID, "the empty separator is refused");
    if (sep_len_code_points > sep_len_bytes) return fail(AM_ERR_INVALID, "sep_len_code_points exceeds sep_len_bytes");
    // Splitter.hs:66 `Aho.build [(sep, ())]`: exactly one state reports, and it reports one value
    if (!a->has_ref) return fail(AM_ERR_UNSUPPORTED, "am_splitter_create: a handle made from an image does not keep values_len");
    size_t reporting = 0, values = 0;
    for (uint32_t v : a->values_len) if (v) { reporting++; values += v; }
    if (reporting != 1 || values != 1) return fail(AM_ERR_INVALID, "am_splitter_create: not a one-needle automaton");
    am_splitter* s = new am_splitter();
    s->a = a; s->sep_bytes = sep_len_bytes; s->sep_cps = sep_len_code_points;
    *out = s;
    return AM_OK;
}

extern "C" void am_splitter_destroy(am_splitter* s) { delete s; }

extern "C" int am_split_batch(const am_splitter* s, int case_mode, const am_batch* cb, am_fragments** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!s || !cb) return fail(AM_ERR_INVALID, "null splitter or batch");
    AM_TRY(check_case(case_mode));
    if (s->a->dev != cb->dev) return fail(AM_ERR_INVALID, "splitter and batch live on different devices");
    AM_TRY(ensure_runtime());
    am_batch* b = const_cast<am_batch*>(cb);
    std::unique_ptr<am_fragments, void (*)(am_fragments*)> f(new am_fragments(), am_fragments_free);
    f->dev = b->dev; f->n_hay = b->n_hay; f->src_total = b->total;
    g_split_rounds.store(0, std::memory_order_relaxed);
    if (b->n_hay == 0) return empty_result(b->dev, out);
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    RecordArray ra(b->dev);
    uint64_t n_rec = 0;
    if (b->total != 0) AM_TRY(run_records(s->a, case_mode, b, records_into(ra), &n_rec));
    const SplitIn in{(const Record*)ra.p, n_rec, (const uint8_t*)b->d_text, b->d_offsets, b->total, b->n_hay, s->sep_bytes, s->sep_cps};
    Bufs w;
    AM_TRY(w.start.ensure((n_rec + 1) * 8));
    AM_TRY(w.head.ensure(n_rec + 1));
    AM_TRY(w.kept.ensure((n_rec + 1) * 4));
    AM_TRY(w.kidx.ensure((n_rec + 1) * 8));
    AM_TRY(w.rec_first.ensure(((uint64_t)b->n_hay + 1) * 8));
    uint32_t* const kept = (uint32_t*)w.kept.p;
    { Prof pr("split_start", st);
      HIP_TRY(launch_split_start(case_mode == AM_IGNORE_CASE, in, (uint64_t*)w.start.p, (uint8_t*)w.head.p, kept, st)); }
    HIP_TRY(launch_rp_ranges(in.recs, n_rec, (uint64_t*)w.rec_first.p, kNoRoute, b->n_hay, st));
    uint32_t rounds = 0;
    uint64_t n_kept = 0;
    AM_TRY(select_chains(SplitChain{in.recs, (const uint64_t*)w.start.p, n_rec}, (const uint8_t*)w.head.p, kept, (uint64_t*)w.kidx.p, w.scan_tmp,
                         cfg::get(cfg::kSplitChainLimit), kSplitChainLimit, {"split_walk", "split_next", "split_double"}, &n_kept, &rounds, st));
    g_split_rounds.store(rounds, std::memory_order_relaxed);
    f->n_items = n_kept + b->n_hay;
    AM_TRY(f->data.ensure(f->n_items * sizeof(Fragment)));
    AM_TRY(f->offsets.ensure(((uint64_t)b->n_hay + 1) * 8));
    { Prof pr("split_emit", st);
      HIP_TRY(launch_split_emit(in, (const uint64_t*)w.start.p, kept, (const uint64_t*)w.kidx.p, (const uint64_t*)w.rec_first.p, (uint64_t*)f->offsets.p,
                                (Fragment*)f->data.p, f->n_items, st)); }
    HIP_TRY(hipStreamSynchronize(st));                      // (the record array goes back to the cache, the workspaces are freed)
    *out = f.release();
    return AM_OK;
}

extern "C" int am_split(const am_splitter* s, int case_mode, const am_slice* hay, size_t n_hay, am_fragments** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!s) return fail(AM_ERR_INVALID, "null splitter");
    AM_TRY(check_slices(hay, n_hay));
    AM_TRY(check_case(case_mode));
    AM_TRY(ensure_runtime());
    const int dev = s->a->dev;
    if (n_hay == 0) return empty_result(dev, out);
    return with_oneshot_batch(dev, hay, n_hay, [&](am_batch* b) { return am_split_batch(s, case_mode, b, out); });
}

extern "C" uint64_t am_fragments_size(const am_fragments* f) { return f ? f->n_items : 0; }
extern "C" uint64_t am_fragments_haystacks(const am_fragments* f) { return f ? f->n_hay : 0; }
extern "C" const void* am_fragments_device_offsets(const am_fragments* f) { return f ? f->offsets.p : nullptr; }
extern "C" const void* am_fragments_device_data(const am_fragments* f) { return f ? f->data.p : nullptr; }

extern "C" const uint64_t* am_fragments_offsets(am_fragments* f)
{
    if (!f) { fail(AM_ERR_INVALID, "null fragments"); return nullptr; }
    return f->fetch_offsets("the fragments");
}

extern "C" const am_fragment* am_fragments_data(am_fragments* f)
{
    if (!f) { fail(AM_ERR_INVALID, "null fragments"); return nullptr; }
    return f->fetch_data("the fragments");
}

extern "C" void am_fragments_free(am_fragments* f) { delete f; }

extern "C" int am_batch_from_fragments(const am_batch* src, const am_fragments* f, am_batch** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!src || !f) return fail(AM_ERR_INVALID, "null batch or fragments");
    if (f->unit != AM_UNIT_BYTES) return fail(AM_ERR_INVALID, "am_batch_from_fragments: the fragments are in converted units (am_coords_fragments); the gather reads byte fragments");
    if (f->n_hay != src->n_hay || f->src_total != src->total || f->dev != src->dev)
        return fail(AM_ERR_INVALID, "the fragments were not produced from a batch with this haystack count and size");
    if (f->n_items >= 0xFFFFFFFFull) return fail(AM_ERR_UNSUPPORTED, "am_batch_from_fragments: 2^32 - 1 fragments and more do not fit a batch");
    AM_TRY(ensure_runtime());
    ON_DEVICE(src->dev);
    hipStream_t st; AM_TRY(get_stream(src->dev, &st));
    DerivedBatch nb;
    nb.begin(src->dev);
    const uint64_t n = f->n_items;
    DevBuf lens, src_at, scan_tmp;
    AM_TRY(lens.ensure((n + 1) * 8));
    AM_TRY(src_at.ensure((n + 1) * 8));
    uint64_t* new_off; uint8_t* new_text;
    AM_TRY(nb.offsets(n, &new_off));
    HIP_TRY(launch_split_sources((const Fragment*)f->data.p, n, (const uint64_t*)f->offsets.p, src->d_offsets, src->n_hay, src->total, (uint64_t*)lens.p, (uint64_t*)src_at.p, st));
    uint64_t total = 0;
    AM_TRY(exclusive_sum64(scan_tmp, (const uint64_t*)lens.p, new_off, n + 1, st, &total));
    AM_TRY(nb.text(total, st, &new_text));
    { Prof pr("split_gather", st);
      HIP_TRY(launch_split_gather((const uint8_t*)src->d_text, src->total, (const uint64_t*)src_at.p, new_off, n, total, new_text, g_rt.dev[src->dev].n_cu, st)); }
    HIP_TRY(hipStreamSynchronize(st));                      // a batch object may be used from any thread and stream afterwards
    return nb.publish(total, n, out);
}
