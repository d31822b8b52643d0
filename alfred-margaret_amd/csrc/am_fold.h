// am_fold.h -- the host-side scaffolding the device stages share (am_splitter.cpp, am_spans.cpp, am_subst.cpp, am_select.cpp, am_extract.cpp, am_contains_all.cpp, am_score.cpp and the
// one-shot entry points of am_abi.cpp): the argument checks of their entry points (a held result's among them: matches_in_hbm, matches_below), the CSR result handle (am_fragments, am_needle_matrix, am_spans), the exclusive sum, the chain
// selector's host sequence, the one-shot form of an entry point, the loop that sends host slices up in segments and folds each in HBM, and the builder of the batches the
// library derives in HBM.  The kernels differ from stage to stage; what is here does not.  Included at the end of am_host.h; internal.
#pragma once

namespace am {
namespace host {

// ---- argument checks.  None of them touches the device: every entry point runs its checks before ensure_runtime(), so a caller without a GPU sees them all.
inline int check_case(int case_mode)
{
    return case_mode == AM_CASE_SENSITIVE || case_mode == AM_IGNORE_CASE ? AM_OK : fail(AM_ERR_INVALID, "case_mode must be AM_CASE_SENSITIVE or AM_IGNORE_CASE");
}

// the host slices of a one-shot call; *total = their bytes
inline int check_slices(const am_slice* hay, size_t n_hay, uint64_t* total = nullptr)
{
    if (n_hay && !hay) return fail(AM_ERR_INVALID, "hay is null");
    if (n_hay >= 0xFFFFFFFFull) return fail(AM_ERR_INVALID, "too many haystacks");
    uint64_t bytes = 0;
    for (size_t i = 0; i < n_hay; i++) { if (hay[i].len && !hay[i].ptr) return fail(AM_ERR_INVALID, "slice with null ptr"); bytes += hay[i].len; }
    if (total) *total = bytes;
    return AM_OK;
}

// a result whose records a fold can read: in HBM, on the device of the values table
inline int matches_in_hbm(const am_matches* m, const am_needle_ids* ids, const char* entry)
{
    if (m->n && !m->d_records) return fail(AM_ERR_UNSUPPORTED, std::string(entry) + ": the result was assembled on the host (am_run on a large host batch) and has no records in HBM");
    if (m->dev != ids->a->dev) return fail(AM_ERR_INVALID, "result and values table live on different devices");
    return AM_OK;
}

// ... and whose haystack fields all lie below n_hay: the records are sorted by haystack, so the last one, read back here, carries the largest index
inline int matches_below(const am_matches* m, size_t n_hay, const char* entry, hipStream_t st)
{
    if (m->n == 0) return AM_OK;
    Record last;
    HIP_TRY(hipMemcpyAsync(&last, m->d_records + m->first + m->n - 1, sizeof(Record), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (last.haystack >= n_hay) return fail(AM_ERR_INVALID, std::string(entry) + ": n_hay is not greater than the largest haystack index of the result");
    return AM_OK;
}

// ---- the host copy of n elements a result keeps in HBM, made once, on first use (the CSR results below, am_selection).  noun: what the error text calls them.  A fetch
// of zero elements answers with a pointer to one placeholder element, never NULL.
template <class T>
const T* fetch_once(std::vector<T>& host, bool& fetched, int dev, const DevBuf& d, uint64_t n, const char* noun)
{
    if (fetched) return host.data();
    try { host.resize((size_t)std::max<uint64_t>(n, 1)); } catch (const std::exception&) { fail(AM_ERR_OOM, std::string("no host memory for ") + noun); return nullptr; }
    if (n) {
        if (ensure_runtime() != AM_OK) return nullptr;
        OnDevice od(dev);
        hipStream_t st;
        if (od.rc != AM_OK || get_stream(dev, &st) != AM_OK) return nullptr;
        if (hipMemcpyAsync(host.data(), d.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            fail(AM_ERR_HIP, std::string("copying ") + noun + " to the host failed");
            return nullptr;
        }
    }
    fetched = true;
    return host.data();
}

// ---- the CSR result of a fold: Item[n_items] and uint64[n_hay + 1] row offsets that stay in HBM until asked for; the host copies are made once, on first use.
// (Holds DevBufs: on the heap only, see THE RULE above DevBuf.)
template <class Item>
struct CsrResult {
    int dev = 0;
    uint64_t n_items = 0, n_hay = 0;
    DevBuf data, offsets;                                   // Item[n_items], uint64[n_hay + 1] in HBM (none when n_hay == 0)
    std::vector<Item> h_data; std::vector<uint64_t> h_offsets;
    bool data_fetched{false}, offsets_fetched{false};

    // no haystacks: zero items, offsets = [0], nothing in HBM
    void make_empty(int d)
    {
        dev = d;
        h_offsets.assign(1, 0); h_data.assign(1, Item{});
        offsets_fetched = data_fetched = true;
    }
    // noun: what the error text calls the result ("the fragments")
    const uint64_t* fetch_offsets(const char* noun) { return fetch_once(h_offsets, offsets_fetched, dev, offsets, n_hay + 1, noun); }
    const Item* fetch_data(const char* noun) { return fetch_once(h_data, data_fetched, dev, data, n_items, noun); }
};

// the result of a call without haystacks
template <class Result>
int empty_result(int dev, Result** out)
{
    Result* r = new Result();
    r->make_empty(dev);
    *out = r;
    return AM_OK;
}

// ---- exclusive sums (am_scan.hip).  out[i] = in[0] + ... + in[i - 1] for i < n; tmp is the scan's temporary, grown when it is too small (a buffer that moves
// is freed: no stream work may be pending on it); total (nullable) = out[n - 1], read back -- the callers' inputs end in a zero, so that is the sum of them all.
inline int read_u64(const void* d_src, uint64_t* out, hipStream_t st)
{
    HIP_TRY(hipMemcpyAsync(out, d_src, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return AM_OK;
}

inline int exclusive_sum(DevBuf& tmp, const uint32_t* in, uint64_t* out, uint64_t n, hipStream_t st, uint64_t* total = nullptr)
{
    size_t bytes = 0;
    HIP_TRY(scan_temp_bytes(n, &bytes));
    AM_TRY(tmp.ensure(bytes));
    HIP_TRY(launch_scan(tmp.p, tmp.cap, in, out, n, st));
    return total ? read_u64(out + n - 1, total, st) : AM_OK;
}

inline int exclusive_sum64(DevBuf& tmp, const uint64_t* in, uint64_t* out, uint64_t n, hipStream_t st, uint64_t* total = nullptr)
{
    size_t bytes = 0;
    HIP_TRY(scan64_temp_bytes(n, &bytes));
    AM_TRY(tmp.ensure(bytes));
    HIP_TRY(launch_scan64(tmp.p, tmp.cap, in, out, n, st));
    return total ? read_u64(out + n - 1, total, st) : AM_OK;
}

// ---- chains (am_chain.h): everything between "the stage has written head and kept = head" and "kept is final and counted".  The heads' lanes walk the short
// chains, pointer doubling finishes the ones beyond the limit, kidx = the exclusive sum of kept (v.n + 1 entries each, kept's last one 0) and *n_kept = kidx[v.n].
// knob: the stage's limit switch (kUnset or 0: dflt).  prof: the profile names of the walk, the next pass and a doubling round.  *rounds = the doubling rounds
// (0: every chain was short).
struct ChainProf { const char *walk, *next, *dbl; };

template <class View>
int select_chains(const View& v, const uint8_t* head, uint32_t* kept, uint64_t* kidx, DevBuf& scan_tmp, long knob, uint32_t dflt, const ChainProf& prof, uint64_t* n_kept,
                  uint32_t* rounds, hipStream_t st)
{
    const uint64_t n = v.n;
    *rounds = 0;
    DevBuf flag_buf, jump0, jump1;                          // 64 bytes: word 0 = chains the walk left unfinished, word 1 = marks of a round; next[] and its double
    AM_TRY(flag_buf.ensure(64));
    uint32_t* const flag = (uint32_t*)flag_buf.p;
    HIP_TRY(hipMemsetAsync(flag, 0, 64, st));
    { Prof pr(prof.walk, st);
      HIP_TRY(launch_chain_walk(v, head, kept, knob > 0 ? (uint32_t)std::min<long>(knob, 1L << 30) : dflt, flag, st)); }
    uint32_t long_chains = 0;
    if (n > 1) {
        HIP_TRY(hipMemcpyAsync(&long_chains, flag, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (long_chains) {
        AM_TRY(jump0.ensure(n * 8));
        AM_TRY(jump1.ensure(n * 8));
        uint64_t* jump[2] = {(uint64_t*)jump0.p, (uint64_t*)jump1.p};
        { Prof pr(prof.next, st);
          HIP_TRY(launch_chain_next(v, head, jump[0], st)); }
        uint32_t r = 0;
        for (uint32_t marked = 1; marked != 0 && r < 64; r++) {      // (a path of k elements is marked after log2(k) + 1 rounds: 64 is no limit for 64-bit indices)
            HIP_TRY(hipMemsetAsync(flag + 1, 0, 4, st));
            { Prof pr(prof.dbl, st);
              HIP_TRY(launch_chain_double(jump[r & 1], jump[(r & 1) ^ 1], n, kept, flag + 1, st)); }
            HIP_TRY(hipMemcpyAsync(&marked, flag + 1, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));              // (the last round's: the jump arrays are free to go)
        }
        *rounds = r;
    }
    return exclusive_sum(scan_tmp, kept, kidx, n + 1, st, n_kept);
}

// ---- the one-shot form of an entry point: the slices into the calling thread's batch on `dev`, form(b) -- the *_batch form -- if they went up, and the batch trimmed
// whatever came of either.  The entry point has made its own checks and early returns; upload_batch's (hay, the haystack count, then the runtime, then every slice's
// pointer) are the first thing that happens here, so this does not make the device current: upload_batch and the batch forms do that themselves.
template <class Form>
int with_oneshot_batch(int dev, const am_slice* hay, size_t n_hay, Form&& form)
{
    am_batch* b = oneshot_batch(dev);
    int rc = upload_batch(hay, n_hay, b, true);
    if (rc == AM_OK) rc = form(b);
    oneshot_batch_trim(dev);
    return rc;
}

// ---- host slices -> batches -> a fold per batch.  fold(b, first) folds batch b, whose haystack 0 is haystack `first` of the call, and returns when the device has
// finished with b.  The caller has made `dev` current.
constexpr uint64_t kFoldSegmentedFrom = 1ull << 30;         // as am_run: host batches from here on go up in segments of whole haystacks
constexpr uint64_t kFoldSegment = 256ull << 20;

template <class Fold>
int fold_slices(int dev, const am_slice* hay, size_t n_hay, uint64_t total, Fold&& fold)
{
    const long forced = cfg::get(cfg::kRunSegments);       // (the switch of am_run's segments: 0 = never, k > 0 = always, segments of k KiB)
    if (n_hay < 2 || forced == 0 || (forced < 0 && total < kFoldSegmentedFrom))
        return with_oneshot_batch(dev, hay, n_hay, [&](am_batch* b) { return fold(b, (size_t)0); });
    // Segments of whole haystacks into two batches that take turns: while this thread uploads segment k + 1, a thread of its own scans segment k and folds its
    // records in HBM.  The worker is joined before the next one starts: folds see the segments one after the other, in order.
    BatchPtr second(new am_batch(), am_batch_destroy);
    second->dev = dev;
    am_batch* turn[2] = {oneshot_batch(dev), second.get()};
    const uint64_t segment = forced > 0 ? (uint64_t)forced << 10 : kFoldSegment;
    std::thread worker;
    int rc = AM_OK, worker_rc = AM_OK; std::string worker_err;      // (am_last_error is per thread: the worker's goes to the caller's)
    auto join = [&] { if (worker.joinable()) worker.join(); if (rc == AM_OK && worker_rc != AM_OK) rc = fail(worker_rc, worker_err); };
    size_t k = 0;
    for (size_t i = 0; i < n_hay && rc == AM_OK; k++) {
        size_t j = i; uint64_t bytes = 0;
        while (j < n_hay && bytes < (i == 0 ? segment / 4 : segment)) bytes += hay[j++].len;      // (the first a quarter of the others: no scan runs beside its upload)
        am_batch* b = turn[k & 1];                          // (its last scan, segment k - 2, was joined before segment k - 1 started)
        rc = upload_batch(hay + i, j - i, b, false);
        join();
        if (rc != AM_OK) break;
        worker = std::thread([&, b, i] {
            worker_rc = fold(b, i);
            if (worker_rc != AM_OK) worker_err = am_last_error();
        });
        i = j;
    }
    join();
    oneshot_batch_trim(dev);
    return rc;
}

// ---- batches the library derives in HBM (the fragments, a selection, a splice, the groups of a fold): a batch of the library's own that owns its offsets and its
// text.  Kernels read whole 16-byte groups, so text() zeroes from the last whole group of the text to the padded end, on the stream and ahead of whatever the producer
// enqueues to write the bytes.  The producer waits for the device itself before ready() / publish(): it knows why.
struct DerivedBatch {
    BatchPtr b{nullptr, am_batch_destroy};
    void begin(int dev) { b.reset(new am_batch()); b->dev = dev; b->owns = true; }
    int offsets(uint64_t n_hay, uint64_t** p)               // room for n_hay + 1 offsets, which the producer writes
    {
        AM_TRY(b->offs_buf.ensure((n_hay + 1) * 8));
        *p = (uint64_t*)b->offs_buf.p;
        return AM_OK;
    }
    int text(uint64_t total, hipStream_t st, uint8_t** p)   // room for the padded text, its zero tail enqueued
    {
        const size_t padded = padded_text(total);
        const uint64_t whole = total & ~15ull;
        AM_TRY(b->text_buf.ensure(padded));
        *p = (uint8_t*)b->text_buf.p;
        HIP_TRY(hipMemsetAsync(*p + whole, 0, padded - whole, st));
        return AM_OK;
    }
    int ready(uint64_t total, uint64_t n_hay)               // offsets and text are in place: a batch like any other (again: the buffers serve the next fill)
    {
        b->d_text = b->text_buf.p; b->d_offsets = (uint64_t*)b->offs_buf.p;
        b->total = total; b->n_hay = (uint32_t)n_hay;
        return finish_batch(b.get());
    }
    int publish(uint64_t total, uint64_t n_hay, am_batch** out)
    {
        AM_TRY(ready(total, n_hay));
        *out = b.release();
        return AM_OK;
    }
    // a batch without haystacks: offsets = [0], one group of zeros
    static int empty(int dev, am_batch** out)
    {
        ON_DEVICE(dev);
        hipStream_t st; AM_TRY(get_stream(dev, &st));
        DerivedBatch nb;
        nb.begin(dev);
        uint64_t* off; uint8_t* text;
        AM_TRY(nb.offsets(0, &off));
        HIP_TRY(hipMemsetAsync(off, 0, 8, st));
        AM_TRY(nb.text(0, st, &text));
        HIP_TRY(hipStreamSynchronize(st));
        return nb.publish(0, 0, out);
    }
};

// haystacks [h0, h1) of b as a batch of its own in `sub` (ONE DerivedBatch serves group after group: the groups of fold_batch, am_contains_all.cpp, and of
// am_rules_eval_batch, am_rules.cpp): the text copied device to device to a 16-byte aligned start, the offsets rebased on the device.  o0 / o1: b's offsets at h0 /
// h1, which the caller has on the host.  Returns when the copies have finished: a batch like any other.
inline int sub_batch(const am_batch* b, uint64_t h0, uint64_t h1, uint64_t o0, uint64_t o1, DerivedBatch& sub, hipStream_t st)
{
    const uint64_t bytes = o1 - o0;
    uint64_t* sub_off; uint8_t* sub_text;
    AM_TRY(sub.text(bytes, st, &sub_text));
    AM_TRY(sub.offsets(h1 - h0, &sub_off));
    if (bytes) HIP_TRY(hipMemcpyAsync(sub_text, (const uint8_t*)b->d_text + o0, bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(launch_offsets_rebase(b->d_offsets + h0, h1 - h0 + 1, 0 - o0, sub_off, st));      // (base + local[i] in 64-bit arithmetic: local[i] - o0)
    HIP_TRY(hipStreamSynchronize(st));
    return sub.ready(bytes, h1 - h0);
}

}  // namespace host
}  // namespace am

// the result of am_split* (am_splitter.cpp) and of am_fragments_from_spans (am_extract.cpp): what am_batch_from_fragments turns into a batch
struct am_fragments : am::host::CsrResult<am_fragment> {
    uint64_t src_total = 0;                               // bytes of the batch they were cut from (am_batch_from_fragments checks it)
    int unit = AM_UNIT_BYTES;                             // what start / len are in; anything else: made by am_coords_fragments, refused by am_batch_from_fragments
};
static_assert(sizeof(am_fragment) == sizeof(am::dev::Fragment), "am_fragment and the kernels' Fragment are one layout");
