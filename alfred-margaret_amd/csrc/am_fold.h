// am_fold.h -- the host-side scaffolding the device folds over a scan's records share (am_splitter.cpp, am_spans.cpp, am_contains_all.cpp): the argument checks of
// their entry points, the CSR result handle (am_fragments, am_needle_matrix, am_spans), the finisher of long chains (pointer doubling) and the loop that sends host
// slices up in segments and folds each in HBM.  The kernels differ from fold to fold; what is here does not.  Included at the end of am_host.h; internal.
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
    // noun: what the error text calls the result ("the fragments").  A fetch of zero items answers with a pointer to one placeholder element, never NULL.
    const uint64_t* fetch_offsets(const char* noun) { return fetch(h_offsets, offsets_fetched, offsets, n_hay + 1, noun); }
    const Item* fetch_data(const char* noun) { return fetch(h_data, data_fetched, data, n_items, noun); }

private:
    template <class T>
    const T* fetch(std::vector<T>& host, bool& fetched, const DevBuf& d, uint64_t n, const char* noun)
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

// ---- chains.  A fold that keeps a path head, next[head], next[next[head]], ... of every chain lets the head's lane walk a short chain and leaves the long ones to
// pointer doubling (am_split.hip): this is everything between "the walk kernel has been launched" and "the kept flags are final".
inline int read_u64(const void* d_src, uint64_t* out, hipStream_t st)
{
    HIP_TRY(hipMemcpyAsync(out, d_src, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return AM_OK;
}

// n elements with their kept flags; flag: 64 bytes the caller cleared before its walk kernel, word 0 = chains the walk left unfinished, word 1 = marks of a round.
// launch_next(jump) launches the caller's *_next kernel, which writes next[] into jump[n].  *rounds_out = the doubling rounds (0: every chain was short).
template <class Next>
int finish_long_chains(uint64_t n, uint32_t* kept, uint32_t* flag, Next&& launch_next, const char* prof_next, const char* prof_double, uint32_t* rounds_out, hipStream_t st)
{
    *rounds_out = 0;
    uint32_t long_chains = 0;
    if (n > 1) {
        HIP_TRY(hipMemcpyAsync(&long_chains, flag, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (!long_chains) return AM_OK;
    DevBuf jump0, jump1;
    AM_TRY(jump0.ensure(n * 8));
    AM_TRY(jump1.ensure(n * 8));
    uint64_t* jump[2] = {(uint64_t*)jump0.p, (uint64_t*)jump1.p};
    { Prof pr(prof_next, st);
      HIP_TRY(launch_next(jump[0])); }
    uint32_t rounds = 0;
    for (uint32_t marked = 1; marked != 0 && rounds < 64; rounds++) {      // (a path of k elements is marked after log2(k) + 1 rounds: 64 is no limit for 64-bit indices)
        HIP_TRY(hipMemsetAsync(flag + 1, 0, 4, st));
        { Prof pr(prof_double, st);
          HIP_TRY(launch_split_double(jump[rounds & 1], jump[(rounds & 1) ^ 1], n, kept, flag + 1, st)); }
        HIP_TRY(hipMemcpyAsync(&marked, flag + 1, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));                  // (the last round's: the jump arrays are free to go)
    }
    *rounds_out = rounds;
    return AM_OK;
}

// ---- host slices -> batches -> a fold per batch.  fold(b, first) folds batch b, whose haystack 0 is haystack `first` of the call, and returns when the device has
// finished with b.  The caller has made `dev` current.
constexpr uint64_t kFoldSegmentedFrom = 1ull << 30;         // as am_run: host batches from here on go up in segments of whole haystacks
constexpr uint64_t kFoldSegment = 256ull << 20;

template <class Fold>
int fold_slices(int dev, const am_slice* hay, size_t n_hay, uint64_t total, Fold&& fold)
{
    const long forced = cfg::get(cfg::kRunSegments);       // (the switch of am_run's segments: 0 = never, k > 0 = always, segments of k KiB)
    if (n_hay < 2 || forced == 0 || (forced < 0 && total < kFoldSegmentedFrom)) {
        am_batch* b = oneshot_batch(dev);                   // this thread's batch on the device
        int rc = upload_batch(hay, n_hay, b, true);
        if (rc == AM_OK) rc = fold(b, (size_t)0);
        oneshot_batch_trim(dev);
        return rc;
    }
    // Segments of whole haystacks into two batches that take turns: while this thread uploads segment k + 1, a thread of its own scans segment k and folds its
    // records in HBM.  The worker is joined before the next one starts: folds see the segments one after the other, in order.
    std::unique_ptr<am_batch, void (*)(am_batch*)> second(new am_batch(), am_batch_destroy);
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

}  // namespace host
}  // namespace am
