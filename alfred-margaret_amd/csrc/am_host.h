// am_host.h -- what the host-side translation units of libam share (am_abi.cpp: runtime and thread state, automata, batches, one-shot entry points, results;
// am_run.cpp: routes and scans; am_replacer.cpp: the Replacer; am_contains_all.cpp: the values table (am_needle_ids, which records_in below turns into the kernels' view), containsAll, the fold checksum, the per-needle counts and the needle matrix;
// am_splitter.cpp: the Splitter; am_spans.cpp: match spans; am_subst.cpp: substitute; am_select.cpp: select; am_rules.cpp: rule sets; am_score.cpp: scores -- substitute, select and scores through
// am_spans.h, which adds the span table and the spans result): error handling, the per-device runtime, device buffers, the handle structs of include/am.h and the few scan entry points the Replacer
// drives.  am_fold.h, included at the end, holds the scaffolding of the device stages: argument checks, the CSR result handle, the chain finisher, the one-shot
// wrapper, the segment loop and the builder of derived batches.  Internal: nothing here is part of the C ABI.
#pragma once
#include "../../include/am.h"
#include "../../include/am_debug.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "am_config.h"
#include "am_device.h"
#include "am_flatten.h"

namespace am { int abi_fail(int code, const std::string& msg); }      // sets the calling thread's am_last_error message (am_abi.cpp)

namespace am {
namespace host {

using namespace am::dev;

inline int fail(int code, const std::string& msg) { return am::abi_fail(code, msg); }
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(AM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define AM_TRY(expr) do { int rc_ = (expr); if (rc_ != AM_OK) return rc_; } while (0)

// ---- per-device runtime.  libam serves every visible HIP device from one process: a handle (automaton, batch, result,
// replacer) lives on the device that was current when it was made (or that its memory belongs to), every entry point makes
// that device current for the calling thread while it runs, and launches go to a stream that belongs to the CALLING THREAD
// (one library stream per thread and device, or the stream the thread gave with am_set_stream): calls from different
// threads do not serialise on a shared stream or lock.
constexpr int kMaxDev = 16;
struct DeviceInfo { int n_cu = 0; size_t hbm = 0; std::string name; };
struct Runtime {
    std::mutex mu;
    bool probed = false;
    int n_dev = 0;
    std::string why;
    DeviceInfo dev[kMaxDev];
    // profiling (process-wide totals per kernel name)
    std::atomic<bool> prof_on{false};
    struct Pending { std::string k; hipEvent_t a, b; int dev; };
    std::vector<Pending> pending;
    std::map<std::string, std::pair<double, uint64_t>> prof;
};
extern Runtime g_rt;

int ensure_runtime();
int get_stream(int dev, hipStream_t* st);                 // the calling thread's stream on `dev` (its own, or the one it gave with am_set_stream)

// RAII: makes `dev` current for the calling thread while an entry point runs
struct OnDevice {
    int prev = -1; bool switched = false; int rc = AM_OK;
    explicit OnDevice(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) { rc = fail(AM_ERR_HIP, "hipGetDevice failed"); return; }
        if (prev != dev) {
            hipError_t e = hipSetDevice(dev);
            if (e != hipSuccess) { rc = fail(AM_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e)); return; }
            switched = true;
        }
    }
    ~OnDevice() { if (switched) (void)hipSetDevice(prev); }
};
#define ON_DEVICE(dev) OnDevice on_device_guard_(dev); AM_TRY(on_device_guard_.rc)

// RAII HIP-event bracket around one kernel launch (only when profiling is enabled)
struct Prof {
    bool on; hipStream_t st; Runtime::Pending p;
    Prof(const char* k, hipStream_t s) : on(g_rt.prof_on.load(std::memory_order_relaxed)), st(s)
    {
        if (!on) return;
        p.k = k; p.dev = 0;
        (void)hipGetDevice(&p.dev);
        if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(p.a, st);
    }
    ~Prof()
    {
        if (!on) return;
        (void)hipEventRecord(p.b, st);
        std::lock_guard<std::mutex> lk(g_rt.mu);
        g_rt.pending.push_back(p);
    }
};

// Device memory of one owner; the destructor frees it, so an owner names its buffers once, as members.  THE RULE: no DevBuf, and no struct that holds one, has
// static or thread storage duration -- its destructor would call into HIP while the runtime is being torn down at process exit (the reason Orphans and
// pinned_cache() in am_abi.cpp are never destroyed).  Handles and workspaces live on the heap or on a call's stack.
inline std::atomic<uint64_t> g_device_buffer_bytes{0};      // bytes all live DevBufs hold (am_debug_device_buffer_bytes: the leak test)
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t n)
    {
        if (n <= cap) return AM_OK;
        release();
        size_t want = n + n / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return fail(e == hipErrorOutOfMemory ? AM_ERR_OOM : AM_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
        cap = want;
        g_device_buffer_bytes.fetch_add(want, std::memory_order_relaxed);
        return AM_OK;
    }
    void release()
    {
        if (p) { (void)hipFree(p); g_device_buffer_bytes.fetch_sub(cap, std::memory_order_relaxed); }
        p = nullptr; cap = 0;
    }
};

struct Flavor {
    bool ready = false;
    void* d_image = nullptr;
    size_t bytes = 0;
    uint64_t generation = 0;     // unique per uploaded image (an address can be reused): what a batch remembers its route by
    ImageHeader h;
    void* d_scan2 = nullptr;     // the two-word scan filter derived from the image's keys (am_image.h scan2_mask), beside the image; null: the rule does not apply
};
uint64_t next_image_generation();
// The image of `f` is on the current device: derive its two-word scan filter (scan2_derive) and put it there too.  host_image: the image's bytes where the caller
// has them, else null (the cold slots are read back from the device).
int attach_scan2(Flavor& f, const void* host_image);

}  // namespace host
}  // namespace am

struct am_automaton {
    int dev = 0;                 // the device its images live on
    std::vector<uint64_t> transitions, root_ascii;
    std::vector<uint32_t> offsets, values_len;
    bool has_ref = false;        // false for handles attached to a received image
    std::shared_ptr<const am::LowerTable> lower;   // the caller's lower-case table (am_automaton_create_ex); null: the built-in one
    std::vector<uint8_t> cs_image;   // CaseSensitive image flattened (= validated) at creation, uploaded on first use
    // the IgnoreCase image is flattened on a thread of its own WHILE am_automaton_create flattens (= validates) the CaseSensitive one: whichever mode the first scan
    // asks for, its image is there or nearly there (the reference's protocol times build + run together, benchmark/haskell/app/Main.hs:62-64,73)
    struct Flat { int rc = 0; std::string err; std::vector<uint8_t> img; };
    std::future<Flat> ic_pending;
    int kernel_pref = 0;
    std::mutex mu;
    am::host::Flavor fl[2];
};

struct am_batch {
    int dev = 0;
    void* d_text = nullptr; uint64_t* d_offsets = nullptr;
    bool owns = false;
    bool hidx_ready = false;     // the per-KiB haystack index depends only on the offsets: built once per batch
    uint64_t total = 0; uint32_t n_hay = 0;
    std::mutex mu;              // guards the workspaces below (calls on one batch serialise)
    am::host::DevBuf text_buf, offs_buf;  // backing store of d_text / d_offsets when the batch owns them
    am::host::DevBuf combo;               // ... or ONE buffer [offsets | text] for small batches that went up with a single copy
    am::host::DevBuf hidx, unit_counts, unit_offsets, scan_tmp, small, hay_counts, flags, unit_first, pool, block_next;
    am::host::DevBuf sparse, dense_counts, dense_offsets, dense_out;      // automata with the empty needle (dense pass)
    // the route a dictionary's image took on this batch the last time it was asked (am_run.cpp make_plan: a sample walk decides once per batch and image)
    uint64_t route_image = 0; bool route_dfa = false;        // (the image's generation; 0: not asked)
    uint32_t route_ends_per_kib = 0;                         // what the sample walk counted: sizes the token pool's first guess
};

struct am_matches {
    int dev = 0;
    am::dev::Record* d_records = nullptr; uint64_t n = 0; size_t cap_bytes = 0;
    uint64_t first = 0;                                  // the result is records [first, first + n) of the array (am_run_range keeps a sub-range)
    std::vector<am_match> host; bool fetched = false;
    am_match* big = nullptr; size_t big_cap = 0;         // large results: a host block of the library's own -- page-locked (big_pinned: the records are
    bool big_pinned = false;                             // DMA'd straight into it), or pageable and filled through pinned staging
};

// machineValues in flat form on the device (am_needle_ids_create, am_contains_all.cpp): what the folds over the records expand a state with
struct am_needle_ids {
    const am_automaton* a = nullptr;
    uint32_t n_needles = 0;
    uint64_t n_states = 0, n_values = 0;     // entries of vals_off - 1 / of vals
    am::host::DevBuf vals_off, vals;
};
// what a fold's kernels read (am_device.h): records [0, n_rec) of a scan, whose haystack fields are below n_hay, with the table
inline am::dev::RecordsIn records_in(const am_needle_ids* ids, const am::dev::Record* recs, uint64_t n_rec, uint32_t n_hay)
{
    return {recs, n_rec, (const uint64_t*)ids->vals_off.p, (const uint32_t*)ids->vals.p, ids->n_states, ids->n_values, ids->n_needles, n_hay};
}

// what am_rules_eval* leaves in HBM (am_rules.cpp; am_select_rule, am_select.cpp, reads it): rule-major bitmaps, first-rule-wins labels, per-rule counts; the host
// copies are made once, on first use.  Remembers the batch it was made from as am_selection does.  (Holds DevBufs: on the heap only.)
struct am_rule_hits {
    int dev = 0;
    uint64_t n_hay = 0, src_total = 0, n_rules = 0, hay_words = 0;
    am::host::DevBuf fired, labels, counts;                 // uint64[n_rules][hay_words], uint32[n_hay], uint64[n_rules]
    std::vector<uint64_t> h_fired, h_counts; std::vector<uint32_t> h_labels;
    bool fired_fetched = false, labels_fetched = false, counts_fetched = false;
};

// the weight columns of a scoring call in HBM beside the values table they are indexed by (am_score.cpp).  (Holds a DevBuf: on the heap only.)
struct am_weights {
    const am_needle_ids* ids = nullptr;                     // must outlive the weights
    int dev = 0;
    uint32_t n_cols = 0, n_needles = 0;
    am::host::DevBuf w;                                     // int64[n_cols][n_needles]
};

// what am_score* leaves in HBM (am_score.cpp; am_select_top_k / am_select_score, am_select.cpp, read it): int64[n_cols][n_hay], column after column; the host copy is
// made once, on first use.  Remembers the batch it was made from as am_selection does.  (Holds a DevBuf: on the heap only.)
struct am_scores {
    int dev = 0;
    uint64_t n_hay = 0, src_total = 0;
    bool src_total_known = true;                            // false: made from a held result (am_matches_score), which does not know the bytes of its batch
    uint32_t n_cols = 0;
    am::host::DevBuf scores;
    std::vector<int64_t> h_scores; bool fetched = false;
    const int64_t* column(uint32_t c) const { return (const int64_t*)scores.p + (uint64_t)c * n_hay; }
};

namespace am {
namespace host {

// Results of a call, device -> caller: small ones travel through the calling thread's pinned result buffer (an asynchronous copy into pageable
// memory is a blocking, staged copy inside the runtime), the caller's buffers are filled after the call's ONE stream synchronisation.  (Defined next
// to the thread state in am_abi.cpp.)
struct ResultCopies {
    struct Item { void* dst; size_t off, n; };
    Item items[4]; int n_items = 0; size_t used = 0;
    int add(void* dst, const void* d_src, size_t n, hipStream_t st);
    int finish(hipStream_t st);
};

// am_abi.cpp: what the scans, the Replacer and containsAll drive
int prepare(const am_automaton* ca, int case_mode, const Flavor** out);                      // the automaton's image for a case mode, on its device
int finish_batch(am_batch* b);                                                               // workspaces of a batch whose text and offsets are in place
// am_run.cpp, the scans.  am_run_batch (allow_small: the one-document path may take the call); am_run_range and the segmented am_run ask for the general path
int run_batch_impl(const am_automaton* a, int case_mode, const am_batch* cb, am_matches** out, bool allow_small);
// Where the per-haystack flags of a containsAny / containsAll scan go.  The scans leave them in HBM; the public entry points copy them to the caller (HostFlagSink), a
// select compacts them where they are (am_select.cpp).
struct FlagSink {
    virtual ~FlagSink() = default;
    virtual int begin(const am_batch* b) = 0;               // once, after the entry point's own checks and before any scan
    // the flags of the batch: n_hay bytes in HBM, the work that writes them enqueued on st.  Called with b->mu held where they are the batch's scratch (b->flags): the sink
    // has taken what it needs when it returns
    virtual int device(const uint8_t* d_flags, hipStream_t st) = 0;
    virtual int constant(uint8_t v) = 0;                    // nothing was scanned: every flag is v
};
// ... into n_hay bytes of host memory, as am_contains_any_batch (clear_first: zeroed in begin) and am_contains_all_batch hand them out
struct HostFlagSink : FlagSink {
    uint8_t* out; bool clear_first; uint32_t n = 0;
    HostFlagSink(uint8_t* flags_out, bool clear) : out(flags_out), clear_first(clear) {}
    int begin(const am_batch* b) override
    {
        n = b->n_hay;
        if (n && !out) return fail(AM_ERR_INVALID, "flags_out is null");
        if (n && clear_first) std::memset(out, 0, n);
        return AM_OK;
    }
    int device(const uint8_t* d_flags, hipStream_t st) override
    {
        ResultCopies rc;
        AM_TRY(rc.add(out, d_flags, n, st));
        return rc.finish(st);
    }
    int constant(uint8_t v) override { if (n) std::memset(out, v, n); return AM_OK; }
};
// am_contains_any_batch / am_contains_all_batch with the flags handed to a sink (am_run.cpp, am_contains_all.cpp)
int contains_any_flags(const am_automaton* a, int case_mode, am_batch* b, FlagSink& sink);
int contains_all_flags(const am_needle_ids* ids, int case_mode, am_batch* b, FlagSink& sink);
// Searcher.containsAll without records (k_sf's ids mode): every reported needle id into the haystack's row of d_bits (n_hay x words, cleared here),
// flag h = 1 iff all n_needles ids were seen, handed to the sink; *taken = false when the automaton does not go this way (general kernel forced, the empty needle's
// dense pass, nothing to scan) and the caller folds the records instead.
int scan_needle_ids(const am_automaton* a, int case_mode, am_batch* b, const uint64_t* d_vals_off, const uint32_t* d_vals, uint32_t n_needles,
                    uint32_t* d_bits, uint32_t words, uint32_t* d_missing, FlagSink& sink, bool* taken);
// The slot rows of a batch (am_contains_all.cpp): d_bits[h * words + v / 32] bit v % 32 set iff the fold over haystack h meets value v < ids->n_needles; n_hay x words
// words that this call clears, d_missing: n_hay words of scratch.  The ids-mode scan where scan_needle_ids takes the call (no record is written), k_idset over the
// records elsewhere, in bounded record memory (fold_batch).  The work is enqueued on the calling thread's stream; what the scans read back they have read back.
int slot_rows(const am_needle_ids* ids, int case_mode, am_batch* b, uint32_t* d_bits, uint32_t words, uint32_t* d_missing);
// What is done with the sorted records of a scan while they are in HBM: records [0, n_rec) belong to haystacks [h0, h0 + n_hay) of the batch the caller handed to
// fold_batch, their haystack fields count from h0.  `scanned` is the batch the records index: the caller's, or the group's sub-batch with a text and offsets of its
// own -- a fold that reads text (the whole-word counts and scores) reads that one.  Returns when the device has finished with the records.
using RecordFold = std::function<int(const Record* recs, uint64_t n_rec, uint32_t h0, uint32_t n_hay, const am_batch* scanned, int dev, hipStream_t st)>;
// A device-resident batch scanned and folded in bounded record memory (am_contains_all.cpp): in one piece, or -- where the records would exceed the budget (1 GiB;
// AM_HIST_RECORDS_MIB) -- counted first and then scanned in groups of whole consecutive haystacks, each group folded before the next is scanned.  `fold` is not called
// for a scan without records.
int fold_batch(const am_needle_ids* ids, int case_mode, am_batch* b, const RecordFold& fold);
// The top-k flags of one column of a scores result (am_score.cpp; am_select_top_k and am_scores_top_k share it), 1 <= k < x->n_hay: d_flags (n_hay bytes, nullable) and
// d_keep (n_hay + 1 words, nullable) as launch_topk_flags writes them, enqueued on st.  The workspace lives in `work`, which the caller keeps until st has finished.
struct TopkBuffers { DevBuf state, tie, tie_rank, scan_tmp; };
int topk_flags(const am_scores* x, uint32_t column, uint64_t k, int largest, TopkBuffers& work, uint8_t* d_flags, uint32_t* d_keep, hipStream_t st);
// sorted records of a batch: sink_final(n, &ptr) names the destination once the count is known
int run_records(const am_automaton* a, int case_mode, am_batch* b, const std::function<int(uint64_t, Record**)>& sink_final, uint64_t* n_out, bool have_lock = false);
// the same without a host round trip (suffix-filter route, worst-case pool): the count stays on the device
int run_records_async(const am_automaton* a, int case_mode, am_batch* b, Record* d_out, const uint64_t** n_dev, hipStream_t st);
// am_abi.cpp: what the one-shot entry points of every stage share (through with_oneshot_batch and fold_slices, am_fold.h): the slices of a call into a batch, re-using its
// device buffers (oneshot: small uploads stay enqueued on the calling thread's stream), the calling thread's one-shot batch on a device and its trim after the call; and the
// device arrays of freed results (kept for the next records: taken from there or allocated, given back)
int upload_batch(const am_slice* hay, size_t n_hay, am_batch* b, bool oneshot);
am_batch* oneshot_batch(int dev);
void oneshot_batch_trim(int dev);
int record_array_get(int dev, size_t need, void** p, size_t* cap);
void record_array_put(int dev, void* p, size_t cap);
// a device array for records out of the cache of freed results; goes back there
struct RecordArray {
    int dev; void* p = nullptr; size_t cap = 0;
    explicit RecordArray(int d) : dev(d) {}
    int ensure(size_t need)
    {
        if (need <= cap) return AM_OK;
        record_array_put(dev, p, cap); p = nullptr; cap = 0;
        return record_array_get(dev, need, &p, &cap);
    }
    ~RecordArray() { record_array_put(dev, p, cap); }
};
using BatchPtr = std::unique_ptr<am_batch, void (*)(am_batch*)>;
inline size_t padded_text(uint64_t total) { return (size_t)((total + 15) & ~15ull) + 16; }
// the sink of run_records that puts the records into `d` (a DevBuf or a RecordArray), with room for `spare` more
template <class Buf>
auto records_into(Buf& d, uint64_t spare = 0)
{
    return [&d, spare](uint64_t n, Record** ptr) -> int { AM_TRY(d.ensure((n + spare) * sizeof(Record))); *ptr = (Record*)d.p; return AM_OK; };
}
// launch_rp_ranges for callers that want the record ranges alone
inline constexpr RpRoute kNoRoute{nullptr, nullptr, nullptr, nullptr, nullptr};

}  // namespace host
}  // namespace am

#include "am_fold.h"
