// am_run.cpp -- scanning: which kernel route a batch takes (make_plan) and the enqueueing of its passes -- the count, containsAny and ids scans, and the records of
// a batch by the general path (run_records), without a host round trip (run_records_async) and for one small document (run_records_small).
#include "am_host.h"

using namespace am;
using namespace am::dev;
using namespace am::host;

namespace {

// k_ac's launcher, handed over by libam_check.so when a test or bench.py's parity gate loads it (am_debug_set_general_kernel); never set in a product process
using AcLauncher = hipError_t (*)(bool ic, int mode, const AcView& a, const BatchView& b, const ScanOut& o, hipStream_t st);
std::atomic<AcLauncher> g_ac_launcher{nullptr};

constexpr uint64_t kDfaMinBytes = 32ull << 20;     // below this the suffix-filter route is the faster one even on natural text: a lane's walk of its unit (>= 128 bytes + warm-up, ~1 us per step) has a floor of 0.3 ms (natural text, 16 MiB: k_sf 0.26 / 0.36 ms counting / emitting, k_dfa 0.29 / 0.41; 32 MiB: 0.44 / 0.57 against 0.33 / 0.47)
constexpr uint64_t kDfaSampleBytes = 32ull << 20;   // from here on -- i.e. whenever the table walk is in question -- a sample walk asks the text which route it wants (round 5 asked from
                                                    // 64 MiB on: a dictionary over text that is not its language took the table walk at 32-64 MiB, 6 x slower than the filter there)
constexpr uint32_t kDfaEndsPerKiB = 48;            // needle ends per KiB from which the table walk wins (k_sf: 670 GiB/s at 10 per KiB, 215 at 63, 76 at 156; k_dfa: ~155 flat)

struct Plan {
    const Flavor* f; bool ic; bool use_sf; bool nothing; uint64_t n_units; uint32_t unit_chunks; int n_cu;
    bool use_dfa;        // the table-walk kernel (am_dfa.hip) on the general route's two passes; never together with use_sf
    DfaView dfa;
    DfaLaunch dfa_shape{};   // k_dfa's launch geometry for this call (use_dfa with something to scan): every launch, the retries and k_dfa_place take this one
    bool dense;          // automaton with the empty needle on the suffix-filter route: k_sf's records + the dense pass (am_dense.hip)
    AcView ac; SfView sf; BatchView bv;
    am_batch* batch;
    uint32_t* next_unit; // k_sf's unit counter (in the batch's `small` block: [0..1] total_values, [4] block counter, [5] overflow, [8] this)
};

// allow_dfa: the caller's route works for the general two-pass protocol (am_count_batch, am_contains_any_batch, run_records)
// have_lock: the caller holds b->mu already (run_records under reduce_dense)
int make_plan(const am_automaton* a, int case_mode, am_batch* b, Plan& p, bool allow_dfa = false, bool have_lock = false)
{
    if (!b) return fail(AM_ERR_INVALID, "null batch");
    if (!a) return fail(AM_ERR_INVALID, "null automaton");
    if (a->dev != b->dev) return fail(AM_ERR_INVALID, "automaton and batch live on different devices");
    AM_TRY(prepare(a, case_mode, &p.f));
    p.ic = case_mode == AM_IGNORE_CASE;
    if (a->kernel_pref == 2 && !p.f->h.sf_enabled) return fail(AM_ERR_UNSUPPORTED, "suffix-filter kernel cannot run this automaton (empty needle with too many prefix terminals)");
    p.dfa = make_dfa_view(p.f->d_image, p.f->h);
    bool has_dfa = p.f->h.dfa_n_states != 0 && p.f->h.root_vlen == 0;
    if (a->kernel_pref == 3 && !has_dfa) return fail(AM_ERR_UNSUPPORTED, "am_automaton_set_kernel(a, 3): this automaton's image has no DFA section");
    if (has_dfa) {
        ON_DEVICE(b->dev);
        if (!dfa_usable(p.dfa)) {                            // (a section this device cannot walk -- its LDS attribute refused, offsets beyond 32 bits -- is no error: the filter takes the batch)
            if (a->kernel_pref == 3) return fail(AM_ERR_UNSUPPORTED, "am_automaton_set_kernel(a, 3): the table-walk kernel cannot run this image on this device");
            has_dfa = false;
        }
    }
    if (has_dfa) {
        // A lane walks its unit byte after byte (~1 us per step): a unit of 2 048 bytes takes milliseconds however small the batch is.  The image's unit is for batches that
        // fill the machine (n_cu x 32 wavefronts x 64 lanes) with it; smaller batches get smaller units, down to 128 bytes (where the warm-up is a third of the walk).
        const long forced = cfg::get(cfg::kDfaChunk);
        if (forced < 64) {
            const uint64_t lanes = (uint64_t)g_rt.dev[b->dev].n_cu * 32u * 64u;
            uint64_t unit = ((b->total / (lanes ? lanes : 1)) + 15u) & ~15ull;
            if (unit < 128) unit = 128;
            if (unit < 4ull * p.dfa.warm) unit = (4ull * p.dfa.warm + 15u) & ~15ull;
            if (unit < p.dfa.chunk) p.dfa.chunk = (uint32_t)unit;
        }
    }
    p.use_dfa = has_dfa && allow_dfa && (a->kernel_pref == 3 || (a->kernel_pref == 0 && b->total >= (cfg::get(cfg::kDfaMinKiB) >= 0 ? (uint64_t)cfg::get(cfg::kDfaMinKiB) << 10 : kDfaMinBytes) && cfg::get(cfg::kDfa) != 0));
    if (p.use_dfa && a->kernel_pref == 0 && b->total >= kDfaSampleBytes) {
        // The table walk costs the same whatever the text is; the suffix filter is 6 x faster where needles are rare and slower where one ends every few bytes.  A large batch
        // is asked: 4 096 lanes spread over it walk 128 bytes each (0.15 ms); below kDfaEndsPerKiB needle ends per KiB the filter takes it.  Decided once per batch and image.
        std::unique_lock<std::mutex> lk(b->mu, std::defer_lock);
        if (!have_lock) lk.lock();
        if (b->route_image != p.f->generation) {
            ON_DEVICE(b->dev);
            hipStream_t st; AM_TRY(get_stream(b->dev, &st));
            AM_TRY(b->small.ensure(64));
            HIP_TRY(hipMemsetAsync(b->small.p, 0, 64, st));
            const uint32_t kSamples = b->total >= (64ull << 20) ? 4096u : 1024u, kLen = 128;       // (a smaller batch is asked with fewer lanes: 0.05 ms of a 0.3-ms scan)
            HIP_TRY(launch_dfa_sample(p.dfa, (const uint8_t*)b->d_text, b->total, kSamples, kLen, (uint32_t*)b->small.p, st));
            uint32_t ends = 0;
            HIP_TRY(hipMemcpyAsync(&ends, b->small.p, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            b->route_dfa = (uint64_t)ends * 1024u >= (uint64_t)kDfaEndsPerKiB * kSamples * kLen;
            b->route_ends_per_kib = (uint32_t)(((uint64_t)ends * 1024u + (uint64_t)kSamples * kLen - 1u) / ((uint64_t)kSamples * kLen));
            b->route_image = p.f->generation;
        }
        p.use_dfa = b->route_dfa;
    }
    p.use_sf = p.f->h.sf_enabled && a->kernel_pref != 1 && !p.use_dfa;
    if (!p.use_sf && !p.use_dfa && !g_ac_launcher.load(std::memory_order_acquire))
        return fail(AM_ERR_UNSUPPORTED, a->kernel_pref == 1 ? "am_automaton_set_kernel(a, 1): the general AC kernel is test infrastructure (libam_check.so) and is not loaded in this process"
                                                           : "this image has no suffix-filter section (sf_enabled == 0) and no table-walk section this batch could take: no kernel of the library can scan with it");
    p.dense = p.use_sf && p.f->h.root_vlen > 0;
    p.ac = make_ac_view(p.f->d_image, p.f->h);
    p.sf = make_sf_view(p.f->d_image, p.f->h);
    p.bv = BatchView{(const uint8_t*)b->d_text, b->d_offsets, (const uint32_t*)b->hidx.p, b->total, b->n_hay, 0};
    // no goto edge at all (no needles, or only empty needles): the reference never reports anything
    const bool no_edges = p.f->h.n_transitions == p.f->h.n_states;
    p.nothing = b->total == 0 || no_edges || (p.use_sf && p.f->h.sf_tiers == 0 && !p.dense);      // dense: first code points still report the root's values
    p.unit_chunks = p.use_sf ? sf_unit_chunks(p.bv, g_rt.dev[b->dev].n_cu) : 0;
    p.next_unit = nullptr;
    if (p.use_sf) { if (!b->small.p) return fail(AM_ERR_INVALID, "batch without its counter block (not made by am_batch_upload / am_batch_from_device)"); p.next_unit = (uint32_t*)b->small.p + 8; }
    p.n_cu = g_rt.dev[b->dev].n_cu;
    p.batch = b;
    p.n_units = p.nothing ? 0 : (p.use_sf ? (sf_chunks(p.bv) + p.unit_chunks - 1) / p.unit_chunks : p.use_dfa ? dfa_units(p.dfa, p.bv) : ac_units(p.ac, p.bv));
    if (p.n_units >= 0x7FFFFFF0ull) return fail(AM_ERR_UNSUPPORTED, "batch too large for one launch; split it");
    if (p.use_dfa && !p.nothing) { ON_DEVICE(b->dev); p.dfa_shape = dfa_launch_shape(p.dfa, p.bv, p.n_cu); }
    return AM_OK;
}

int launch_scan_kernel(const Plan& p, int mode, const ScanOut& o, hipStream_t st)
{
    if (p.use_sf) {
        ScanOut os = o;
        os.next_unit = p.next_unit;
        Prof pr("sf", st);
        HIP_TRY(launch_sf(p.ic, mode, p.sf, p.bv, os, p.n_cu, st, (const uint32_t*)p.f->d_scan2));
    }
    else if (p.use_dfa) {
        Prof pr("dfa", st);
        HIP_TRY(launch_dfa(mode, p.dfa, p.bv, o, p.dfa_shape, st));
    }
    else {
        // the general AC-walk kernel is test infrastructure (libam_check.so, tests/native/am_ac.hip): make_plan refused the scan if it is not loaded
        const AcLauncher ac = g_ac_launcher.load(std::memory_order_acquire);
        if (!ac) return fail(AM_ERR_UNSUPPORTED, "the general AC kernel is not loaded");
        Prof pr("ac", st);
        HIP_TRY(ac(p.ic, mode, p.ac, p.bv, o, st));
    }
    return AM_OK;
}

int build_hidx(const Plan& p, am_batch* b, hipStream_t st)
{
    if (b->hidx_ready) return AM_OK;
    Prof pr("hidx", st);
    HIP_TRY(launch_hidx(p.bv, (uint32_t*)b->hidx.p, (b->total >> kHidxShift) + 2, st));
    b->hidx_ready = true;
    return AM_OK;
}

// the haystack index and the clearing of (up to two) arrays in ONE launch when the index has to be built anyway -- the one-document call;
// with the index in place the arrays are cleared by memsets.  bytes0 / bytes1 are multiples of 4.
int build_hidx_and_clear(const Plan& p, am_batch* b, hipStream_t st, void* z0, size_t bytes0, void* z1, size_t bytes1)
{
    if (b->hidx_ready) {
        if (bytes0) HIP_TRY(hipMemsetAsync(z0, 0, bytes0, st));
        if (bytes1) HIP_TRY(hipMemsetAsync(z1, 0, bytes1, st));
        return AM_OK;
    }
    Prof pr("hidx", st);
    HIP_TRY(launch_hidx(p.bv, (uint32_t*)b->hidx.p, (b->total >> kHidxShift) + 2, st, (uint32_t*)z0, bytes0 / 4, (uint32_t*)z1, bytes1 / 4));
    b->hidx_ready = true;
    return AM_OK;
}

constexpr const char* kSfWatchdog = "suffix-filter kernel: internal hand-over between its wavefronts timed out (watchdog)";      // (pool_ctrl[2], i.e. word [6] of the batch's counter block)

// what every records pass of a batch scans with: unit_counts / unit_offsets of n = units + 1 entries (trailing zero: offsets[n_units] = total), the counter block, launch_scan's scratch
struct ScanSpace { uint64_t n = 0; size_t tmp_bytes = 0; };
int scan_workspaces(am_batch* b, uint64_t n_units, ScanSpace* s)
{
    s->n = n_units + 1;
    AM_TRY(b->unit_counts.ensure(s->n * sizeof(uint32_t)));
    AM_TRY(b->unit_offsets.ensure(s->n * sizeof(uint64_t)));
    AM_TRY(b->small.ensure(64));
    if (scan_temp_bytes(s->n, &s->tmp_bytes) != hipSuccess) return fail(AM_ERR_HIP, "scan sizing failed");
    return b->scan_tmp.ensure(s->tmp_bytes + 16);
}

// Blocks of k_sf's record pool.  Guess: a record per 128 haystack bytes + one block per unit -- or the pool that is there already when it is larger, or what AM_SF_POOL_BLOCKS
// says (tests: force the overflow / retry path).  WorstCase: a record at every byte (ceil(records / 64) per unit, records <= bytes): the pass cannot overflow.  Exact: the
// retry after an overflow, `drawn` = pool_ctrl[0] = the blocks the pass asked for.  All of them + the grants' unused remainders.
enum class SfPool { Guess, WorstCase, Exact };
uint64_t sf_pool_blocks(const Plan& p, SfPool mode, uint64_t drawn = 0)
{
    const am_batch* b = p.batch;
    const uint64_t slack = pool_grant_slack(p.n_cu, p.n_units, sf_lds_bytes(p.sf) <= 80 * 1024);
    if (mode == SfPool::Exact) return drawn + 64 + slack;
    if (mode == SfPool::WorstCase) return b->total / kPoolBlock + p.n_units + 8 + slack;
    uint64_t want = b->total / (128 * kPoolBlock) + p.n_units + 1024 + slack;
    if (b->pool.cap / (kPoolBlock * sizeof(Record)) > want) want = b->pool.cap / (kPoolBlock * sizeof(Record));
    if (cfg::get(cfg::kSfPoolBlocks) > 0) want = (uint64_t)cfg::get(cfg::kSfPoolBlocks);
    return want;
}

// One emitting k_sf pass on a batch (the caller holds b->mu): ONE scan pass writes records into pool blocks (chained per unit), then scan(unit_counts) + k_permute put them
// in order.  setup: the pool's workspaces and the kernel's arguments; scan: clears + haystack index, k_sf, unit offsets; permute: the sorted records.  Where the records
// go, who synchronises and what happens on an overflow (pool_ctrl[1]) is the caller's.
struct SfEmit {
    const Plan& p; hipStream_t st; ScanSpace sp;
    ScanOut o{};
    int setup(uint64_t want_blocks)
    {
        am_batch* b = p.batch;
        if (want_blocks >= (1ull << 26)) return fail(AM_ERR_UNSUPPORTED, "too many match records for one call (2^32 record slots); split the batch");      // k_sf addresses record slots with 32 bits
        AM_TRY(b->unit_first.ensure(2 * p.n_units * sizeof(uint32_t)));          // first block + slot count per unit
        AM_TRY(b->pool.ensure(want_blocks * kPoolBlock * sizeof(Record)));
        AM_TRY(b->block_next.ensure(want_blocks * sizeof(uint32_t)));
        o = ScanOut{};
        o.unit_chunks = p.unit_chunks;
        o.unit_counts = (uint32_t*)b->unit_counts.p;
        o.unit_first = (uint32_t*)b->unit_first.p;
        o.unit_slots = (uint32_t*)b->unit_first.p + p.n_units;
        o.pool = (Record*)b->pool.p;
        o.block_next = (uint32_t*)b->block_next.p;
        o.pool_ctrl = (uint32_t*)b->small.p + 4;            // small: [0..1] total_values, [4] blocks drawn, [5] overflow, [6] kernel watchdog
        o.n_blocks = (uint32_t)want_blocks;
        return AM_OK;
    }
    // fused_clear: the clears ride on the haystack index's launch when the index has to be built anyway (batches that are new every call); jobs_scan: few units take the
    // single-workgroup scan (one dispatch, no library sizing / configuration on the host)
    int scan(bool fused_clear, bool jobs_scan)
    {
        am_batch* b = p.batch;
        uint32_t* tail = (uint32_t*)b->unit_counts.p + p.n_units;
        if (fused_clear) AM_TRY(build_hidx_and_clear(p, b, st, b->small.p, 64, tail, sizeof(uint32_t)));
        else {
            HIP_TRY(hipMemsetAsync(b->small.p, 0, 64, st));
            HIP_TRY(hipMemsetAsync(tail, 0, sizeof(uint32_t), st));
            AM_TRY(build_hidx(p, b, st));
        }
        AM_TRY(launch_scan_kernel(p, kModeEmit, o, st));
        Prof pr("scan", st);
        if (jobs_scan && sp.n <= (1u << 16)) {
            ScanJobs jobs{}; jobs.n_jobs = 1;
            jobs.j[0] = ScanJob{(const uint32_t*)b->unit_counts.p, nullptr, (uint64_t*)b->unit_offsets.p, sp.n, nullptr};
            HIP_TRY(launch_scan_jobs(jobs, st));
        } else HIP_TRY(launch_scan(b->scan_tmp.p, sp.tmp_bytes, (const uint32_t*)b->unit_counts.p, (uint64_t*)b->unit_offsets.p, sp.n, st));
        return AM_OK;
    }
    int permute(Record* out) { Prof pr("permute", st); HIP_TRY(launch_permute(o, (const uint64_t*)p.batch->unit_offsets.p, out, p.n_units, st)); return AM_OK; }
};

}  // namespace

// count / containsAny of an automaton with the empty needle on the suffix-filter route: a record at almost every position, so
// the records are made (k_sf + dense pass) and reduced
static int reduce_dense(const am_automaton* a, int case_mode, am_batch* b, uint64_t* counts_out, uint64_t* total_out, FlagSink* flag_sink)
{
    uint64_t n_rec = 0;
    auto sink = [&](uint64_t n, Record** ptr) -> int { AM_TRY(b->dense_out.ensure(n * sizeof(Record))); *ptr = (Record*)b->dense_out.p; return AM_OK; };
    const Flavor* f = nullptr;
    AM_TRY(prepare(a, case_mode, &f));
    std::lock_guard<std::mutex> lk(b->mu);          // ONE lock over the scan and the reduction: b->dense_out must not be refilled by another thread in between
    AM_TRY(run_records(a, case_mode, b, sink, &n_rec, true));
    if (n_rec == 0) return flag_sink ? flag_sink->constant(0) : AM_OK;
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    AM_TRY(b->small.ensure(64));
    HIP_TRY(hipMemsetAsync(b->small.p, 0, 64, st));
    if (counts_out) { AM_TRY(b->hay_counts.ensure((size_t)b->n_hay * 8)); HIP_TRY(hipMemsetAsync(b->hay_counts.p, 0, (size_t)b->n_hay * 8, st)); }
    if (flag_sink) { AM_TRY(b->flags.ensure(b->n_hay)); HIP_TRY(hipMemsetAsync(b->flags.p, 0, b->n_hay, st)); }
    const AcView ac = make_ac_view(f->d_image, f->h);
    HIP_TRY(launch_records_reduce((const Record*)b->dense_out.p, n_rec, ac.vlen, counts_out ? (uint64_t*)b->hay_counts.p : nullptr, (uint64_t*)b->small.p,
                                  flag_sink ? (uint8_t*)b->flags.p : nullptr, st));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, b->small.p, 8, hipMemcpyDeviceToHost, st));
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, b->hay_counts.p, (size_t)b->n_hay * 8, hipMemcpyDeviceToHost, st));
    if (flag_sink) AM_TRY(flag_sink->device((const uint8_t*)b->flags.p, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (total_out) *total_out = total;
    return AM_OK;
}

extern "C" int am_count_batch(const am_automaton* a, int case_mode, const am_batch* cb, uint64_t* counts_out, uint64_t* total_out)
{
    am_batch* b = const_cast<am_batch*>(cb);
    Plan p; AM_TRY(make_plan(a, case_mode, b, p, true));
    if (total_out) *total_out = 0;
    if (counts_out && b->n_hay) std::memset(counts_out, 0, (size_t)b->n_hay * sizeof(uint64_t));
    if (p.nothing) return AM_OK;
    if (p.dense) return reduce_dense(a, case_mode, b, counts_out, total_out, nullptr);
    std::lock_guard<std::mutex> lk(b->mu);
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    AM_TRY(b->small.ensure(64));
    ScanOut o{};
    o.unit_chunks = p.unit_chunks;
    if (!p.use_sf) { AM_TRY(b->unit_counts.ensure((p.n_units + 1) * sizeof(uint32_t))); o.unit_counts = (uint32_t*)b->unit_counts.p; }
    o.total_values = (uint64_t*)b->small.p;
    if (counts_out) {
        AM_TRY(b->hay_counts.ensure((size_t)b->n_hay * sizeof(uint64_t)));
        o.hay_counts = (uint64_t*)b->hay_counts.p;
    }
    AM_TRY(build_hidx_and_clear(p, b, st, b->small.p, 64, counts_out ? b->hay_counts.p : nullptr, counts_out ? (size_t)b->n_hay * sizeof(uint64_t) : 0));
    if (p.use_sf) o.pool_ctrl = (uint32_t*)b->small.p + 4;          // ([2]: the role-specialised kernel's watchdog reports here)
    AM_TRY(launch_scan_kernel(p, kModeCount, o, st));
    uint64_t head[4] = {0, 0, 0, 0};                                // total_values, -, {pool counter, overflow}, {watchdog, -}
    ResultCopies rc;
    AM_TRY(rc.add(head, b->small.p, 32, st));
    if (counts_out) AM_TRY(rc.add(counts_out, b->hay_counts.p, (size_t)b->n_hay * sizeof(uint64_t), st));
    AM_TRY(rc.finish(st));
    if ((uint32_t)head[3] != 0) return fail(AM_ERR_HIP, kSfWatchdog);
    if (total_out) *total_out = head[0];
    return AM_OK;
}

// containsAny with the flags left in HBM: the sink decides what becomes of them (am_contains_any_batch: the copy to the caller; a select: the compaction)
int am::host::contains_any_flags(const am_automaton* a, int case_mode, am_batch* b, FlagSink& sink)
{
    Plan p; AM_TRY(make_plan(a, case_mode, b, p, true));
    AM_TRY(sink.begin(b));
    if (p.nothing) return sink.constant(0);
    if (p.dense) return reduce_dense(a, case_mode, b, nullptr, nullptr, &sink);
    std::lock_guard<std::mutex> lk(b->mu);
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    AM_TRY(b->flags.ensure(((size_t)b->n_hay + 3) & ~(size_t)3));
    AM_TRY(b->small.ensure(64));
    ScanOut o{};
    o.unit_chunks = p.unit_chunks;
    o.flags = (uint8_t*)b->flags.p;
    AM_TRY(build_hidx_and_clear(p, b, st, b->flags.p, ((size_t)b->n_hay + 3) & ~(size_t)3, b->small.p, 64));      // (the counter block: k_sf's unit ticket)
    AM_TRY(launch_scan_kernel(p, kModeAny, o, st));
    return sink.device((const uint8_t*)b->flags.p, st);
}

extern "C" int am_contains_any_batch(const am_automaton* a, int case_mode, const am_batch* cb, uint8_t* flags_out)
{
    HostFlagSink sink(flags_out, true);
    return contains_any_flags(a, case_mode, const_cast<am_batch*>(cb), sink);
}

int am::host::scan_needle_ids(const am_automaton* a, int case_mode, am_batch* b, const uint64_t* d_vals_off, const uint32_t* d_vals, uint32_t n_needles,
                              uint32_t* d_bits, uint32_t words, uint32_t* d_missing, FlagSink& sink, bool* taken)
{
    *taken = false;
    Plan p; AM_TRY(make_plan(a, case_mode, b, p));
    if (p.nothing || p.dense || !p.use_sf) return AM_OK;
    std::lock_guard<std::mutex> lk(b->mu);
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    AM_TRY(b->flags.ensure(((size_t)b->n_hay + 3) & ~(size_t)3));
    AM_TRY(b->small.ensure(64));
    ScanOut o{};
    o.unit_chunks = p.unit_chunks;
    o.flags = (uint8_t*)b->flags.p;
    o.ids_vals_off = d_vals_off; o.ids_vals = d_vals; o.ids_bits = d_bits; o.ids_missing = d_missing; o.ids_words = words; o.ids_n = n_needles;
    HIP_TRY(hipMemsetAsync(d_bits, 0, (size_t)b->n_hay * words * 4, st));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_missing, (int)n_needles, b->n_hay, st));
    AM_TRY(build_hidx_and_clear(p, b, st, b->flags.p, ((size_t)b->n_hay + 3) & ~(size_t)3, b->small.p, 64));      // (the counter block: k_sf's unit ticket)
    AM_TRY(launch_scan_kernel(p, kModeIds, o, st));
    AM_TRY(sink.device((const uint8_t*)b->flags.p, st));
    *taken = true;
    return AM_OK;
}

// The whole scan: leaves every record of the batch, sorted by (haystack, end_pos), in device memory
// obtained from `sink(total, &ptr)` (called once, only when total > 0); *n_out = number of records.
int am::host::run_records(const am_automaton* a, int case_mode, am_batch* b, const std::function<int(uint64_t, Record**)>& sink_final, uint64_t* n_out, bool have_lock)
{
    *n_out = 0;
    Plan p; AM_TRY(make_plan(a, case_mode, b, p, true, have_lock));
    if (p.nothing) return AM_OK;
    std::unique_lock<std::mutex> lk(b->mu, std::defer_lock);
    if (!have_lock) lk.lock();
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    // automata with the empty needle: k_sf's (sparse) records go to a buffer of the batch, the dense pass writes the result
    uint64_t n_sparse = 0;
    auto sink_sparse = [&](uint64_t n, Record** ptr) -> int { AM_TRY(b->sparse.ensure(n * sizeof(Record))); *ptr = (Record*)b->sparse.p; return AM_OK; };
    const std::function<int(uint64_t, Record**)>& sink = p.dense ? std::function<int(uint64_t, Record**)>(sink_sparse) : sink_final;
    uint64_t* n_scan = p.dense ? &n_sparse : n_out;
    ScanSpace sp; AM_TRY(scan_workspaces(b, p.n_units, &sp));
    const uint64_t n = sp.n; const size_t tmp_bytes = sp.tmp_bytes;
    Record* d_records = nullptr;
    // general kernel: count pass -> exclusive scan -> emit pass (unit = one lane's chunk)
    auto body_ac = [&]() -> int {
        ScanOut o{};
        o.unit_counts = (uint32_t*)b->unit_counts.p;
        o.total_values = (uint64_t*)b->small.p;
        HIP_TRY(hipMemsetAsync(b->small.p, 0, 64, st));
        HIP_TRY(hipMemsetAsync((uint32_t*)b->unit_counts.p + p.n_units, 0, sizeof(uint32_t), st));
        AM_TRY(build_hidx(p, b, st));
        AM_TRY(launch_scan_kernel(p, kModeCount, o, st));
        { Prof pr("scan", st); HIP_TRY(launch_scan(b->scan_tmp.p, tmp_bytes, (const uint32_t*)b->unit_counts.p, (uint64_t*)b->unit_offsets.p, n, st)); }
        uint64_t total = 0;
        HIP_TRY(hipMemcpyAsync(&total, (uint64_t*)b->unit_offsets.p + p.n_units, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *n_scan = total;
        if (total == 0) return AM_OK;
        AM_TRY(sink(total, &d_records));
        ScanOut w{};
        w.unit_offsets = (const uint64_t*)b->unit_offsets.p;
        w.records = d_records;
        AM_TRY(launch_scan_kernel(p, kModeEmit, w, st));
        HIP_TRY(hipStreamSynchronize(st));
        return AM_OK;
    };
    // table-walk kernel: ONE walk drops a token per match into the pool (superblocks per wavefront, any order) and counts per unit; scan(unit_counts) + k_dfa_place
    // put token (unit, seq) where its record belongs.  The pool is sized by a guess (a record per 6 haystack bytes: the density these automata are made for);
    // if it is exhausted the counts are still exact and the walk is repeated once with the pool they ask for.
    auto body_dfa = [&]() -> int {
        const uint32_t n_waves = p.dfa_shape.workgroups * 16u;
        const uint64_t sb_bytes = dfa_superblock_bytes();
        // (the guess stays below 32 GiB of pool; a batch that needs more finds out with exact counts in hand, and one that needs more than the device has left
        // takes the plain count -> scan -> emit protocol, which needs no pool)
        constexpr uint64_t kFirstPoolBytes = 16ull << 30;
        // (the sample walk of make_plan has counted the needle ends of this batch: a quarter above its estimate; a batch too small to have been asked: a record per 6 bytes)
        const uint64_t guess = b->route_image == p.f->generation && b->route_ends_per_kib ? (b->total >> 10) * b->route_ends_per_kib * 5u / 4u + 4096u : b->total / 6u;
        uint64_t want = dfa_token_superblocks(guess, n_waves, p.n_units);
        if (want * sb_bytes > kFirstPoolBytes) want = std::max<uint64_t>(kFirstPoolBytes / sb_bytes, (uint64_t)n_waves + 16);
        if (b->pool.cap / sb_bytes > want) want = b->pool.cap / sb_bytes;
        if (cfg::get(cfg::kSfPoolBlocks) > 0) want = (uint64_t)cfg::get(cfg::kSfPoolBlocks);       // tests: force the exhausted-pool path
        for (int attempt = 0; attempt < 3; attempt++) {
            if (want >= (1ull << 31)) return body_ac();
            if (want * sb_bytes > b->pool.cap) {
                size_t free_b = 0, total_b = 0;
                if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || want * sb_bytes + (want * sb_bytes) / 8 + (1ull << 30) > (uint64_t)free_b + b->pool.cap) return body_ac();
            }
            AM_TRY(b->pool.ensure(want * sb_bytes));
            AM_TRY(b->block_next.ensure(2 * want * sizeof(uint32_t)));
            ScanOut o{};
            o.unit_counts = (uint32_t*)b->unit_counts.p;
            o.pool = (Record*)b->pool.p;
            o.block_next = (uint32_t*)b->block_next.p;           // here: tokens in each superblock, then each superblock's first group
            o.pool_ctrl = (uint32_t*)b->small.p + 4;             // small: [4] superblocks drawn, [5] pool exhausted
            o.n_blocks = (uint32_t)want;
            HIP_TRY(hipMemsetAsync(b->small.p, 0, 64, st));
            HIP_TRY(hipMemsetAsync(b->block_next.p, 0, want * sizeof(uint32_t), st));
            HIP_TRY(hipMemsetAsync((uint32_t*)b->unit_counts.p + p.n_units, 0, sizeof(uint32_t), st));
            AM_TRY(build_hidx(p, b, st));
            { Prof pr("dfa", st); HIP_TRY(launch_dfa_tokens(p.dfa, p.bv, o, p.dfa_shape, st)); }
            { Prof pr("scan", st); HIP_TRY(launch_scan(b->scan_tmp.p, tmp_bytes, (const uint32_t*)b->unit_counts.p, (uint64_t*)b->unit_offsets.p, n, st)); }
            uint64_t total = 0; uint32_t ctrl[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(&total, (uint64_t*)b->unit_offsets.p + p.n_units, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(ctrl, o.pool_ctrl, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (ctrl[1]) { want = dfa_token_superblocks(total, n_waves, p.n_units); continue; }
            *n_scan = total;
            if (total == 0) return AM_OK;
            AM_TRY(sink(total, &d_records));
            { Prof pr("dfa_place", st); HIP_TRY(launch_dfa_place(p.dfa, p.bv, o, ctrl[0] < o.n_blocks ? ctrl[0] : o.n_blocks, (const uint64_t*)b->unit_offsets.p, p.dfa_shape, p.f->h.n_states, d_records, st)); }
            HIP_TRY(hipStreamSynchronize(st));
            return AM_OK;
        }
        return fail(AM_ERR_HIP, "token pool exhausted repeatedly (internal error)");
    };
    // suffix-filter kernel (SfEmit).  The pool size is a guess; if it overflows the kernel still counts, and the pass is repeated once with the exact number of blocks.
    auto body_sf = [&]() -> int {
        SfEmit e{p, st, sp};
        uint64_t want_blocks = sf_pool_blocks(p, SfPool::Guess);
        for (int attempt = 0; attempt < 4; attempt++) {
            AM_TRY(e.setup(want_blocks));
            AM_TRY(e.scan(false, false));
            uint64_t total = 0; uint32_t ctrl[4] = {0, 0, 0, 0};
            HIP_TRY(hipMemcpyAsync(&total, (uint64_t*)b->unit_offsets.p + p.n_units, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(ctrl, e.o.pool_ctrl, 16, hipMemcpyDeviceToHost, st));      // [0] blocks drawn, [1] overflow, [2] kernel watchdog
            HIP_TRY(hipStreamSynchronize(st));
            if (ctrl[2]) return fail(AM_ERR_HIP, kSfWatchdog);
            if (ctrl[1]) { want_blocks = sf_pool_blocks(p, SfPool::Exact, ctrl[0]); continue; }    // pool too small: ctrl[0] = blocks actually needed
            *n_scan = total;
            if (total == 0) return AM_OK;
            AM_TRY(sink(total, &d_records));
            AM_TRY(e.permute(d_records));
            HIP_TRY(hipStreamSynchronize(st));
            return AM_OK;
        }
        return fail(AM_ERR_HIP, "record pool overflowed repeatedly (internal error)");
    };
    if (!p.dense) return p.use_sf ? body_sf() : (p.use_dfa && dfa_tokens_ok(p.dfa)) ? body_dfa() : body_ac();
    if (p.f->h.sf_tiers != 0) AM_TRY(body_sf());
    else {                                                  // no needle end is reachable (e.g. upper-case needles under IgnoreCase): only the dense part
        HIP_TRY(hipMemsetAsync(b->unit_offsets.p, 0, n * sizeof(uint64_t), st));
        AM_TRY(build_hidx(p, b, st));
    }
    // dense pass: count per unit -> scan -> write (the unit boundaries and b->unit_offsets are those of the k_sf pass)
    AM_TRY(b->sparse.ensure(sizeof(Record)));
    AM_TRY(b->dense_counts.ensure(n * sizeof(uint32_t)));
    AM_TRY(b->dense_offsets.ensure(n * sizeof(uint64_t)));
    HIP_TRY(hipMemsetAsync((uint32_t*)b->dense_counts.p + p.n_units, 0, sizeof(uint32_t), st));
    { Prof pr("dense", st);
      HIP_TRY(launch_dense(p.ic, false, p.ac, p.bv, (const Record*)b->sparse.p, (const uint64_t*)b->unit_offsets.p, p.unit_chunks, p.n_units, (uint32_t*)b->dense_counts.p, nullptr, nullptr, st)); }
    { Prof pr("scan", st); HIP_TRY(launch_scan(b->scan_tmp.p, tmp_bytes, (const uint32_t*)b->dense_counts.p, (uint64_t*)b->dense_offsets.p, n, st)); }
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, (uint64_t*)b->dense_offsets.p + p.n_units, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_out = total;
    if (total == 0) return AM_OK;
    Record* d_out = nullptr;
    AM_TRY(sink_final(total, &d_out));
    { Prof pr("dense", st);
      HIP_TRY(launch_dense(p.ic, true, p.ac, p.bv, (const Record*)b->sparse.p, (const uint64_t*)b->unit_offsets.p, p.unit_chunks, p.n_units, nullptr, (const uint64_t*)b->dense_offsets.p, d_out, st)); }
    HIP_TRY(hipStreamSynchronize(st));
    return AM_OK;
}

// The suffix-filter scan of a (small) batch WITHOUT a host round trip: the record pool is sized for the worst case -- a record at
// every byte -- so the pass cannot overflow and needs no retry; the sorted records go to d_out (room for b->total records), their
// number stays on the device (*n_dev points at it).  Used between Replacer passes, where a sync per scan would cost more than
// the scan.
int am::host::run_records_async(const am_automaton* a, int case_mode, am_batch* b, Record* d_out, const uint64_t** n_dev, hipStream_t st)
{
    Plan p; AM_TRY(make_plan(a, case_mode, b, p));
    if (!p.use_sf || p.dense) return fail(AM_ERR_UNSUPPORTED, "internal: asynchronous scan needs the plain suffix-filter route");
    std::lock_guard<std::mutex> lk(b->mu);
    ScanSpace sp; AM_TRY(scan_workspaces(b, p.n_units, &sp));
    *n_dev = (const uint64_t*)b->unit_offsets.p + p.n_units;
    if (p.nothing) { HIP_TRY(hipMemsetAsync(b->unit_offsets.p, 0, sp.n * sizeof(uint64_t), st)); return AM_OK; }
    SfEmit e{p, st, sp};
    AM_TRY(e.setup(sf_pool_blocks(p, SfPool::WorstCase)));
    AM_TRY(e.scan(true, true));                              // (the Replacer's window batches are new every pass: the clears and the index in one launch)
    return e.permute(d_out);
}

// Small batches (the one-document call): the whole chain -- clears + haystack index, scan, unit offsets, k_permute into a record array of
// the worst-case size (a record per byte) -- and the copies of the count and of the first records are enqueued at once, so the call has
// ONE stream synchronisation.  (The general path needs the count on the host before it sizes the record array: two, and a third when the
// caller reads the records.)  *done = false: not taken, or the record pool overflowed -- the general path runs.
constexpr uint64_t kSmallRunBytes = 64u << 10;
constexpr uint64_t kSmallRunEager = 256;                  // records that travel with the count (2048 of them: 10 us slower on a 10-KB document with 1 187 matches than a second copy)
static int run_records_small(const am_automaton* a, int case_mode, am_batch* b, am_matches* m, bool* done)
{
    *done = false;
    if (b->total == 0 || b->total > kSmallRunBytes || a->kernel_pref == 3) return AM_OK;
    Plan p; AM_TRY(make_plan(a, case_mode, b, p));
    if (p.nothing || p.dense || !p.use_sf || cfg::get(cfg::kSfPoolBlocks) > 0) return AM_OK;       // (AM_SF_POOL_BLOCKS, tests of the overflow / retry path: the general path has it)
    std::lock_guard<std::mutex> lk(b->mu);
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    ScanSpace sp; AM_TRY(scan_workspaces(b, p.n_units, &sp));
    SfEmit e{p, st, sp};
    AM_TRY(e.setup(sf_pool_blocks(p, SfPool::Guess)));
    void* d_records = nullptr; size_t cap_bytes = 0;
    AM_TRY(record_array_get(b->dev, (size_t)b->total * sizeof(Record), &d_records, &cap_bytes));
    auto body = [&]() -> int {
        AM_TRY(e.scan(true, false));
        AM_TRY(e.permute((Record*)d_records));
        uint64_t total = 0; uint32_t ctrl[2] = {0, 0};
        const uint64_t eager = b->total < kSmallRunEager ? b->total : kSmallRunEager;
        m->host.resize(eager);
        ResultCopies rc;
        AM_TRY(rc.add(&total, (uint64_t*)b->unit_offsets.p + p.n_units, 8, st));
        AM_TRY(rc.add(ctrl, e.o.pool_ctrl, 8, st));
        AM_TRY(rc.add(m->host.data(), d_records, eager * sizeof(Record), st));
        AM_TRY(rc.finish(st));
        if (ctrl[1]) return AM_OK;                            // record pool too small (cannot happen with this guess on <= 64 KiB, but the general path knows what to do)
        m->n = total;
        if (total <= eager) { m->host.resize(total); m->fetched = true; }
        else { m->host.clear(); m->fetched = false; }
        *done = true;
        return AM_OK;
    };
    const int rc = body();
    if (rc == AM_OK && *done && m->n) { m->d_records = (Record*)d_records; m->cap_bytes = cap_bytes; }
    else record_array_put(b->dev, d_records, cap_bytes);
    return rc;
}

int am::host::run_batch_impl(const am_automaton* a, int case_mode, const am_batch* cb, am_matches** out, bool allow_small)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!cb) return fail(AM_ERR_INVALID, "null batch");
    am_matches* m = new am_matches();
    m->dev = cb->dev;
    if (allow_small) {
        bool done = false;
        const int rc = run_records_small(a, case_mode, const_cast<am_batch*>(cb), m, &done);
        if (rc != AM_OK) { am_matches_free(m); return rc; }
        if (done) { *out = m; return AM_OK; }
        m->host.clear(); m->fetched = false; m->n = 0;
    }
    auto sink = [&](uint64_t total, Record** ptr) -> int {
        void* r = nullptr;
        AM_TRY(record_array_get(m->dev, total * sizeof(Record), &r, &m->cap_bytes));
        *ptr = m->d_records = (Record*)r;
        return AM_OK;
    };
    const int rc = run_records(a, case_mode, const_cast<am_batch*>(cb), sink, &m->n);
    if (rc != AM_OK) { am_matches_free(m); return rc; }
    *out = m;
    return AM_OK;
}

extern "C" int am_run_batch(const am_automaton* a, int case_mode, const am_batch* cb, am_matches** out) { return run_batch_impl(a, case_mode, cb, out, true); }

// include/am_debug.h: libam_check.so hands over k_ac's launcher when it is loaded (tests and measurements only)
extern "C" int am_debug_set_general_kernel(void* launcher, uint32_t image_version)
{
    if (launcher && image_version != kImageVersion) return fail(AM_ERR_INVALID, "libam_check.so was built against another image version");
    g_ac_launcher.store(reinterpret_cast<AcLauncher>(launcher), std::memory_order_release);
    return AM_OK;
}
