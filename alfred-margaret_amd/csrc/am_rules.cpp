// am_rules.cpp -- rule sets on the device (include/am.h "rule sets"): many boolean rules over needle groups answered from ONE scan of a batch.  The scan is
// containsAll's: it leaves, per haystack, the set of slots that occurred as a bitmap row in HBM (slot_rows, am_contains_all.cpp) and writes no record where the
// ids-mode scan takes the call.  k_rules_eval (am_rules.hip) turns the rows into rule-major bitmaps, first-rule-wins labels and per-rule counts, all of which stay in
// HBM until asked for; am_select_rule (am_select.cpp) hands one rule's haystacks to the select's compaction.
// The slot rows are bounded workspace: a batch whose rows exceed the budget (1 GiB; AM_RULES_ROWS_MIB) goes through in groups of whole consecutive haystacks, every
// group a multiple of 64 haystacks -- no word of `fired` belongs to two groups -- and a sub-batch made the way fold_batch makes one.  A group's rows are evaluated into
// its words of `fired` and its labels before the next group is scanned; the counts accumulate.  What crosses to the host during an am_rules_eval_batch: what the scans
// read back themselves, and -- only where there are groups -- one offset of the batch per group.
// Every argument is checked before any device work.
#include "am_host.h"
#include "am_rules.h"

using namespace am;
using namespace am::dev;
using namespace am::host;

// the program in HBM beside the slot table it speaks about.  (Holds DevBufs: on the heap only.)
struct am_rules {
    const am_needle_ids* slots = nullptr;                   // must outlive the rules
    int dev = 0;
    uint32_t n_rules = 0, n_slots = 0;
    uint64_t n_clauses = 0, n_literals = 0;
    DevBuf rule_off, clause_off, literals;
    RulesView view() const
    {
        return RulesView{(const uint64_t*)rule_off.p, (const uint64_t*)clause_off.p, (const uint32_t*)literals.p, n_rules, n_slots, n_clauses, n_literals};
    }
};

namespace {

constexpr uint64_t kRowsBudget = 1ull << 30;                // bytes of slot rows in HBM at a time
constexpr uint64_t kGroupQuantum = 64;                      // haystacks per word of `fired`: a group is a multiple of it

uint64_t rows_budget() { const long v = cfg::get(cfg::kRulesRowsMiB); return v >= 0 ? (uint64_t)v << 20 : kRowsBudget; }

using HitsPtr = std::unique_ptr<am_rule_hits, void (*)(am_rule_hits*)>;

// n entries of `off` that start at 0 and never decrease; *last = off[n - 1 + 1]
int check_offsets(const uint64_t* off, uint64_t n, const char* name, uint64_t* last)
{
    if (!off) return fail(AM_ERR_INVALID, std::string(name) + " is null");
    if (off[0] != 0) return fail(AM_ERR_INVALID, std::string(name) + "[0] must be 0");
    for (uint64_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return fail(AM_ERR_INVALID, std::string(name) + " decreases");
    *last = off[n];
    return AM_OK;
}

// haystacks [h0, h0 + n) of the result from their slot rows
int eval_rows(const am_rules* r, const uint32_t* d_rows, uint32_t words, uint64_t h0, uint64_t n, am_rule_hits* x, hipStream_t st)
{
    RulesEvalIn in{};
    in.rows = d_rows; in.words = words; in.n_hay = n;
    in.p = r->view();
    in.fired = (uint64_t*)x->fired.p; in.hay_words = x->hay_words; in.word0 = h0 / kGroupQuantum;
    in.labels = (uint32_t*)x->labels.p + h0; in.counts = (uint64_t*)x->counts.p;
    Prof pr("rules_eval", st);
    HIP_TRY(launch_rules_eval(in, g_rt.dev[x->dev].n_cu, st));
    return AM_OK;
}

}  // namespace

extern "C" int am_rules_create(const am_needle_ids* slots, const uint64_t* rule_off, const uint64_t* clause_off, const uint32_t* literals, uint32_t n_rules, am_rules** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (n_rules == 0xFFFFFFFFu) return fail(AM_ERR_INVALID, "too many rules");
    uint64_t n_clauses = 0, n_literals = 0;
    AM_TRY(check_offsets(rule_off, n_rules, "rule_off", &n_clauses));          // (rule_off[n_rules] IS the clause count: clause_off has that many entries + 1)
    AM_TRY(check_offsets(clause_off, n_clauses, "clause_off", &n_literals));
    if (n_literals && !literals) return fail(AM_ERR_INVALID, "literals is null");
    if (!slots) return fail(AM_ERR_INVALID, "null slot table");                 // (last of the checks a caller without a device can see: the table is looked at from here on)
    for (uint64_t i = 0; i < n_literals; i++)
        if ((literals[i] & ~kRuleNegate) >= slots->n_needles) return fail(AM_ERR_INVALID, "a literal names a slot >= n_slots");
    AM_TRY(ensure_runtime());
    const int dev = slots->a->dev;
    ON_DEVICE(dev);
    std::unique_ptr<am_rules> r(new am_rules());
    r->slots = slots; r->dev = dev; r->n_rules = n_rules; r->n_slots = slots->n_needles; r->n_clauses = n_clauses; r->n_literals = n_literals;
    AM_TRY(r->rule_off.ensure(((size_t)n_rules + 1) * 8));
    AM_TRY(r->clause_off.ensure((n_clauses + 1) * 8));
    AM_TRY(r->literals.ensure(n_literals * 4 + 4));
    HIP_TRY(hipMemcpy(r->rule_off.p, rule_off, ((size_t)n_rules + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r->clause_off.p, clause_off, (n_clauses + 1) * 8, hipMemcpyHostToDevice));
    if (n_literals) HIP_TRY(hipMemcpy(r->literals.p, literals, n_literals * 4, hipMemcpyHostToDevice));
    *out = r.release();
    return AM_OK;
}

extern "C" void am_rules_destroy(am_rules* r)
{
    if (!r) return;
    OnDevice od(r->dev);
    delete r;
}

extern "C" int am_rules_eval_batch(const am_rules* r, int case_mode, const am_batch* cb, am_rule_hits** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_case(case_mode));
    if (!r || !cb) return fail(AM_ERR_INVALID, "null rules or batch");
    if (r->dev != cb->dev) return fail(AM_ERR_INVALID, "rules and batch live on different devices");
    AM_TRY(ensure_runtime());
    am_batch* b = const_cast<am_batch*>(cb);
    ON_DEVICE(b->dev);
    hipStream_t st; AM_TRY(get_stream(b->dev, &st));
    const uint64_t n_hay = b->n_hay;
    HitsPtr x(new am_rule_hits(), am_rule_hits_free);
    x->dev = b->dev; x->n_hay = n_hay; x->src_total = b->total; x->n_rules = r->n_rules; x->hay_words = (n_hay + kGroupQuantum - 1) / kGroupQuantum;
    AM_TRY(x->fired.ensure(x->n_rules * x->hay_words * 8));
    AM_TRY(x->labels.ensure(n_hay * 4));
    AM_TRY(x->counts.ensure(x->n_rules * 8));
    if (x->n_rules) HIP_TRY(hipMemsetAsync(x->counts.p, 0, x->n_rules * 8, st));
    if (n_hay != 0) {
        const uint32_t words = (r->n_slots + 31) / 32;
        const uint64_t row_bytes = (uint64_t)words * 4;
        // haystacks per group: as many rows as the budget holds, in whole words of `fired`
        uint64_t group = row_bytes ? std::max<uint64_t>(rows_budget() / row_bytes / kGroupQuantum, 1) * kGroupQuantum : n_hay;
        if (group > n_hay) group = n_hay;
        DevBuf rows, missing;
        AM_TRY(rows.ensure(group * row_bytes + 64));
        AM_TRY(missing.ensure(group * 4 + 64));
        if (group == n_hay) {
            AM_TRY(slot_rows(r->slots, case_mode, b, (uint32_t*)rows.p, words, (uint32_t*)missing.p));
            AM_TRY(eval_rows(r, (const uint32_t*)rows.p, words, 0, n_hay, x.get(), st));
        } else {
            // groups of whole consecutive haystacks, each a batch of its own (sub_batch, am_fold.h: fold_batch's); one offset per group crosses to the host
            uint64_t o0 = 0, o1 = 0;
            AM_TRY(read_u64(b->d_offsets, &o0, st));
            DerivedBatch sub;                               // ONE batch: its buffers serve group after group
            sub.begin(b->dev);
            for (uint64_t h0 = 0; h0 < n_hay; h0 += group, o0 = o1) {
                const uint64_t h1 = std::min(n_hay, h0 + group);
                AM_TRY(read_u64(b->d_offsets + h1, &o1, st));      // (waits for the stream: the last group's evaluation has finished with the rows as well)
                if (o1 < o0 || o1 > b->total) return fail(AM_ERR_INVALID, "am_rules_eval_batch: the batch's offsets decrease or leave its text");
                AM_TRY(sub_batch(b, h0, h1, o0, o1, sub, st));
                AM_TRY(slot_rows(r->slots, case_mode, sub.b.get(), (uint32_t*)rows.p, words, (uint32_t*)missing.p));
                AM_TRY(eval_rows(r, (const uint32_t*)rows.p, words, h0, h1 - h0, x.get(), st));
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(st));                      // (the workspaces are freed; a result may be used from any thread and stream afterwards)
    *out = x.release();
    return AM_OK;
}

extern "C" int am_rules_eval(const am_rules* r, int case_mode, const am_slice* hay, size_t n_hay, am_rule_hits** out)
{
    if (!out) return fail(AM_ERR_INVALID, "out is null");
    *out = nullptr;
    AM_TRY(check_slices(hay, n_hay));
    AM_TRY(check_case(case_mode));
    if (!r) return fail(AM_ERR_INVALID, "null rules");           // (last: a caller without a device can see every other check)
    AM_TRY(ensure_runtime());
    return with_oneshot_batch(r->dev, hay, n_hay, [&](am_batch* b) { return am_rules_eval_batch(r, case_mode, b, out); });
}

extern "C" uint64_t am_rule_hits_haystacks(const am_rule_hits* x) { return x ? x->n_hay : 0; }
extern "C" uint64_t am_rule_hits_rules(const am_rule_hits* x) { return x ? x->n_rules : 0; }
extern "C" uint64_t am_rule_hits_hay_words(const am_rule_hits* x) { return x ? x->hay_words : 0; }
extern "C" const void* am_rule_hits_device_fired(const am_rule_hits* x) { return x && x->n_rules * x->hay_words ? x->fired.p : nullptr; }
extern "C" const void* am_rule_hits_device_labels(const am_rule_hits* x) { return x && x->n_hay ? x->labels.p : nullptr; }
extern "C" const void* am_rule_hits_device_counts(const am_rule_hits* x) { return x && x->n_rules ? x->counts.p : nullptr; }

extern "C" const uint64_t* am_rule_hits_fired(am_rule_hits* x)
{
    if (!x) { fail(AM_ERR_INVALID, "null rule hits"); return nullptr; }
    return fetch_once(x->h_fired, x->fired_fetched, x->dev, x->fired, x->n_rules * x->hay_words, "the fired bitmaps");
}

extern "C" const uint32_t* am_rule_hits_labels(am_rule_hits* x)
{
    if (!x) { fail(AM_ERR_INVALID, "null rule hits"); return nullptr; }
    return fetch_once(x->h_labels, x->labels_fetched, x->dev, x->labels, x->n_hay, "the labels");
}

extern "C" const uint64_t* am_rule_hits_counts(am_rule_hits* x)
{
    if (!x) { fail(AM_ERR_INVALID, "null rule hits"); return nullptr; }
    return fetch_once(x->h_counts, x->counts_fetched, x->dev, x->counts, x->n_rules, "the rule counts");
}

extern "C" void am_rule_hits_free(am_rule_hits* x)
{
    if (!x) return;
    OnDevice od(x->dev);
    delete x;
}

extern "C" void am_rules_geometry(uint32_t* tile_haystacks, uint32_t* lds_slot_words, uint32_t* lds_rules) { rules_geometry(tile_haystacks, lds_slot_words, lds_rules); }
