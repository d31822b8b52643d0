// facade.cpp -- flat C entry points over the C++ host mirror (automaton.hpp / searcher.hpp /
// replacer.hpp) so that Python (ctypes) tests and bench.py can drive it.  Values are uint32 handles.
#include <cstring>
#include <memory>
#include <string>

#include "near.hpp"
#include "replacer.hpp"
#include "rules.hpp"
#include "spans.hpp"
#include "splitter.hpp"

using namespace alfred_margaret;

namespace {
thread_local std::string g_err;
struct MachineBox {
    AcMachine<uint32_t> m;
    std::vector<uint64_t> valuesOff; std::vector<uint32_t> valuesFlat;   // flattened machineValues for inspection
};
std::vector<Text> sliceTexts(const am_slice* hay, size_t n)
{
    std::vector<Text> t(n);
    for (size_t i = 0; i < n; i++) t[i] = Text(hay[i].ptr, hay[i].off, hay[i].len);
    return t;
}
template <class Fn> int guarded(Fn fn)
{
    try { fn(); return 0; }
    catch (const AmError& e) { g_err = e.what(); return e.code; }
    catch (const std::exception& e) { g_err = e.what(); return AM_ERR_INVALID; }
}
}  // namespace

extern "C" {

const char* amh_last_error(void) { return g_err.c_str(); }

// Automaton.build; values[i] (or i when values == NULL) is the payload handle of needle i
// (lower_from / lower_to / n_pairs: the caller's lower-case table, am_automaton_create_ex; null = built-in)
int amh_build_ex(const uint8_t* bytes, const uint64_t* offs, size_t n, const uint32_t* values, const uint32_t* lower_from, const uint32_t* lower_to,
                 size_t n_pairs, void** out)
{
    *out = nullptr;
    return guarded([&] {
        std::vector<std::pair<Text, uint32_t>> nv(n);
        for (size_t i = 0; i < n; i++) nv[i] = {Text(bytes, (size_t)offs[i], (size_t)(offs[i + 1] - offs[i])), values ? values[i] : (uint32_t)i};
        std::unique_ptr<utf8::LowerTable> lt;
        if (lower_from && lower_to) lt.reset(new utf8::LowerTable(lower_from, lower_to, n_pairs));
        auto* box = new MachineBox{build(nv, lt.get()), {}, {}};
        box->valuesOff.assign(1, 0);
        for (auto& vs : box->m.machineValues) { box->valuesFlat.insert(box->valuesFlat.end(), vs.begin(), vs.end()); box->valuesOff.push_back(box->valuesFlat.size()); }
        *out = box;
    });
}
int amh_build(const uint8_t* bytes, const uint64_t* offs, size_t n, const uint32_t* values, void** out)
{
    return amh_build_ex(bytes, offs, n, values, nullptr, nullptr, 0, out);
}
void amh_free(void* h) { delete static_cast<MachineBox*>(h); }
size_t amh_num_states(void* h) { return static_cast<MachineBox*>(h)->m.numStates(); }
size_t amh_num_transitions(void* h) { return static_cast<MachineBox*>(h)->m.machineTransitions.size(); }
const uint64_t* amh_transitions(void* h) { return static_cast<MachineBox*>(h)->m.machineTransitions.data(); }
const uint32_t* amh_offsets(void* h) { return static_cast<MachineBox*>(h)->m.machineOffsets.data(); }
const uint64_t* amh_root_ascii(void* h) { return static_cast<MachineBox*>(h)->m.machineRootAsciiTransitions.data(); }
const uint64_t* amh_values_off(void* h) { return static_cast<MachineBox*>(h)->valuesOff.data(); }
const uint32_t* amh_values(void* h) { return static_cast<MachineBox*>(h)->valuesFlat.data(); }
am_automaton* amh_device(void* h) { return static_cast<MachineBox*>(h)->m.device.get(); }

// runWithCase with a list-building fold over a batch: triples (haystack, matchPos, value) in fold
// order.  Call with cap = 0 to get the count.
int amh_run_list(void* h, int case_mode, const am_slice* hay, size_t n_hay, uint32_t* hay_out, uint64_t* pos_out, uint32_t* val_out,
                 uint64_t cap, uint64_t* n_out)
{
    return guarded([&] {
        struct Acc { std::vector<std::pair<uint64_t, uint32_t>> v; };
        auto f = [](Acc a, const Match<uint32_t>& m) { a.v.emplace_back(m.matchPos, m.matchValue); return Next<Acc>::Step(std::move(a)); };
        auto accs = runBatchWithCase((CaseSensitivity)case_mode, Acc{}, f, static_cast<MachineBox*>(h)->m, sliceTexts(hay, n_hay));
        uint64_t k = 0;
        for (size_t i = 0; i < accs.size(); i++)
            for (auto& pv : accs[i].v) { if (k < cap) { hay_out[k] = (uint32_t)i; pos_out[k] = pv.first; val_out[k] = pv.second; } k++; }
        *n_out = k;
    });
}

// countMatches (benchmark/haskell/app/Main.hs:67-76) per haystack
int amh_count(void* h, int case_mode, const am_slice* hay, size_t n_hay, uint64_t* counts_out)
{
    return guarded([&] { amCheck(am_count(static_cast<MachineBox*>(h)->m.device.get(), case_mode, hay, n_hay, counts_out)); });
}

// per-value match counts of a batch (countByNeedle): counts_out has n_values entries
int amh_count_by_needle(void* h, int case_mode, const am_slice* hay, size_t n_hay, size_t n_values, uint64_t* counts_out)
{
    return guarded([&] {
        auto r = countByNeedle((CaseSensitivity)case_mode, static_cast<MachineBox*>(h)->m, sliceTexts(hay, n_hay), n_values);
        for (size_t i = 0; i < r.size(); i++) counts_out[i] = r[i];
    });
}

// the term-document matrix of a batch (countMatrix): offsets (n_hay + 1) and 2 x n_entries words per entry as the C ABI lays them out (count; needle | haystack << 32);
// free both with amh_free_u64
int amh_count_matrix(void* h, int case_mode, const am_slice* hay, size_t n_hay, size_t n_values, uint64_t** offs_out, uint64_t** entries_out, uint64_t* n_entries_out)
{
    *offs_out = nullptr; *entries_out = nullptr; *n_entries_out = 0;
    return guarded([&] {
        const NeedleMatrix r = countMatrix((CaseSensitivity)case_mode, static_cast<MachineBox*>(h)->m, sliceTexts(hay, n_hay), n_values);
        const uint64_t ne = r.entries.size();
        uint64_t* offs = (uint64_t*)malloc((n_hay + 1) * sizeof(uint64_t));
        uint64_t* ents = (uint64_t*)malloc((ne ? ne : 1) * sizeof(am_needle_count));
        std::memcpy(offs, r.offsets.data(), (n_hay + 1) * sizeof(uint64_t));
        if (ne) std::memcpy(ents, r.entries.data(), ne * sizeof(am_needle_count));
        *offs_out = offs; *entries_out = ents; *n_entries_out = ne;
    });
}

// ---- match spans (spans.hpp)
namespace {
void spansOut(const Spans& r, size_t n_hay, uint64_t** offs_out, uint64_t** spans_out, uint64_t* n_out)
{
    const uint64_t ns = r.spans.size();
    uint64_t* offs = (uint64_t*)malloc((n_hay + 1) * sizeof(uint64_t));
    uint64_t* sp = (uint64_t*)malloc((ns ? ns : 1) * sizeof(am_span));
    std::memcpy(offs, r.offsets.data(), (n_hay + 1) * sizeof(uint64_t));
    if (ns) std::memcpy(sp, r.spans.data(), ns * sizeof(am_span));
    *offs_out = offs; *spans_out = sp; *n_out = ns;
}
}  // namespace
// spansFold over fold steps the caller brings (n triples in fold order, haystacks ascending): no device is touched.  offsets (n_hay + 1) and the spans as the C ABI
// lays them out (am_span, 24 bytes each); free both with amh_free_u64
// amh_spans_fold_words: the same with a word class (256 flags, nullable: none) -- only the whole-word spans are rows, filter before select
int amh_spans_fold_words(int case_mode, int mode, const uint32_t* hay_in, const uint64_t* pos_in, const uint32_t* val_in, uint64_t n, const am_slice* hay, size_t n_hay,
                         const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values, const uint8_t* word_bytes, uint64_t** offs_out, uint64_t** spans_out,
                         uint64_t* n_out)
{
    *offs_out = nullptr; *spans_out = nullptr; *n_out = 0;
    return guarded([&] {
        if ((case_mode != AM_CASE_SENSITIVE && case_mode != AM_IGNORE_CASE) || (mode != AM_SPANS_ALL && mode != AM_SPANS_LEFTMOST_LONGEST))
            throw AmError(AM_ERR_INVALID, "amh_spans_fold: bad case_mode or mode");
        std::vector<FoldStep> steps((size_t)n);
        for (uint64_t i = 0; i < n; i++) steps[i] = FoldStep{hay_in[i], pos_in[i], val_in[i]};
        const std::vector<uint32_t> lb(len_bytes, len_bytes + n_values), lc(len_code_points, len_code_points + n_values);
        spansOut(spansFold((CaseSensitivity)case_mode, mode == AM_SPANS_LEFTMOST_LONGEST, steps, sliceTexts(hay, n_hay), lb, lc, word_bytes), n_hay, offs_out, spans_out, n_out);
    });
}
int amh_spans_fold(int case_mode, int mode, const uint32_t* hay_in, const uint64_t* pos_in, const uint32_t* val_in, uint64_t n, const am_slice* hay, size_t n_hay,
                   const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values, uint64_t** offs_out, uint64_t** spans_out, uint64_t* n_out)
{
    return amh_spans_fold_words(case_mode, mode, hay_in, pos_in, val_in, n, hay, n_hay, len_bytes, len_code_points, n_values, nullptr, offs_out, spans_out, n_out);
}
// amh_run_list's fold (runWithCase with a list-building fold over the batch), then amh_spans_fold's
int amh_spans(void* h, int case_mode, int mode, const am_slice* hay, size_t n_hay, const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values,
              uint64_t** offs_out, uint64_t** spans_out, uint64_t* n_out)
{
    *offs_out = nullptr; *spans_out = nullptr; *n_out = 0;
    return guarded([&] {
        if ((case_mode != AM_CASE_SENSITIVE && case_mode != AM_IGNORE_CASE) || (mode != AM_SPANS_ALL && mode != AM_SPANS_LEFTMOST_LONGEST))
            throw AmError(AM_ERR_INVALID, "amh_spans: bad case_mode or mode");
        struct Acc { std::vector<std::pair<uint64_t, uint32_t>> v; };
        auto f = [](Acc a, const Match<uint32_t>& m) { a.v.emplace_back(m.matchPos, m.matchValue); return Next<Acc>::Step(std::move(a)); };
        const std::vector<Text> texts = sliceTexts(hay, n_hay);
        auto accs = runBatchWithCase((CaseSensitivity)case_mode, Acc{}, f, static_cast<MachineBox*>(h)->m, texts);
        std::vector<FoldStep> steps;
        for (size_t i = 0; i < accs.size(); i++)
            for (auto& pv : accs[i].v) steps.push_back(FoldStep{(uint32_t)i, pv.first, pv.second});
        const std::vector<uint32_t> lb(len_bytes, len_bytes + n_values), lc(len_code_points, len_code_points + n_values);
        spansOut(spansFold((CaseSensitivity)case_mode, mode == AM_SPANS_LEFTMOST_LONGEST, steps, texts, lb, lc), n_hay, offs_out, spans_out, n_out);
    });
}

// ---- exact case (include/am.h "exact case"): the siblings of amh_spans_fold_words / amh_spans / amh_substitute_fold_words that take the spellings as
// am_span_table_create_cased does -- exact_off: n_values + 1 offsets into exact_bytes, an empty range = no spelling, exact_off null = none at all; word_bytes nullable
namespace {
ExactSpellings spellingsOf(const uint64_t* exact_off, const uint8_t* exact_bytes, size_t n_values)
{
    ExactSpellings out(n_values);
    if (!exact_off) return out;
    if (exact_off[0] != 0) throw AmError(AM_ERR_INVALID, "exact_off[0] is not 0");
    for (size_t v = 0; v < n_values; v++) {
        if (exact_off[v + 1] < exact_off[v]) throw AmError(AM_ERR_INVALID, "exact_off descends");
        if (exact_off[v + 1] > exact_off[v]) out[v] = std::string(reinterpret_cast<const char*>(exact_bytes) + exact_off[v], (size_t)(exact_off[v + 1] - exact_off[v]));
    }
    return out;
}
}  // namespace
int amh_spans_fold_cased(int case_mode, int mode, const uint32_t* hay_in, const uint64_t* pos_in, const uint32_t* val_in, uint64_t n, const am_slice* hay, size_t n_hay,
                         const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values, const uint8_t* word_bytes, const uint64_t* exact_off,
                         const uint8_t* exact_bytes, uint64_t** offs_out, uint64_t** spans_out, uint64_t* n_out)
{
    *offs_out = nullptr; *spans_out = nullptr; *n_out = 0;
    return guarded([&] {
        if ((case_mode != AM_CASE_SENSITIVE && case_mode != AM_IGNORE_CASE) || (mode != AM_SPANS_ALL && mode != AM_SPANS_LEFTMOST_LONGEST))
            throw AmError(AM_ERR_INVALID, "amh_spans_fold_cased: bad case_mode or mode");
        std::vector<FoldStep> steps((size_t)n);
        for (uint64_t i = 0; i < n; i++) steps[i] = FoldStep{hay_in[i], pos_in[i], val_in[i]};
        const std::vector<uint32_t> lb(len_bytes, len_bytes + n_values), lc(len_code_points, len_code_points + n_values);
        const ExactSpellings exact = spellingsOf(exact_off, exact_bytes, n_values);
        spansOut(spansFold((CaseSensitivity)case_mode, mode == AM_SPANS_LEFTMOST_LONGEST, steps, sliceTexts(hay, n_hay), lb, lc, word_bytes, &exact), n_hay, offs_out, spans_out,
                 n_out);
    });
}
// amh_spans with a class and spellings: amh_run_list's fold, then amh_spans_fold_cased's
int amh_spans_cased(void* h, int case_mode, int mode, const am_slice* hay, size_t n_hay, const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values,
                    const uint8_t* word_bytes, const uint64_t* exact_off, const uint8_t* exact_bytes, uint64_t** offs_out, uint64_t** spans_out, uint64_t* n_out)
{
    *offs_out = nullptr; *spans_out = nullptr; *n_out = 0;
    return guarded([&] {
        if ((case_mode != AM_CASE_SENSITIVE && case_mode != AM_IGNORE_CASE) || (mode != AM_SPANS_ALL && mode != AM_SPANS_LEFTMOST_LONGEST))
            throw AmError(AM_ERR_INVALID, "amh_spans_cased: bad case_mode or mode");
        struct Acc { std::vector<std::pair<uint64_t, uint32_t>> v; };
        auto f = [](Acc a, const Match<uint32_t>& m) { a.v.emplace_back(m.matchPos, m.matchValue); return Next<Acc>::Step(std::move(a)); };
        const std::vector<Text> texts = sliceTexts(hay, n_hay);
        auto accs = runBatchWithCase((CaseSensitivity)case_mode, Acc{}, f, static_cast<MachineBox*>(h)->m, texts);
        std::vector<FoldStep> steps;
        for (size_t i = 0; i < accs.size(); i++)
            for (auto& pv : accs[i].v) steps.push_back(FoldStep{(uint32_t)i, pv.first, pv.second});
        const std::vector<uint32_t> lb(len_bytes, len_bytes + n_values), lc(len_code_points, len_code_points + n_values);
        const ExactSpellings exact = spellingsOf(exact_off, exact_bytes, n_values);
        spansOut(spansFold((CaseSensitivity)case_mode, mode == AM_SPANS_LEFTMOST_LONGEST, steps, texts, lb, lc, word_bytes, &exact), n_hay, offs_out, spans_out, n_out);
    });
}

// ---- rule sets (rules.hpp): rulesFold over fold steps the caller brings (n (haystack, value) pairs in fold order, haystacks ascending) and a program in the C ABI's
// form (rule_off: n_rules + 1, clause_off: rule_off[n_rules] + 1, literals: clause_off[last]): no device is touched.  fired_out: n_rules x ceil(n_hay / 64) words,
// labels_out: n_hay, counts_out: n_rules, all the caller's
int amh_rules_fold(const uint32_t* hay_in, const uint32_t* val_in, uint64_t n, size_t n_hay, size_t n_slots, const uint64_t* rule_off, const uint64_t* clause_off,
                   const uint32_t* literals, uint32_t n_rules, uint64_t* fired_out, uint32_t* labels_out, uint64_t* counts_out)
{
    return guarded([&] {
        if (!rule_off || !clause_off) throw AmError(AM_ERR_INVALID, "amh_rules_fold: null offsets");
        RuleProgram p;
        p.ruleOff.assign(rule_off, rule_off + (size_t)n_rules + 1);
        p.clauseOff.assign(clause_off, clause_off + (size_t)p.ruleOff.back() + 1);
        if (p.clauseOff.back()) p.literals.assign(literals, literals + (size_t)p.clauseOff.back());
        std::vector<FoldStep> steps((size_t)n);
        for (uint64_t i = 0; i < n; i++) steps[i] = FoldStep{hay_in[i], 0, val_in[i]};
        const RuleHits r = rulesFold(steps, n_hay, n_slots, p);
        if (!r.fired.empty()) std::memcpy(fired_out, r.fired.data(), r.fired.size() * 8);
        if (!r.labels.empty()) std::memcpy(labels_out, r.labels.data(), r.labels.size() * 4);
        if (!r.counts.empty()) std::memcpy(counts_out, r.counts.data(), r.counts.size() * 8);
    });
}

// ---- scores (automaton.hpp scoreByHaystack) over fold steps the caller brings (n (haystack, value) pairs in fold order): no device is touched.  weights: n_cols x
// n_values, scores_out: n_cols x n_hay, both column after column, the caller's
int amh_score(const uint32_t* hay_in, const uint32_t* val_in, uint64_t n, size_t n_hay, size_t n_values, const int64_t* weights, uint32_t n_cols, int64_t* scores_out)
{
    return guarded([&] {
        if (n && (!hay_in || !val_in)) throw AmError(AM_ERR_INVALID, "amh_score: null fold steps");
        if (n_values && !weights) throw AmError(AM_ERR_INVALID, "amh_score: null weights");
        const std::vector<int64_t> r = scoreByHaystack(hay_in, val_in, n, n_hay, n_values, weights, n_cols);
        if (!r.empty()) std::memcpy(scores_out, r.data(), r.size() * 8);
    });
}

// ---- proximity (near.hpp): nearFold over leftmost-longest spans the caller brings (CSR: span_offs has n_hay + 1 entries, spans_in span_offs[n_hay] rows of am_span), a
// group mask per needle handle and queries in the C ABI's form: no device is touched.  fired_out: n_queries x ceil(n_hay / 64) words, counts_out: n_queries, both the
// caller's; offsets (n_hay + 1) and the pairs as the C ABI lays them out (am_near_pair, 32 bytes each): free both with amh_free_u64
int amh_near_fold(const uint64_t* span_offs, const am_span* spans_in, size_t n_hay, const uint32_t* group_mask, size_t n_needles, const am_near_query* queries,
                  uint32_t n_queries, uint64_t** offs_out, uint64_t** pairs_out, uint64_t* n_out, uint64_t* fired_out, uint64_t* counts_out)
{
    *offs_out = nullptr; *pairs_out = nullptr; *n_out = 0;
    return guarded([&] {
        if (!span_offs || span_offs[0] != 0) throw AmError(AM_ERR_INVALID, "amh_near_fold: span_offs is null or does not begin with 0");
        if ((n_needles && !group_mask) || (n_queries && !queries)) throw AmError(AM_ERR_INVALID, "amh_near_fold: null group masks or queries");
        for (size_t h = 0; h < n_hay; h++)
            if (span_offs[h + 1] < span_offs[h]) throw AmError(AM_ERR_INVALID, "amh_near_fold: span_offs descends");
        Spans sp;
        sp.offsets.assign(span_offs, span_offs + n_hay + 1);
        if (span_offs[n_hay]) sp.spans.assign(spans_in, spans_in + span_offs[n_hay]);
        const NearHits r = nearFold(sp, std::vector<uint32_t>(group_mask, group_mask + n_needles), std::vector<am_near_query>(queries, queries + n_queries));
        const uint64_t np = r.pairs.size();
        uint64_t* offs = (uint64_t*)malloc((n_hay + 1) * sizeof(uint64_t));
        uint64_t* pr = (uint64_t*)malloc((np ? np : 1) * sizeof(am_near_pair));
        std::memcpy(offs, r.offsets.data(), (n_hay + 1) * sizeof(uint64_t));
        if (np) std::memcpy(pr, r.pairs.data(), np * sizeof(am_near_pair));
        if (!r.fired.empty()) std::memcpy(fired_out, r.fired.data(), r.fired.size() * 8);
        if (!r.counts.empty()) std::memcpy(counts_out, r.counts.data(), r.counts.size() * 8);
        *offs_out = offs; *pairs_out = pr; *n_out = np;
    });
}

// ---- extract (spans.hpp): extractFold over spans the caller brings (CSR: span_offs has n_hay + 1 entries, spans_in span_offs[n_hay] rows of am_span): no device is
// touched.  offsets (n_hay + 1) and the fragments as the C ABI lays them out (am_fragment, 16 bytes each); free both with amh_free_u64
int amh_extract_fold(const uint64_t* span_offs, const am_span* spans_in, const am_slice* hay, size_t n_hay, uint32_t before, uint32_t after, int merged,
                     uint64_t** offs_out, uint64_t** frags_out, uint64_t* n_out)
{
    *offs_out = nullptr; *frags_out = nullptr; *n_out = 0;
    return guarded([&] {
        if (merged != 0 && merged != 1) throw AmError(AM_ERR_INVALID, "amh_extract_fold: bad mode");
        if (!span_offs || span_offs[0] != 0) throw AmError(AM_ERR_INVALID, "amh_extract_fold: span_offs is null or does not begin with 0");
        for (size_t h = 0; h < n_hay; h++)
            if (span_offs[h + 1] < span_offs[h]) throw AmError(AM_ERR_INVALID, "amh_extract_fold: span_offs descends");
        Spans sp;
        sp.offsets.assign(span_offs, span_offs + n_hay + 1);
        if (span_offs[n_hay]) sp.spans.assign(spans_in, spans_in + span_offs[n_hay]);
        const Extracted r = extractFold(sp, sliceTexts(hay, n_hay), before, after, merged != 0);
        const uint64_t nf = r.fragments.size();
        uint64_t* offs = (uint64_t*)malloc((n_hay + 1) * sizeof(uint64_t));
        uint64_t* fr = (uint64_t*)malloc((nf ? nf : 1) * sizeof(am_fragment));
        std::memcpy(offs, r.offsets.data(), (n_hay + 1) * sizeof(uint64_t));
        if (nf) std::memcpy(fr, r.fragments.data(), nf * sizeof(am_fragment));
        *offs_out = offs; *frags_out = fr; *n_out = nf;
    });
}

// ---- substitute (spans.hpp): the leftmost-longest spans spliced with replacement v = repl_bytes[repl_off[v], repl_off[v + 1]); the texts come back as one malloc'd blob
// (amh_free_blob) + offsets (n_hay + 1, the caller's)
namespace {
void substituteOut(const Spans& sp, const std::vector<Text>& texts, const uint8_t* repl_bytes, const uint64_t* repl_off, size_t n_values, uint8_t** blob_out, uint64_t* offs_out)
{
    std::vector<std::string> repl(n_values);
    for (size_t v = 0; v < n_values; v++) if (repl_off[v + 1] > repl_off[v]) repl[v].assign((const char*)repl_bytes + repl_off[v], (size_t)(repl_off[v + 1] - repl_off[v]));
    const std::vector<std::string> res = substitute(sp, texts, repl);
    uint64_t total = 0;
    for (size_t i = 0; i < res.size(); i++) { offs_out[i] = total; total += res[i].size(); }
    offs_out[res.size()] = total;
    uint8_t* blob = (uint8_t*)malloc(total ? total : 1);
    for (size_t i = 0; i < res.size(); i++) if (!res[i].empty()) std::memcpy(blob + offs_out[i], res[i].data(), res[i].size());
    *blob_out = blob;
}
}  // namespace
// over fold steps the caller brings (as amh_spans_fold): no device is touched
// amh_substitute_fold_words: the same with a word class (256 flags, nullable: none)
int amh_substitute_fold_words(int case_mode, const uint32_t* hay_in, const uint64_t* pos_in, const uint32_t* val_in, uint64_t n, const am_slice* hay, size_t n_hay,
                              const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values, const uint8_t* repl_bytes, const uint64_t* repl_off,
                              const uint8_t* word_bytes, uint8_t** blob_out, uint64_t* offs_out)
{
    *blob_out = nullptr;
    return guarded([&] {
        if (case_mode != AM_CASE_SENSITIVE && case_mode != AM_IGNORE_CASE) throw AmError(AM_ERR_INVALID, "amh_substitute_fold: bad case_mode");
        std::vector<FoldStep> steps((size_t)n);
        for (uint64_t i = 0; i < n; i++) steps[i] = FoldStep{hay_in[i], pos_in[i], val_in[i]};
        const std::vector<uint32_t> lb(len_bytes, len_bytes + n_values), lc(len_code_points, len_code_points + n_values);
        const std::vector<Text> texts = sliceTexts(hay, n_hay);
        substituteOut(spansFold((CaseSensitivity)case_mode, true, steps, texts, lb, lc, word_bytes), texts, repl_bytes, repl_off, n_values, blob_out, offs_out);
    });
}
int amh_substitute_fold(int case_mode, const uint32_t* hay_in, const uint64_t* pos_in, const uint32_t* val_in, uint64_t n, const am_slice* hay, size_t n_hay,
                        const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values, const uint8_t* repl_bytes, const uint64_t* repl_off,
                        uint8_t** blob_out, uint64_t* offs_out)
{
    return amh_substitute_fold_words(case_mode, hay_in, pos_in, val_in, n, hay, n_hay, len_bytes, len_code_points, n_values, repl_bytes, repl_off, nullptr, blob_out, offs_out);
}
// amh_substitute_fold_words with spellings (as amh_spans_fold_cased takes them): substituteFold over the kept rows
int amh_substitute_fold_cased(int case_mode, const uint32_t* hay_in, const uint64_t* pos_in, const uint32_t* val_in, uint64_t n, const am_slice* hay, size_t n_hay,
                              const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values, const uint8_t* repl_bytes, const uint64_t* repl_off,
                              const uint8_t* word_bytes, const uint64_t* exact_off, const uint8_t* exact_bytes, uint8_t** blob_out, uint64_t* offs_out)
{
    *blob_out = nullptr;
    return guarded([&] {
        if (case_mode != AM_CASE_SENSITIVE && case_mode != AM_IGNORE_CASE) throw AmError(AM_ERR_INVALID, "amh_substitute_fold_cased: bad case_mode");
        std::vector<FoldStep> steps((size_t)n);
        for (uint64_t i = 0; i < n; i++) steps[i] = FoldStep{hay_in[i], pos_in[i], val_in[i]};
        const std::vector<uint32_t> lb(len_bytes, len_bytes + n_values), lc(len_code_points, len_code_points + n_values);
        const std::vector<Text> texts = sliceTexts(hay, n_hay);
        const ExactSpellings exact = spellingsOf(exact_off, exact_bytes, n_values);
        substituteOut(spansFold((CaseSensitivity)case_mode, true, steps, texts, lb, lc, word_bytes, &exact), texts, repl_bytes, repl_off, n_values, blob_out, offs_out);
    });
}
// amh_run_list's fold (the scan on the device, the fold on the host), then spansFold and substitute
int amh_substitute(void* h, int case_mode, const am_slice* hay, size_t n_hay, const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values,
                   const uint8_t* repl_bytes, const uint64_t* repl_off, uint8_t** blob_out, uint64_t* offs_out)
{
    *blob_out = nullptr;
    return guarded([&] {
        if (case_mode != AM_CASE_SENSITIVE && case_mode != AM_IGNORE_CASE) throw AmError(AM_ERR_INVALID, "amh_substitute: bad case_mode");
        struct Acc { std::vector<std::pair<uint64_t, uint32_t>> v; };
        auto f = [](Acc a, const Match<uint32_t>& m) { a.v.emplace_back(m.matchPos, m.matchValue); return Next<Acc>::Step(std::move(a)); };
        const std::vector<Text> texts = sliceTexts(hay, n_hay);
        auto accs = runBatchWithCase((CaseSensitivity)case_mode, Acc{}, f, static_cast<MachineBox*>(h)->m, texts);
        std::vector<FoldStep> steps;
        for (size_t i = 0; i < accs.size(); i++)
            for (auto& pv : accs[i].v) steps.push_back(FoldStep{(uint32_t)i, pv.first, pv.second});
        const std::vector<uint32_t> lb(len_bytes, len_bytes + n_values), lc(len_code_points, len_code_points + n_values);
        substituteOut(spansFold((CaseSensitivity)case_mode, true, steps, texts, lb, lc), texts, repl_bytes, repl_off, n_values, blob_out, offs_out);
    });
}

// ---- substitute templates (spans.hpp substituteTemplates): the arrays of am_subst_table_create_templates -- template of handle v = segments [seg_off[v],
// seg_off[v + 1]), segment s of kind seg_kind[s] with the literal lit_bytes[lit_off[s], lit_off[s + 1]) -- checked as the C ABI checks them
namespace {
void templatesOut(const Spans& sp, const std::vector<Text>& texts, size_t n_values, const uint64_t* seg_off, const uint8_t* seg_kind, const uint64_t* lit_off,
                  const uint8_t* lit_bytes, uint8_t** blob_out, uint64_t* offs_out)
{
    if (!seg_off || seg_off[0] != 0) throw AmError(AM_ERR_INVALID, "substitute templates: seg_off is null or does not begin with 0");
    std::vector<Template> tpl(n_values);
    for (size_t v = 0; v < n_values; v++) {
        if (seg_off[v + 1] < seg_off[v] || seg_off[v + 1] - seg_off[v] > AM_SUBST_MAX_SEGMENTS) throw AmError(AM_ERR_INVALID, "substitute templates: seg_off descends or a template has too many segments");
        for (uint64_t s = seg_off[v]; s < seg_off[v + 1]; s++) {
            if (!seg_kind || !lit_off || lit_off[s + 1] < lit_off[s]) throw AmError(AM_ERR_INVALID, "substitute templates: seg_kind or lit_off is null, or lit_off descends");
            const uint64_t len = lit_off[s + 1] - lit_off[s];
            if (seg_kind[s] == AM_SEG_MATCH && len == 0) { tpl[v].push_back(TemplateSegment{true, std::string()}); continue; }
            if (seg_kind[s] != AM_SEG_LITERAL || (len && !lit_bytes)) throw AmError(AM_ERR_INVALID, "substitute templates: an unknown kind, a MATCH segment with bytes or no lit_bytes");
            tpl[v].push_back(TemplateSegment{false, len ? std::string((const char*)lit_bytes + lit_off[s], (size_t)len) : std::string()});
        }
    }
    const std::vector<std::string> res = substituteTemplates(sp, texts, tpl);
    uint64_t total = 0;
    for (size_t i = 0; i < res.size(); i++) { offs_out[i] = total; total += res[i].size(); }
    offs_out[res.size()] = total;
    uint8_t* blob = (uint8_t*)malloc(total ? total : 1);
    for (size_t i = 0; i < res.size(); i++) if (!res[i].empty()) std::memcpy(blob + offs_out[i], res[i].data(), res[i].size());
    *blob_out = blob;
}
}  // namespace
// over fold steps the caller brings (as amh_substitute_fold_words; word_bytes nullable: no class): no device is touched
int amh_substitute_templates_fold(int case_mode, const uint32_t* hay_in, const uint64_t* pos_in, const uint32_t* val_in, uint64_t n, const am_slice* hay, size_t n_hay,
                                  const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values, const uint64_t* seg_off, const uint8_t* seg_kind,
                                  const uint64_t* lit_off, const uint8_t* lit_bytes, const uint8_t* word_bytes, uint8_t** blob_out, uint64_t* offs_out)
{
    *blob_out = nullptr;
    return guarded([&] {
        if (case_mode != AM_CASE_SENSITIVE && case_mode != AM_IGNORE_CASE) throw AmError(AM_ERR_INVALID, "amh_substitute_templates_fold: bad case_mode");
        std::vector<FoldStep> steps((size_t)n);
        for (uint64_t i = 0; i < n; i++) steps[i] = FoldStep{hay_in[i], pos_in[i], val_in[i]};
        const std::vector<uint32_t> lb(len_bytes, len_bytes + n_values), lc(len_code_points, len_code_points + n_values);
        const std::vector<Text> texts = sliceTexts(hay, n_hay);
        templatesOut(spansFold((CaseSensitivity)case_mode, true, steps, texts, lb, lc, word_bytes), texts, n_values, seg_off, seg_kind, lit_off, lit_bytes, blob_out, offs_out);
    });
}
// amh_run_list's fold (the scan on the device, the fold on the host), then spansFold and substituteTemplates
int amh_substitute_templates(void* h, int case_mode, const am_slice* hay, size_t n_hay, const uint32_t* len_bytes, const uint32_t* len_code_points, size_t n_values,
                             const uint64_t* seg_off, const uint8_t* seg_kind, const uint64_t* lit_off, const uint8_t* lit_bytes, uint8_t** blob_out, uint64_t* offs_out)
{
    *blob_out = nullptr;
    return guarded([&] {
        if (case_mode != AM_CASE_SENSITIVE && case_mode != AM_IGNORE_CASE) throw AmError(AM_ERR_INVALID, "amh_substitute_templates: bad case_mode");
        struct Acc { std::vector<std::pair<uint64_t, uint32_t>> v; };
        auto f = [](Acc a, const Match<uint32_t>& m) { a.v.emplace_back(m.matchPos, m.matchValue); return Next<Acc>::Step(std::move(a)); };
        const std::vector<Text> texts = sliceTexts(hay, n_hay);
        auto accs = runBatchWithCase((CaseSensitivity)case_mode, Acc{}, f, static_cast<MachineBox*>(h)->m, texts);
        std::vector<FoldStep> steps;
        for (size_t i = 0; i < accs.size(); i++)
            for (auto& pv : accs[i].v) steps.push_back(FoldStep{(uint32_t)i, pv.first, pv.second});
        const std::vector<uint32_t> lb(len_bytes, len_bytes + n_values), lc(len_code_points, len_code_points + n_values);
        templatesOut(spansFold((CaseSensitivity)case_mode, true, steps, texts, lb, lc), texts, n_values, seg_off, seg_kind, lit_off, lit_bytes, blob_out, offs_out);
    });
}

// ---- Searcher
int amh_searcher_build(int case_mode, const uint8_t* bytes, const uint64_t* offs, size_t n, void** out)
{
    *out = nullptr;
    return guarded([&] {
        std::vector<std::string> ns(n);
        for (size_t i = 0; i < n; i++) ns[i].assign((const char*)bytes + offs[i], (size_t)(offs[i + 1] - offs[i]));
        *out = new Searcher<int>(buildNeedleIdSearcher((CaseSensitivity)case_mode, ns));
    });
}
void amh_searcher_free(void* s) { delete static_cast<Searcher<int>*>(s); }
void amh_searcher_set_case(void* s, int case_mode) { static_cast<Searcher<int>*>(s)->setCaseSensitivity((CaseSensitivity)case_mode); }
int amh_searcher_contains_any(void* s, const am_slice* hay, size_t n_hay, uint8_t* out)
{
    return guarded([&] { auto r = containsAnyBatch(*static_cast<Searcher<int>*>(s), sliceTexts(hay, n_hay)); for (size_t i = 0; i < n_hay; i++) out[i] = r[i]; });
}
int amh_searcher_contains_all(void* s, const am_slice* hay, size_t n_hay, uint8_t* out)
{
    return guarded([&] { auto r = containsAllBatch(*static_cast<Searcher<int>*>(s), sliceTexts(hay, n_hay)); for (size_t i = 0; i < n_hay; i++) out[i] = r[i]; });
}

int amh_searcher_contains_all_host_fold(void* s, const am_slice* hay, size_t n_hay, uint8_t* out)
{
    return guarded([&] { auto r = containsAllBatchHostFold(*static_cast<Searcher<int>*>(s), sliceTexts(hay, n_hay)); for (size_t i = 0; i < n_hay; i++) out[i] = r[i]; });
}

// ---- Replacer
int amh_replacer_build_ex(int case_mode, const uint8_t* nbytes, const uint64_t* noffs, const uint8_t* rbytes, const uint64_t* roffs, size_t n,
                          const uint32_t* lower_from, const uint32_t* lower_to, size_t n_pairs, void** out)
{
    *out = nullptr;
    return guarded([&] {
        std::unique_ptr<utf8::LowerTable> lt;
        if (lower_from && lower_to) lt.reset(new utf8::LowerTable(lower_from, lower_to, n_pairs));
        std::vector<std::pair<std::string, std::string>> pairs(n);
        for (size_t i = 0; i < n; i++) {
            pairs[i].first.assign((const char*)nbytes + noffs[i], (size_t)(noffs[i + 1] - noffs[i]));
            pairs[i].second.assign((const char*)rbytes + roffs[i], (size_t)(roffs[i + 1] - roffs[i]));
        }
        *out = new Replacer((CaseSensitivity)case_mode, pairs, lt.get());
    });
}
int amh_replacer_build(int case_mode, const uint8_t* nbytes, const uint64_t* noffs, const uint8_t* rbytes, const uint64_t* roffs, size_t n, void** out)
{
    return amh_replacer_build_ex(case_mode, nbytes, noffs, rbytes, roffs, n, nullptr, nullptr, 0, out);
}
void amh_replacer_free(void* r) { delete static_cast<Replacer*>(r); }
// mapReplacement with the new replacements given as a list (needle i gets rbytes[roffs[i] .. roffs[i+1]))
int amh_replacer_with_replacements(void* r, const uint8_t* rbytes, const uint64_t* roffs, void** out)
{
    *out = nullptr;
    return guarded([&] {
        const Replacer* src = static_cast<Replacer*>(r);
        size_t i = 0;
        std::vector<std::string> fresh(src->searcher().numNeedles());
        for (auto& f : fresh) { f.assign((const char*)rbytes + roffs[i], (size_t)(roffs[i + 1] - roffs[i])); i++; }
        // mapReplacement sees the payloads in needle order for `needles`, and per state for the automaton: map by priority
        *out = new Replacer(src->mapReplacementIndexed([&](size_t needle, const std::string&) { return fresh[needle]; }));
    });
}
// Replacer.compose (Replacer.hs:120-133): *out = null (and AM_OK) when the case sensitivities differ (the reference's Nothing)
int amh_replacer_compose(void* r1, void* r2, void** out)
{
    *out = nullptr;
    return guarded([&] {
        std::optional<Replacer> c = Replacer::compose(*static_cast<Replacer*>(r1), *static_cast<Replacer*>(r2));
        if (c) *out = new Replacer(std::move(*c));
    });
}
int amh_replacer_set_case(void* r, int case_mode, void** out)
{
    *out = nullptr;
    return guarded([&] { *out = new Replacer(static_cast<Replacer*>(r)->setCaseSensitivity((CaseSensitivity)case_mode)); });
}
// Runs a batch; results are returned as one malloc'd blob + offsets (n+1); is_nothing[i] = 1 where the
// reference returns Nothing.  max_len < 0 = maxBound.
static int replacer_run_batch(void* r, bool host_splice, const am_slice* hay, size_t n_hay, long long max_len, uint8_t** blob_out, uint64_t* offs_out, uint8_t* is_nothing)
{
    *blob_out = nullptr;
    return guarded([&] {
        std::vector<std::string> in(n_hay);
        for (size_t i = 0; i < n_hay; i++) in[i].assign((const char*)hay[i].ptr + hay[i].off, hay[i].len);
        const size_t lim = max_len < 0 ? SIZE_MAX : (size_t)max_len;
        auto* rp = static_cast<Replacer*>(r);
        auto res = host_splice ? rp->runBatchWithLimitHostSplice(in, lim) : rp->runBatchWithLimit(in, lim);
        uint64_t total = 0;
        for (size_t i = 0; i < n_hay; i++) { offs_out[i] = total; is_nothing[i] = !res[i].has_value(); if (res[i]) total += res[i]->size(); }
        offs_out[n_hay] = total;
        uint8_t* blob = (uint8_t*)malloc(total ? total : 1);
        for (size_t i = 0; i < n_hay; i++) if (res[i] && !res[i]->empty()) std::memcpy(blob + offs_out[i], res[i]->data(), res[i]->size());
        *blob_out = blob;
    });
}
int amh_replacer_run_batch(void* r, const am_slice* hay, size_t n_hay, long long max_len, uint8_t** blob_out, uint64_t* offs_out, uint8_t* is_nothing)
{
    return replacer_run_batch(r, false, hay, n_hay, max_len, blob_out, offs_out, is_nothing);
}
// same function with only the scans on the GPU (cross-check of the device passes)
int amh_replacer_run_batch_host_splice(void* r, const am_slice* hay, size_t n_hay, long long max_len, uint8_t** blob_out, uint64_t* offs_out, uint8_t* is_nothing)
{
    return replacer_run_batch(r, true, hay, n_hay, max_len, blob_out, offs_out, is_nothing);
}
// the am_replacer* (flattened Searcher Payload in HBM) behind this Replacer, for callers that keep their batches on the device
int amh_replacer_device(void* r, const void** out)
{
    *out = nullptr;
    return guarded([&] { *out = static_cast<Replacer*>(r)->device(); });
}
void amh_replacer_last_stats(void* r, uint64_t* passes, uint64_t* scanned_bytes)
{
    const auto st = static_cast<Replacer*>(r)->lastStats();
    *passes = st.passes; *scanned_bytes = st.scannedBytes;
}
void amh_free_blob(uint8_t* p) { free(p); }

// ---- Splitter
int amh_splitter_build(const uint8_t* sep, size_t len, void** out)
{
    *out = nullptr;
    return guarded([&] { *out = new Splitter(std::string((const char*)sep, len)); });
}
void amh_splitter_free(void* s) { delete static_cast<Splitter*>(s); }
// fragments of all haystacks concatenated: blob + fragment offsets (n_frag + 1) + per-haystack fragment counts
int amh_splitter_split_batch(void* sp, int ignore_case, const am_slice* hay, size_t n_hay, uint8_t** blob_out, uint64_t** offs_out,
                             uint64_t* n_frag_out, uint32_t* frags_per_hay)
{
    *blob_out = nullptr; *offs_out = nullptr;
    return guarded([&] {
        std::vector<std::string> in(n_hay);
        for (size_t i = 0; i < n_hay; i++) in[i].assign((const char*)hay[i].ptr + hay[i].off, hay[i].len);
        auto res = static_cast<Splitter*>(sp)->splitBatch(in, ignore_case != 0);
        uint64_t nf = 0, total = 0;
        for (auto& r : res) { nf += r.size(); for (auto& f : r) total += f.size(); }
        uint8_t* blob = (uint8_t*)malloc(total ? total : 1);
        uint64_t* offs = (uint64_t*)malloc((nf + 1) * sizeof(uint64_t));
        uint64_t k = 0, at = 0;
        for (size_t i = 0; i < n_hay; i++) {
            frags_per_hay[i] = (uint32_t)res[i].size();
            for (auto& f : res[i]) { offs[k++] = at; if (!f.empty()) std::memcpy(blob + at, f.data(), f.size()); at += f.size(); }
        }
        offs[k] = at;
        *blob_out = blob; *offs_out = offs; *n_frag_out = nf;
    });
}
// the same lists with the fold on the device (Splitter::splitBatchDevice)
int amh_splitter_split_batch_device(void* sp, int ignore_case, const am_slice* hay, size_t n_hay, uint8_t** blob_out, uint64_t** offs_out,
                                    uint64_t* n_frag_out, uint32_t* frags_per_hay)
{
    *blob_out = nullptr; *offs_out = nullptr;
    return guarded([&] {
        const std::vector<Text> ts = sliceTexts(hay, n_hay);
        const Splitter::Fragments fr = static_cast<Splitter*>(sp)->splitBatchFragments(ts, ignore_case != 0);
        const uint64_t nf = fr.fragments.size();
        uint64_t total = 0;
        for (auto& f : fr.fragments) total += f.len;
        uint8_t* blob = (uint8_t*)malloc(total ? total : 1);
        uint64_t* offs = (uint64_t*)malloc((nf + 1) * sizeof(uint64_t));
        uint64_t at = 0;
        for (size_t i = 0; i < n_hay; i++) {
            frags_per_hay[i] = (uint32_t)(fr.offsets[i + 1] - fr.offsets[i]);
            for (uint64_t k = fr.offsets[i]; k < fr.offsets[i + 1]; k++) {
                offs[k] = at;
                if (fr.fragments[k].len) std::memcpy(blob + at, ts[i].begin() + fr.fragments[k].start, (size_t)fr.fragments[k].len);
                at += fr.fragments[k].len;
            }
        }
        offs[nf] = at;
        *blob_out = blob; *offs_out = offs; *n_frag_out = nf;
    });
}
// (start, length) per fragment: offsets (n_hay + 1) and 2 x n_frag words; free both with amh_free_u64
int amh_splitter_fragments_batch(void* sp, int ignore_case, const am_slice* hay, size_t n_hay, uint64_t** offs_out, uint64_t** frags_out, uint64_t* n_frag_out)
{
    *offs_out = nullptr; *frags_out = nullptr; *n_frag_out = 0;
    return guarded([&] {
        const Splitter::Fragments fr = static_cast<Splitter*>(sp)->splitBatchFragments(sliceTexts(hay, n_hay), ignore_case != 0);
        const uint64_t nf = fr.fragments.size();
        uint64_t* offs = (uint64_t*)malloc((n_hay + 1) * sizeof(uint64_t));
        uint64_t* frags = (uint64_t*)malloc((nf ? nf : 1) * 2 * sizeof(uint64_t));
        std::memcpy(offs, fr.offsets.data(), (n_hay + 1) * sizeof(uint64_t));
        for (uint64_t k = 0; k < nf; k++) { frags[2 * k] = fr.fragments[k].start; frags[2 * k + 1] = fr.fragments[k].len; }
        *offs_out = offs; *frags_out = frags; *n_frag_out = nf;
    });
}
// the am_splitter* behind this Splitter, for callers that keep their batches on the device
int amh_splitter_device(void* sp, const void** out)
{
    *out = nullptr;
    return guarded([&] { *out = static_cast<Splitter*>(sp)->device(); });
}
// the am_automaton* of the separator (tests choose the scan route on it)
int amh_splitter_automaton(void* sp, const void** out)
{
    *out = nullptr;
    return guarded([&] { *out = static_cast<Splitter*>(sp)->automaton().device.get(); });
}
void amh_free_u64(uint64_t* p) { free(p); }

// ---- Utf8 helpers
int64_t amh_skip_code_points_backwards(const uint8_t* d, size_t len, size_t index, size_t n)
{
    try { return (int64_t)utf8::skipCodePointsBackwards(Text(d, 0, len), index, n); } catch (...) { return -1; }
}
size_t amh_lower_utf8(const uint8_t* d, size_t len, uint8_t* out, size_t cap)
{
    std::string s = utf8::lowerUtf8(Text(d, 0, len));
    if (s.size() <= cap) std::memcpy(out, s.data(), s.size());
    return s.size();
}

// Utf8.isCaseInvariant (Utf8.hs:169-171): 1 / 0; -1 on error
int amh_is_case_invariant(const uint8_t* d, size_t len, const uint32_t* lower_from, const uint32_t* lower_to, size_t n_pairs)
{
    try {
        std::unique_ptr<utf8::LowerTable> lt;
        if (lower_from && lower_to) lt.reset(new utf8::LowerTable(lower_from, lower_to, n_pairs));
        return utf8::isCaseInvariant(Text(d, 0, len), lt.get()) ? 1 : 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// Automaton.needleCasings (Automaton.hs:555-566): the casings concatenated + their offsets (n + 1); free with amh_free_blob / amh_free_u64
int amh_needle_casings(const uint8_t* d, size_t len, const uint32_t* lower_from, const uint32_t* lower_to, size_t n_pairs, uint8_t** blob_out, uint64_t** offs_out, uint64_t* n_out)
{
    *blob_out = nullptr; *offs_out = nullptr; *n_out = 0;
    return guarded([&] {
        std::unique_ptr<utf8::LowerTable> lt;
        if (lower_from && lower_to) lt.reset(new utf8::LowerTable(lower_from, lower_to, n_pairs));
        const std::vector<std::string> cs = needleCasings(Text(d, 0, len), lt.get());
        uint64_t total = 0;
        for (auto& c : cs) total += c.size();
        uint8_t* blob = (uint8_t*)malloc(total ? total : 1);
        uint64_t* offs = (uint64_t*)malloc((cs.size() + 1) * sizeof(uint64_t));
        uint64_t at = 0;
        for (size_t i = 0; i < cs.size(); i++) { offs[i] = at; if (!cs[i].empty()) std::memcpy(blob + at, cs[i].data(), cs[i].size()); at += cs[i].size(); }
        offs[cs.size()] = at;
        *blob_out = blob; *offs_out = offs; *n_out = cs.size();
    });
}

}  // extern "C"
