// rules.hpp -- host mirror of am_rules_eval (include/am.h "rule sets"): the sequential definition.  The fold steps `Match _ v` of runWithCase (reference:
// src/Data/Text/AhoCorasick/Automaton.hs:442-553) over a haystack give the set P(h) of the slots v < nSlots it meets -- the complement of containsAll's final IntSet
// (src/Data/Text/AhoCorasick/Searcher.hs:173-187) -- and a program in conjunctive normal form over slot literals is evaluated on it, three loops deep: a rule is the
// AND of its clauses (no clause: true), a clause the OR of its literals (no literal: false), a literal (slot in P(h)) != negated.  rulesFold takes the fold steps as
// they are and touches no device.
#pragma once
#include <vector>

#include "spans.hpp"

namespace alfred_margaret {

struct RuleProgram {
    std::vector<uint64_t> ruleOff, clauseOff;               // nRules + 1, nClauses + 1
    std::vector<uint32_t> literals;                         // bits 0..30 the slot, bit 31 (AM_RULE_NEGATE): negated
    size_t numRules() const { return ruleOff.empty() ? 0 : ruleOff.size() - 1; }
};

struct RuleHits {
    uint64_t hayWords = 0;
    std::vector<uint64_t> fired;                            // [nRules][hayWords], bit h % 64 of word h / 64; bits beyond nHay are zero
    std::vector<uint32_t> labels;                           // nHay: the smallest rule that fires, 0xFFFFFFFF when none does
    std::vector<uint64_t> counts;                           // nRules
};

inline void checkProgram(const RuleProgram& p, size_t nSlots)
{
    if (p.ruleOff.empty() || p.ruleOff[0] != 0 || p.clauseOff.empty() || p.clauseOff[0] != 0) throw AmError(AM_ERR_INVALID, "rulesFold: offsets must start at 0");
    for (size_t i = 0; i + 1 < p.ruleOff.size(); i++) if (p.ruleOff[i + 1] < p.ruleOff[i]) throw AmError(AM_ERR_INVALID, "rulesFold: rule_off decreases");
    if (p.ruleOff.back() + 1 != p.clauseOff.size()) throw AmError(AM_ERR_INVALID, "rulesFold: rule_off[n_rules] is not the number of clauses");
    for (size_t i = 0; i + 1 < p.clauseOff.size(); i++) if (p.clauseOff[i + 1] < p.clauseOff[i]) throw AmError(AM_ERR_INVALID, "rulesFold: clause_off decreases");
    if (p.clauseOff.back() != p.literals.size()) throw AmError(AM_ERR_INVALID, "rulesFold: clause_off[n_clauses] is not the number of literals");
    for (uint32_t lit : p.literals) if ((lit & ~AM_RULE_NEGATE) >= nSlots) throw AmError(AM_ERR_INVALID, "rulesFold: a literal names a slot >= n_slots");
}

inline RuleHits rulesFold(const std::vector<FoldStep>& steps, size_t nHay, size_t nSlots, const RuleProgram& p)
{
    checkProgram(p, nSlots);
    const size_t nRules = p.numRules();
    RuleHits out;
    out.hayWords = (nHay + 63) / 64;
    out.fired.assign(nRules * out.hayWords, 0);
    out.labels.assign(nHay, 0xFFFFFFFFu);
    out.counts.assign(nRules, 0);
    std::vector<char> present(nSlots);
    size_t k = 0;
    for (size_t h = 0; h < nHay; h++) {
        std::fill(present.begin(), present.end(), 0);
        for (; k < steps.size() && steps[k].haystack == h; k++)
            if (steps[k].value < nSlots) present[steps[k].value] = 1;      // the am_needle_ids convention: values beyond the table are skipped
        for (size_t r = 0; r < nRules; r++) {
            bool rule = true;
            for (uint64_t c = p.ruleOff[r]; c < p.ruleOff[r + 1]; c++) {
                bool clause = false;
                for (uint64_t l = p.clauseOff[c]; l < p.clauseOff[c + 1]; l++) {
                    const uint32_t lit = p.literals[l];
                    if ((present[lit & ~AM_RULE_NEGATE] != 0) != ((lit & AM_RULE_NEGATE) != 0)) clause = true;
                }
                if (!clause) rule = false;
            }
            if (!rule) continue;
            out.fired[r * out.hayWords + h / 64] |= 1ull << (h % 64);
            out.counts[r]++;
            if (out.labels[h] == 0xFFFFFFFFu) out.labels[h] = (uint32_t)r;
        }
    }
    if (k != steps.size()) throw AmError(AM_ERR_INVALID, "rulesFold: the fold steps are not grouped by ascending haystack below n_hay");
    return out;
}

}  // namespace alfred_margaret
