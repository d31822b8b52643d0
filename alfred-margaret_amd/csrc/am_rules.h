// am_rules.h -- the evaluator of rule sets (include/am.h "rule sets"): ONE function for the device and the host.  A program is in conjunctive normal form over slot
// literals: rule r = the AND of clauses [rule_off[r], rule_off[r + 1]), clause c = the OR of literals [clause_off[c], clause_off[c + 1]), a literal = a slot number in
// bits 0..30 and "negated" in bit 31; a literal is true iff (the slot's bit is set in the haystack's slot row) != negated.  An empty clause is false, a rule without a
// clause is true.
//
// rule_fires evaluates one rule over one row.  The row arrives as word(w) -- word w of the haystack's slot row, wherever the caller keeps it (k_rules_eval: a
// transposed tile in LDS or the row in HBM; the host: an array) -- and the two early exits ask any(x): "is x true for one of the haystacks that are evaluated in
// lockstep with this one?".  k_rules_eval answers with the wavefront's ballot, so the loops stay wave-uniform (the program is read through scalar indices); a
// sequential caller answers with x itself.  Plain C++: tests/native/rules_eval_main.cpp compiles it with g++ and holds it to a three-loop evaluator under a sanitizer.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AM_RULES_HD __host__ __device__ __forceinline__
#else
#define AM_RULES_HD inline
#endif
#ifndef AM_BOUNDS                                           // (a kernel's translation unit brings am_bounds.h; everywhere else an index out of range is an assert)
#include <cassert>
#define AM_BOUNDS(cond) assert(cond)
#endif

namespace am {
namespace dev {

constexpr uint32_t kRuleNegate = 0x80000000u;               // AM_RULE_NEGATE
constexpr uint32_t kRuleNone = 0xFFFFFFFFu;                 // the label of a haystack on which no rule fires

// the program as the kernels and the host read it: three arrays and their sizes (n_clauses = rule_off[n_rules], n_literals = clause_off[n_clauses])
struct RulesView {
    const uint64_t* rule_off; const uint64_t* clause_off; const uint32_t* literals;
    uint32_t n_rules, n_slots; uint64_t n_clauses, n_literals;
};

// what k_rules_eval is launched with (launch_rules_eval, am_device.h): the slot rows of n_hay consecutive haystacks -- a whole batch, or one group of it that begins at
// haystack 64 * word0 of the batch -- and where their results go.  n_tiles and lds_rules are the launcher's.
struct RulesEvalIn {
    const uint32_t* rows; uint32_t words; uint64_t n_hay;   // n_hay x words, haystack-major; words = ceil(n_slots / 32)
    RulesView p;
    uint64_t* fired; uint64_t hay_words, word0;             // the whole result's rows; this call writes words [word0, word0 + ceil(n_hay / 64)) of each
    uint32_t* labels; uint64_t* counts;                     // labels: of THESE haystacks (n_hay entries); counts: n_rules, accumulating
    uint64_t n_tiles; uint32_t lds_rules;
};

// does rule r fire on the haystack whose slot row is word(0 .. ceil(n_slots / 32))?  active: this caller has a haystack at all (a lane beyond the batch: false, and
// false comes back)
template <class Word, class Any>
AM_RULES_HD bool rule_fires(const RulesView& p, uint32_t r, bool active, Word&& word, Any&& any)
{
    AM_BOUNDS(r < p.n_rules);
    const uint64_t c0 = p.rule_off[r], c1 = p.rule_off[r + 1];
    AM_BOUNDS(c0 <= c1 && c1 <= p.n_clauses);
    bool alive = active;
    for (uint64_t c = c0; c < c1 && any(alive); c++) {      // (a rule may stop once nobody is still true)
        const uint64_t l0 = p.clause_off[c], l1 = p.clause_off[c + 1];
        AM_BOUNDS(l0 <= l1 && l1 <= p.n_literals);
        bool sat = false;
        for (uint64_t l = l0; l < l1 && any(alive && !sat); l++) {      // (a clause may stop once everybody who is still true is satisfied)
            const uint32_t lit = p.literals[l];
            const uint32_t slot = lit & ~kRuleNegate;
            AM_BOUNDS(slot < p.n_slots);
            const bool present = ((word(slot >> 5) >> (slot & 31u)) & 1u) != 0;
            sat = sat || (present != ((lit & kRuleNegate) != 0));
        }
        alive = alive && sat;
    }
    return alive;
}

}  // namespace dev
}  // namespace am
