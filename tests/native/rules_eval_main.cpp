// rules_eval_main.cpp -- a stand-alone program that runs the evaluator of csrc/am_rules.h (rule_fires: the __host__ __device__ function k_rules_eval calls once per
// rule) ON THE CPU and holds it to a naive three-loop evaluator on random programs, so that the evaluator is checked -- every index it forms included, under a
// sanitizer -- before it meets a GPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I alfred-margaret_amd/csrc tests/native/rules_eval_main.cpp \
//       -o rules_eval && ./rules_eval
// The three arrays of a program and the slot row are heap blocks of exactly their size: a read beyond one is a sanitizer report.  The evaluator runs in both of its
// roles: alone (any(x) = x, the sequential caller: every early exit is taken) and in lockstep with other haystacks, where any(x) -- the wavefront's ballot -- is true
// whenever x is and sometimes when it is not: the early exits must not change a lane's result.  Corner programs: no rules, empty rules, empty clauses, x AND NOT x,
// x OR NOT x, duplicate literals, one slot, slot counts around a word of the row and around the widest row k_rules_eval keeps in LDS.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "am_rules.h"

using namespace am::dev;

namespace {

int g_failed = 0;

struct Program {
    std::vector<uint64_t> rule_off{0}, clause_off{0};
    std::vector<uint32_t> literals;
    uint32_t n_slots = 0;
    void clause(const std::vector<uint32_t>& lits) { literals.insert(literals.end(), lits.begin(), lits.end()); clause_off.push_back(literals.size()); }
    void end_rule() { rule_off.push_back(clause_off.size() - 1); }
    uint32_t n_rules() const { return (uint32_t)rule_off.size() - 1; }
};

// exact-size heap copies: what the sanitizer watches
template <class T>
struct Block {
    T* p; size_t n;
    explicit Block(const std::vector<T>& v) : p(static_cast<T*>(std::malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0)))), n(v.size())
    {
        for (size_t i = 0; i < n; i++) p[i] = v[i];
    }
    ~Block() { std::free(p); }
};

// the definition: three loops, no early exit
bool naive(const Program& p, uint32_t r, const std::vector<uint32_t>& row)
{
    bool rule = true;
    for (uint64_t c = p.rule_off[r]; c < p.rule_off[r + 1]; c++) {
        bool clause = false;
        for (uint64_t l = p.clause_off[c]; l < p.clause_off[c + 1]; l++) {
            const uint32_t slot = p.literals[l] & 0x7FFFFFFFu;
            const bool present = (row[slot / 32] >> (slot % 32)) & 1u;
            if (present != ((p.literals[l] >> 31) != 0)) clause = true;
        }
        if (!clause) rule = false;
    }
    return rule;
}

void check(const Program& p, std::mt19937& rng, const char* what)
{
    const uint32_t words = (p.n_slots + 31) / 32;
    Block<uint64_t> ro(p.rule_off), co(p.clause_off);
    Block<uint32_t> li(p.literals);
    const RulesView v{ro.p, co.p, li.p, p.n_rules(), p.n_slots, p.clause_off.size() - 1, p.literals.size()};
    constexpr int kLanes = 64;
    std::vector<std::vector<uint32_t>> rows(kLanes, std::vector<uint32_t>(words));
    for (int round = 0; round < 8; round++) {
        const int active = round == 0 ? kLanes : 1 + (int)(rng() % kLanes);       // (a tail wavefront: the lanes beyond `active` have no haystack)
        const uint32_t density = rng() % 5;
        for (auto& row : rows)
            for (auto& w : row) w = density == 0 ? 0u : density == 4 ? ~0u : (uint32_t)rng() & (density == 1 ? (uint32_t)rng() : ~0u);
        std::vector<Block<uint32_t>*> blocks;
        for (auto& row : rows) blocks.push_back(new Block<uint32_t>(row));
        for (uint32_t r = 0; r < p.n_rules(); r++) {
            // alone
            for (int t = 0; t < active; t++) {
                const uint32_t* row = blocks[t]->p;
                const bool got = rule_fires(v, r, true, [&](uint32_t w) { AM_BOUNDS(w < words); return row[w]; }, [](bool x) { return x; });
                if (got != naive(p, r, rows[t])) { g_failed++; std::printf("FAILED %s: rule %u, lane %d alone\n", what, r, t); }
            }
            if (rule_fires(v, r, false, [&](uint32_t w) { AM_BOUNDS(w < words); return blocks[0]->p[w]; }, [](bool x) { return x; })) { g_failed++; std::printf("FAILED %s: an idle caller fired\n", what); }
            // in lockstep with others: the group's answer to any(x) is true whenever the lane's own x is, and sometimes when it is not (another lane is still
            // undecided).  The result must not depend on it: never stopping early (always true) and stopping at the whim of the others (x || coin)
            for (int t = 0; t < kLanes; t++) {
                const bool is_active = t < active;
                const uint32_t* row = blocks[t]->p;
                const bool never_stop = rule_fires(v, r, is_active, [&](uint32_t w) { AM_BOUNDS(w < words); return row[w]; }, [](bool) { return true; });
                const bool others = rule_fires(v, r, is_active, [&](uint32_t w) { AM_BOUNDS(w < words); return row[w]; }, [&](bool x) { return x || (rng() & 1u) != 0; });
                const bool want = is_active && naive(p, r, rows[t]);
                if (never_stop != want || others != want) { g_failed++; std::printf("FAILED %s: rule %u, lane %d in lockstep\n", what, r, t); }
            }
        }
        for (auto* b : blocks) delete b;
    }
}

Program random_program(std::mt19937& rng, uint32_t n_slots, uint32_t n_rules)
{
    Program p;
    p.n_slots = n_slots;
    for (uint32_t r = 0; r < n_rules; r++) {
        const uint32_t n_clauses = n_slots ? rng() % 5 : rng() % 2;
        for (uint32_t c = 0; c < n_clauses; c++) {
            std::vector<uint32_t> lits;
            const uint32_t n_lits = n_slots ? rng() % 5 : 0;
            for (uint32_t l = 0; l < n_lits; l++) lits.push_back((rng() % n_slots) | (rng() % 3 == 0 ? 0x80000000u : 0u));
            if (!lits.empty() && rng() % 8 == 0) lits.push_back(lits[0]);      // a duplicate literal
            p.clause(lits);
        }
        p.end_rule();
    }
    return p;
}

}  // namespace

int main()
{
    std::mt19937 rng(20260);
    {
        Program p;                                          // the corners, over two slots
        p.n_slots = 2;
        p.end_rule();                                       // an empty rule: true
        p.clause({}); p.end_rule();                         // an empty clause: false
        p.clause({0x80000000u}); p.clause({0x80000001u}); p.end_rule();      // negative only
        p.clause({0}); p.clause({0x80000000u}); p.end_rule();                 // x AND NOT x
        p.clause({1, 0x80000001u}); p.end_rule();           // x OR NOT x
        p.clause({1, 1, 1}); p.end_rule();                  // duplicates
        p.clause({0}); p.clause({}); p.end_rule();          // an empty clause behind a true one
        check(p, rng, "corners");
        Program none;                                       // no rules at all
        none.n_slots = 3;
        check(none, rng, "no rules");
    }
    for (uint32_t n_slots : {0u, 1u, 2u, 31u, 32u, 33u, 63u, 64u, 65u, 1535u, 1536u, 1537u, 5000u})
        for (int k = 0; k < 40; k++) check(random_program(rng, n_slots, 1 + rng() % 40), rng, "random");
    std::printf(g_failed ? "%d FAILED\n" : "rules_eval: all programs agree with the three-loop evaluator\n", g_failed);
    return g_failed ? 1 : 0;
}
