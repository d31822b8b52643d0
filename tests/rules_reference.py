"""The definition of rule sets (include/am.h "rule sets") in Python.  P(h) -- the slots the fold of runWithCase over haystack h meets -- comes from
oracle.Machine(needles, slots).run_list(case, h)[1], values >= n_slots skipped; the program in conjunctive normal form is evaluated in plain Python: a literal is true
iff (slot in P(h)) != negated, a clause is any() of its literals, a rule all() of its clauses.  What the rule tests expect -- never another path of the library."""
import random

import numpy as np

from oracle import oracle

NEGATE = 0x80000000
NONE = 0xFFFFFFFF


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def program(rules):
    """(rule_off, clause_off, literals) of rules given as lists of clauses of literals (ints: the slot, | NEGATE when negated)."""
    rule_off, clause_off, literals = [0], [0], []
    for clauses in rules:
        for c in clauses:
            literals += [int(x) for x in c]
            clause_off.append(len(literals))
        rule_off.append(len(clause_off) - 1)
    return np.asarray(rule_off, np.uint64), np.asarray(clause_off, np.uint64), np.asarray(literals, np.uint32)


def rules_of(rule_off, clause_off, literals):
    """The inverse of program()."""
    return [[[int(x) for x in literals[int(clause_off[c]):int(clause_off[c + 1])]] for c in range(int(rule_off[r]), int(rule_off[r + 1]))] for r in range(len(rule_off) - 1)]


def present(needles, slots, n_slots, case):
    """h -> P(h)."""
    needles = list(needles)
    if not needles:
        return lambda h: set()
    m = oracle.Machine(needles, list(slots))
    return lambda h: {int(v) for v in m.run_list(case, _b(h))[1] if v < n_slots}


def fires(rule, p):
    """One rule (a list of clauses) on the slot set p."""
    return all(any(((x & ~NEGATE) in p) != bool(x & NEGATE) for x in clause) for clause in rule)


def expect(needles, slots, n_slots, case, rules, hays):
    """(fired_words uint64[n_rules, hay_words], fired bool[n_rules, n_hay], labels uint32[n_hay], counts uint64[n_rules]) of the rules (lists of clauses) over hays."""
    pres = present(needles, slots, n_slots, case)
    n_hay, n_rules = len(hays), len(rules)
    fired = np.zeros((n_rules, n_hay), bool)
    labels = np.full(n_hay, NONE, np.uint32)
    for h, hay in enumerate(hays):
        p = pres(hay)
        for r, rule in enumerate(rules):
            if fires(rule, p):
                fired[r, h] = True
                if labels[h] == NONE:
                    labels[h] = r
    return words_of(fired), fired, labels, fired.sum(axis=1).astype(np.uint64)


def words_of(fired):
    """bool[n_rules, n_hay] as uint64[n_rules, ceil(n_hay / 64)]: bit h % 64 of word h // 64, the bits beyond n_hay zero."""
    n_rules, n_hay = fired.shape
    hw = (n_hay + 63) // 64
    padded = np.zeros((n_rules, hw * 64), np.uint8)
    padded[:, :n_hay] = fired
    if n_rules == 0 or hw == 0:
        return np.zeros((n_rules, hw), np.uint64)
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(n_rules, hw)


def random_rules(rng, n_slots, n_rules, max_clauses=3, max_literals=3, negate=0.3):
    """n_rules random rules over slots 0 .. n_slots-1; now and then an empty rule, an empty clause, a duplicate literal."""
    rules = []
    for _ in range(n_rules):
        rule = []
        for _ in range(rng.randint(0, max_clauses) if n_slots else rng.randint(0, 1)):
            clause = [rng.randrange(n_slots) | (NEGATE if rng.random() < negate else 0) for _ in range(rng.randint(0, max_literals))] if n_slots else []
            if clause and rng.random() < 0.1:
                clause.append(clause[0])
            rule.append(clause)
        rules.append(rule)
    return rules


def rng(seed):
    return random.Random(seed)
