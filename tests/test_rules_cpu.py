"""am_rules_* / am_rule_hits_* / am_select_rule (include/am.h "rule sets"): the definition (tests/rules_reference.py) agrees with Python itself, the host mirror agrees
with the definition, the slot compiler shares slots where it may, and the entry points exist, are bound and check their arguments before any device work.

No needle-id table or batch can be made without a device: there the checks are seen with handles that are never looked at, and a well-formed call reaches the
runtime and reports AM_ERR_NO_DEVICE."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import rules_reference as ref
from tests.conftest import ROOT
from tests.test_select_cpu import cases

NAMES = ("am_rules_create", "am_rules_destroy", "am_rules_eval_batch", "am_rules_eval", "am_rule_hits_haystacks", "am_rule_hits_rules", "am_rule_hits_hay_words",
         "am_rule_hits_fired", "am_rule_hits_labels", "am_rule_hits_counts", "am_rule_hits_device_fired", "am_rule_hits_device_labels", "am_rule_hits_device_counts",
         "am_rule_hits_free", "am_select_rule", "am_rules_geometry")


def _gpu():
    import torch
    return torch.cuda.is_available()


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


@pytest.mark.parametrize("seed", range(2))
def test_the_definition_is_pythons_in_all_any(seed):
    """250 fragment-pool cases a seed, a random CNF each: the definition over the oracle's fold against `in`, any() and all() over the texts; under IgnoreCase with the
    needles lower-cased, where str.lower is the table's."""
    rng = random.Random(9100 + seed)
    for needles, hays, lower_ok in cases(5100 + seed, 250):
        needles = [n for n in needles if n]
        if not needles:
            continue
        rules = ref.random_rules(rng, len(needles), rng.randint(1, 6))
        for case in (0, 1) if lower_ok else (0,):
            ns = [n.lower() for n in needles] if case else needles
            _, fired, labels, counts = ref.expect(ns, range(len(ns)), len(ns), case, rules, hays)
            for h, hay in enumerate(hays):
                text = hay.lower() if case else hay
                got = [all(any((ns[x & ~ref.NEGATE] in text) != bool(x & ref.NEGATE) for x in c) for c in rule) for rule in rules]
                assert fired[:, h].tolist() == got, (ns, hay, rules)
                assert labels[h] == (got.index(True) if True in got else ref.NONE)
            assert counts.tolist() == fired.sum(axis=1).tolist()


def test_the_definitions_corners():
    needles, slots = ["a", "b", "ab"], [0, 1, 0]                                # two needles under one slot
    rules = [[], [[]], [[0 | ref.NEGATE], [1 | ref.NEGATE]], [[0], [0 | ref.NEGATE]], [[1, 1 | ref.NEGATE]], [[1, 1]], [[0], []]]
    words, fired, labels, counts = ref.expect(needles, slots, 2, 0, rules, ["", "a", "b", "xab", "c"])
    assert fired.astype(int).tolist() == [[1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [1, 0, 0, 0, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 1, 1, 0], [0, 0, 0, 0, 0]]
    assert labels.tolist() == [0] * 5 and counts.tolist() == [5, 0, 2, 0, 5, 2, 0] and words.shape == (7, 1) and words[:, 0].tolist() == [31, 0, 17, 0, 31, 12, 0]
    assert ref.rules_of(*ref.program(rules)) == rules
    # a value beyond the table is skipped
    _, fired, _, _ = ref.expect(["a", "b"], [0, 7], 1, 0, [[[0]]], ["a", "b"])
    assert fired.tolist() == [[True, False]]
    assert ref.expect([], [], 0, 0, [[], [[]]], ["x"])[2].tolist() == [0] and ref.words_of(np.zeros((0, 3), bool)).shape == (0, 1)


def steps_of(needles, slots, case, hays):
    """(haystack, value) arrays of the oracle's fold over the texts, in fold order."""
    m = oracle.Machine(list(needles), list(slots)) if needles else None
    hay, val = [], []
    for h, text in enumerate(hays):
        vs = m.run_list(case, _b(text))[1] if m else []
        hay += [h] * len(vs)
        val += [int(v) for v in vs]
    return np.asarray(hay, np.uint32), np.asarray(val, np.uint32)


@pytest.mark.parametrize("seed", range(2))
def test_the_host_mirror_is_the_definition(seed):
    rng = random.Random(9200 + seed)
    for needles, hays, _ in cases(5200 + seed, 120):
        n_slots = rng.randint(1, len(needles))
        slots = [rng.randrange(n_slots + 1) for _ in needles]                   # (n_slots itself: a value beyond the table)
        rules = ref.random_rules(rng, n_slots, rng.randint(0, 70))
        for case in (0, 1):
            ns = [oracle.lower_utf8(n).decode() for n in needles] if case else needles
            words, _, labels, counts = ref.expect(ns, slots, n_slots, case, rules, hays)
            hay, val = steps_of(ns, slots, case, hays)
            got = am.api.rules_fold_host(hay, val, len(hays), n_slots, *ref.program(rules))
            assert np.array_equal(got[0], words) and np.array_equal(got[1], labels) and np.array_equal(got[2], counts), (ns, slots, rules)
    # more than one word of haystacks; no rules; no haystacks
    rules = [[[0]], [[0 | ref.NEGATE]]]
    hays = ["a" if h % 3 == 0 else "b" for h in range(130)]
    words, _, labels, counts = ref.expect(["a"], [0], 1, 0, rules, hays)
    got = am.api.rules_fold_host(*steps_of(["a"], [0], 0, hays), 130, 1, *ref.program(rules))
    assert got[0].shape == (2, 3) and np.array_equal(got[0], words) and np.array_equal(got[1], labels) and np.array_equal(got[2], counts)
    got = am.api.rules_fold_host([], [], 3, 0, *ref.program([]))
    assert got[0].shape == (0, 1) and got[1].tolist() == [ref.NONE] * 3 and got[2].size == 0
    got = am.api.rules_fold_host([], [], 0, 1, *ref.program(rules))
    assert got[0].shape == (2, 0) and got[1].size == 0 and got[2].tolist() == [0, 0]
    for bad in (lambda: am.api.rules_fold_host([], [], 1, 1, [0, 1], [0, 1], [1]),            # a slot >= n_slots
                lambda: am.api.rules_fold_host([], [], 1, 1, [1, 1], [0, 0], []),            # offsets that do not start at 0
                lambda: am.api.rules_fold_host([2], [0], 1, 1, [0, 0], [0], [])):            # a fold step beyond the haystacks
        with pytest.raises(am.AmError) as e:
            bad()
        assert e.value.code == am.AM_ERR_INVALID


def test_the_slot_compiler():
    brands = ["brand%d" % i for i in range(1000)]
    rs = am.RuleSet(0, [am.Rule(any_of=brands)])
    assert rs.n_slots == 1 and len(rs.needles) == 1000 and set(rs.slots) == {0} and ref.rules_of(rs.rule_off, rs.clause_off, rs.literals) == [[[0]]]
    # the same list in two rules: the needles' memberships are the same two clauses -- still one slot; a needle of its own in one of them: a second slot
    rs = am.RuleSet(0, [am.Rule(any_of=brands), am.Rule(any_of=brands + ["own"])])
    assert rs.n_slots == 2 and ref.rules_of(rs.rule_off, rs.clause_off, rs.literals) == [[[0]], [[0, 1]]]
    # one needle, positive in one rule and negated in another: ONE needle with two memberships, a slot of its own
    rs = am.RuleSet(0, [am.Rule(all_of=["nike", "shoe"]), am.Rule(any_of=["adidas"], none_of=["nike"])])
    assert rs.needles == [b"nike", b"shoe", b"adidas"] and rs.n_slots == 3
    assert ref.rules_of(rs.rule_off, rs.clause_off, rs.literals) == [[[0], [1]], [[2], [0 | ref.NEGATE]]]
    # negated needles never share: NOT a OR NOT b is not NOT (a OR b)
    rs = am.RuleSet(0, [am.Rule.cnf([[am.Not("a"), am.Not("b")], ["c", "d"]])])
    assert rs.n_slots == 3 and ref.rules_of(rs.rule_off, rs.clause_off, rs.literals) == [[[0 | ref.NEGATE, 1 | ref.NEGATE], [2]]]
    # duplicates: by text (after lower-casing under IgnoreCase), inside a clause and across clauses
    rs = am.RuleSet(1, [am.Rule(any_of=["Nike", "NIKE", "nike", "Puma"]), am.Rule(all_of=["puma", "puma"])])
    assert rs.needles == [b"nike", b"puma"] and rs.n_slots == 2
    assert ref.rules_of(rs.rule_off, rs.clause_off, rs.literals) == [[[0, 1]], [[1], [1]]]
    # an absent any_of adds no clause, an explicit empty one adds an empty clause; no rules at all
    rs = am.RuleSet(0, [am.Rule(), am.Rule(any_of=[]), am.Rule(all_of=["a"], any_of=[])])
    assert rs.n_slots == 1 and ref.rules_of(rs.rule_off, rs.clause_off, rs.literals) == [[], [[]], [[0], []]]
    rs = am.RuleSet(0, [])
    assert rs.n_slots == 0 and rs.rule_off.tolist() == [0] and rs.clause_off.tolist() == [0] and rs.literals.size == 0


def test_the_compiled_program_means_what_the_rules_say():
    """The rules over needles, evaluated with Python's `in`, against the definition over the compiled slots."""
    rng = random.Random(77)
    words = ["ab", "b", "abc", "c", "ca", "aa", "x"]
    for _ in range(60):
        rules = []
        for _ in range(rng.randint(1, 5)):
            kind = rng.random()
            if kind < 0.5:
                rules.append(am.Rule(all_of=rng.sample(words, rng.randint(0, 2)), any_of=rng.choice([None, [], rng.sample(words, rng.randint(1, 4))]),
                                     none_of=rng.sample(words, rng.randint(0, 2))))
            else:
                rules.append(am.Rule.cnf([[am.Not(w) if rng.random() < 0.4 else w for w in rng.sample(words, rng.randint(0, 3))] for _ in range(rng.randint(0, 3))]))
        rs = am.RuleSet(0, rules)
        hays = ["".join(rng.choice("abcx") for _ in range(rng.randint(0, 6))) for _ in range(20)]
        _, fired, _, _ = ref.expect(rs.needles, rs.slots, rs.n_slots, 0, ref.rules_of(rs.rule_off, rs.clause_off, rs.literals), hays)
        for r, rule in enumerate(rules):
            for h, hay in enumerate(hays):
                assert fired[r, h] == all(any((n in hay) != neg for n, neg in c) for c in rule.clauses), (rule.clauses, hay)


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    assert re.search(r"typedef struct am_rules am_rules;", src) and re.search(r"typedef struct am_rule_hits am_rule_hits;", src)
    assert re.search(r"#define AM_RULE_NEGATE 0x80000000u", src) and re.search(r"#define AM_RULE_FIRED 0", src) and re.search(r"#define AM_RULE_FIRST 1", src)
    assert len(am.api.DEBUG_ABI) == 14                     # no new am_debug_* symbol
    assert "AM_RULES_ROWS_MIB" in am.api.DEBUG_SWITCHES
    for n in ("RuleSet", "Rule", "Not", "RuleHits", "rules_geometry", "rules_fold_host", "compile_rules"):
        assert hasattr(am.api, n), n
    build_py = open(os.path.join(ROOT, "alfred-margaret_amd", "build.py")).read()
    assert '"am_rules.cpp"' in build_py and '"am_rules.hip"' in build_py


def test_the_geometry_is_known_without_a_device():
    tile, slot_words, rules = am.api.rules_geometry()
    assert tile >= 64 and tile % 64 == 0 and slot_words >= 1 and rules >= 1
    assert (slot_words * (tile + 1) * 4 + rules * 8) * 2 <= 160 << 10      # two workgroups fit the LDS of a CU
    am.api.libam().am_rules_geometry(None, None, None)


def test_every_argument_is_refused_before_any_device_work():
    lib = am.api.libam()
    s = am.api._Slices(["abc"])
    out = C.c_void_p(1)
    fake = C.c_void_p(1)                                   # a handle that is never looked at: the check that refuses the call comes first

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and not out.value and word in lib.am_last_error(), (rc, out.value, lib.am_last_error())
        out.value = 1

    def u64(*xs):
        return np.asarray(xs, np.uint64)

    lits = np.asarray([0], np.uint32)
    ok_r, ok_c = u64(0, 1), u64(0, 1)
    create = lambda slots, ro, co, li, n, o: lib.am_rules_create(slots, None if ro is None else ro.ctypes.data, None if co is None else co.ctypes.data,
                                                                 None if li is None else li.ctypes.data, n, o)
    assert create(fake, ok_r, ok_c, lits, 1, None) == am.AM_ERR_INVALID
    refused(create(fake, ok_r, ok_c, lits, 0xFFFFFFFF, C.byref(out)), b"too many rules")
    refused(create(fake, None, ok_c, lits, 1, C.byref(out)), b"rule_off is null")
    refused(create(fake, u64(1, 1), ok_c, lits, 1, C.byref(out)), b"rule_off[0] must be 0")
    refused(create(fake, u64(0, 2, 1), u64(0, 1, 1), lits, 2, C.byref(out)), b"rule_off decreases")
    refused(create(fake, ok_r, None, lits, 1, C.byref(out)), b"clause_off is null")
    refused(create(fake, ok_r, u64(1, 1), lits, 1, C.byref(out)), b"clause_off[0] must be 0")
    refused(create(fake, u64(0, 2), u64(0, 1, 0), lits, 1, C.byref(out)), b"clause_off decreases")
    refused(create(fake, ok_r, ok_c, None, 1, C.byref(out)), b"literals is null")
    refused(create(None, ok_r, ok_c, lits, 1, C.byref(out)), b"null slot table")
    refused(create(None, u64(0), u64(0), None, 0, C.byref(out)), b"null slot table")
    lib.am_rules_destroy(None)
    # the evaluations
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    assert lib.am_rules_eval(fake, 0, s.arr, s.n, None) == am.AM_ERR_INVALID
    refused(lib.am_rules_eval(fake, 0, None, 1, C.byref(out)), b"hay is null")
    refused(lib.am_rules_eval(fake, 1, s.arr, 0xFFFFFFFF, C.byref(out)), b"too many")
    refused(lib.am_rules_eval(fake, 0, bad, 1, C.byref(out)), b"slice with null ptr")
    refused(lib.am_rules_eval(fake, 2, s.arr, s.n, C.byref(out)), b"case_mode")
    refused(lib.am_rules_eval(None, 0, s.arr, s.n, C.byref(out)), b"null rules")
    assert lib.am_rules_eval_batch(fake, 0, fake, None) == am.AM_ERR_INVALID
    refused(lib.am_rules_eval_batch(fake, -1, fake, C.byref(out)), b"case_mode")
    refused(lib.am_rules_eval_batch(None, 0, fake, C.byref(out)), b"null rules or batch")
    refused(lib.am_rules_eval_batch(fake, 1, None, C.byref(out)), b"null rules or batch")
    # the select
    assert lib.am_select_rule(fake, 0, 0, 0, fake, None) == am.AM_ERR_INVALID
    refused(lib.am_select_rule(fake, 0, 2, 0, fake, C.byref(out)), b"which")
    refused(lib.am_select_rule(fake, 0, -1, 1, fake, C.byref(out)), b"which")
    refused(lib.am_select_rule(None, 0, 0, 0, fake, C.byref(out)), b"null rule hits or batch")
    refused(lib.am_select_rule(fake, 0, 1, 0, None, C.byref(out)), b"null rule hits or batch")
    # the accessors of a null result
    assert lib.am_rule_hits_haystacks(None) == 0 and lib.am_rule_hits_rules(None) == 0 and lib.am_rule_hits_hay_words(None) == 0
    assert not lib.am_rule_hits_fired(None) and not lib.am_rule_hits_labels(None) and not lib.am_rule_hits_counts(None)
    assert not lib.am_rule_hits_device_fired(None) and not lib.am_rule_hits_device_labels(None) and not lib.am_rule_hits_device_counts(None)
    lib.am_rule_hits_free(None)
    if not _gpu():
        # valid arguments reach the runtime
        x = C.c_void_p(1)
        assert lib.am_rules_eval(fake, 0, None, 0, C.byref(x)) == am.AM_ERR_NO_DEVICE and x.value is None
    # (the refusals that need a real slot table or rule set -- a literal's slot >= n_slots, rule >= n_rules -- are in tests/test_gpu_rules.py)


def test_without_a_gpu_the_front_end_reports_no_device():
    rs = am.RuleSet(am.IGNORE_CASE, [am.Rule(all_of=["nike", "shoe"], none_of=["kids"]), am.Rule(any_of=["adidas", "puma"])])      # compiled on the host
    assert rs.n_slots == 4
    if _gpu():
        return                                             # (what the front end computes is tests/test_gpu_rules.py's)
    with pytest.raises(am.AmError) as e:
        rs.eval(["nike shoe"])
    assert e.value.code == am.AM_ERR_NO_DEVICE
