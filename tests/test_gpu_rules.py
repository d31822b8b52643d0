"""Rule sets on the device (am_rules_* / am_select_rule, csrc/am_rules.hip) against the definition.  Every check compares every word of `fired` (tail bits included),
the labels and the counts with what tests/rules_reference.py says -- built over the oracle's fold and plain Python -- never with another path of the library.  Shapes
sit on the real seams: the evaluation's tile, the widest slot row it keeps in LDS and its LDS count table (am_rules_geometry)."""
import ctypes as C
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from tests import rules_reference as ref, select_reference as sel
from tests.test_gpu_select import Batch, check_texts, lib, lowered, pool_case

pytestmark = pytest.mark.gpu

ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}
N, NONE = ref.NEGATE, ref.NONE


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield ROUTES[request.param]
    am.debug_set("AM_DFA", -1)


def rule_set(case, needles, slots, n_slots, rules, route=0):
    rs = am.RuleSet.from_program(case, needles, slots, n_slots, *ref.program(rules))
    rs.automaton.set_kernel(route)
    return rs


def check_hits(hits, expected, what=None):
    """Every word of fired, the labels, the counts; counts == popcount(fired)."""
    words, fired, labels, counts = expected
    n_rules, n_hay = fired.shape
    assert (hits.n_rules, hits.n_hay, hits.hay_words) == (n_rules, n_hay, (n_hay + 63) // 64), what
    got = hits.fired_words
    assert got.dtype == np.uint64 and got.shape == words.shape, what
    if not np.array_equal(got, words):
        r, w = np.argwhere(got != words)[0]
        raise AssertionError((what, "fired", int(r), int(w), hex(int(got[r, w])), hex(int(words[r, w]))))
    assert np.array_equal(hits.labels, labels), (what, "labels", np.flatnonzero(hits.labels != labels)[:8].tolist())
    assert np.array_equal(hits.counts, counts), (what, "counts", hits.counts[:8].tolist(), counts[:8].tolist())
    assert hits.counts.tolist() == [int(sum(bin(int(x)).count("1") for x in row)) for row in got], what
    assert np.array_equal(hits.fired, fired)
    assert bool(lib().am_rule_hits_device_fired(hits.handle)) == (n_rules * n_hay > 0)
    assert bool(lib().am_rule_hits_device_labels(hits.handle)) == (n_hay > 0) and bool(lib().am_rule_hits_device_counts(hits.handle)) == (n_rules > 0)


def run_and_check(needles, slots, n_slots, rules, hays, cases=(0, 1), route=0, what=None):
    """The batch form, twice (bit-identical from run to run), and the one-shot form, in both case modes, against the definition."""
    for case in cases:
        ns = lowered(needles) if case else list(needles)
        expected = ref.expect(ns, slots, n_slots, case, rules, hays)
        rs = rule_set(case, ns, slots, n_slots, rules, route)
        with Batch(hays) as b:
            first = rs.eval_batch(b)
            check_hits(first, expected, (what, case))
            again = rs.eval_batch(b)
            assert np.array_equal(first.fired_words, again.fired_words) and np.array_equal(first.labels, again.labels) and np.array_equal(first.counts, again.counts)
        check_hits(rs.eval(hays), expected, (what, case, "one-shot"))
    return expected


def short_hays(rng, n, alphabet, needles=()):
    """n haystacks of 0 .. 49 bytes, some empty, some that hold a few needles."""
    hays = []
    for k in range(n):
        if k % 29 == 7:
            hays.append("")
        elif needles and k % 5 == 0:
            hays.append(" ".join(rng.choice(needles) for _ in range(rng.randint(1, 6)))[:49])
        else:
            hays.append("".join(rng.choice(alphabet) for _ in range(rng.randint(0, 49))))
    return hays


# ---- 1. shapes: haystacks, slots, rules around every internal limit

HAY_COUNTS = [1, 63, 64, 65, "tile - 1", "tile", "tile + 1", "2 * tile + 1"]


@pytest.mark.parametrize("n_hay", HAY_COUNTS)
def test_haystack_counts(n_hay):
    tile, _, _ = am.api.rules_geometry()
    n_hay = n_hay if isinstance(n_hay, int) else {"tile - 1": tile - 1, "tile": tile, "tile + 1": tile + 1, "2 * tile + 1": 2 * tile + 1}[n_hay]
    rng = random.Random(n_hay)
    needles = ["ab", "b", "abc", "ca", "1", "A2"]
    rules = ref.random_rules(rng, len(needles), 9) + [[], [[0], [3 | N]]]
    hays = short_hays(rng, n_hay, "abcAB12 ", needles)
    hays[-1] = "abc 1"                                      # the last haystack: the last bit of the tail word
    _, fired, _, _ = run_and_check(needles, range(len(needles)), len(needles), rules, hays, what=n_hay)
    assert fired[-2].all() and fired[-1, -1]


def byte_needles(n):
    """n distinct needles of one and two bytes: the dictionary stays tiny however many slots there are."""
    alphabet = "abcdefghijklmnopqrstuvwxyz0123456789ABCD"
    out = list(alphabet) + [x + y for x in alphabet for y in alphabet]
    assert n <= len(out)
    return out[:n], alphabet


SLOT_COUNTS = [1, 31, 32, 33, 64, 65, "lds - 1", "lds", "lds + 1"]


@pytest.mark.parametrize("n_slots", SLOT_COUNTS)
def test_slot_counts(n_slots):
    """Rows of one word, around a word, and around the widest row the evaluation keeps in LDS (beyond: the rows are read in HBM); over more than one tile."""
    tile, lds_words, _ = am.api.rules_geometry()
    n_slots = n_slots if isinstance(n_slots, int) else lds_words * 32 + {"lds - 1": -1, "lds": 0, "lds + 1": 1}[n_slots]
    rng = random.Random(n_slots)
    needles, alphabet = byte_needles(n_slots)
    last = n_slots - 1
    rules = ref.random_rules(rng, n_slots, 20, max_literals=6) + [[[last]], [[last | N]], [[0], [last | N]], [[x for x in range(n_slots)]], [[x | N] for x in range(min(n_slots, 40))]]
    hays = short_hays(rng, tile + 70, alphabet + "    ")
    hays[3] = needles[last] + " " + needles[0]
    run_and_check(needles, range(n_slots), n_slots, rules, hays, cases=(0,), what=n_slots)
    if n_slots in (33, lds_words * 32 + 1):
        run_and_check(needles, range(n_slots), n_slots, rules, hays[:80], cases=(1,), what=n_slots)


RULE_COUNTS = [0, 1, 31, 32, 33, 65, "lds - 1", "lds", "lds + 1", "lds + 70"]


@pytest.mark.parametrize("n_rules", RULE_COUNTS)
def test_rule_counts(n_rules):
    """... around the LDS count table: the counts of the rules beyond it are added in HBM per wavefront."""
    tile, _, lds_rules = am.api.rules_geometry()
    n_rules = n_rules if isinstance(n_rules, int) else lds_rules + {"lds - 1": -1, "lds": 0, "lds + 1": 1, "lds + 70": 70}[n_rules]
    rng = random.Random(n_rules)
    needles = ["ab", "b", "abc", "ca", "1", "A2", "2"]
    rules = ref.random_rules(rng, len(needles), n_rules, max_clauses=2)
    if n_rules:
        rules[-1] = [[1], [4 | N]]                          # the last rule fires somewhere, not everywhere
    hays = short_hays(rng, tile + 45, "abcAB12 ", needles)
    _, fired, _, counts = run_and_check(needles, range(len(needles)), len(needles), rules, hays, cases=(0,), what=n_rules)
    if n_rules:
        assert 0 < counts[-1] < len(hays)


def test_corner_rules():
    needles, slots = ["a", "b", "ab", "zz"], [0, 1, 0, 5]                       # two needles under one slot; a value beyond the table
    rules = [[[]], [], [[0 | N], [1 | N]], [[0], [0 | N]], [[1, 1 | N]], [[1, 1]], [[0], []], [[0 | N, 0 | N]], [[1], [1], [1]]]
    hays = ["", "a", "b", "xab", "c", "zz", ""] * 11
    _, fired, labels, counts = run_and_check(needles, slots, 2, rules, hays)
    assert not fired[0].any() and fired[1].all() and fired[4].all() and not fired[3].any() and not fired[6].any()
    assert fired[2].astype(int).tolist() == [1, 0, 0, 0, 1, 1, 1] * 11         # negative only: fires on the empty haystacks (and where neither occurs)
    assert set(labels.tolist()) == {1}
    # rules without slots at all: a dictionary without needles, nothing is scanned
    run_and_check([], [], 0, [[], [[]], []], ["abc", "", "x"], what="no slots")
    # no haystacks
    for rules in ([[[0]], []], []):
        rs = rule_set(0, ["a"], [0], 1, rules)
        with Batch([]) as b:
            hits = rs.eval_batch(b)
            check_hits(hits, ref.expect(["a"], [0], 1, 0, rules, []))
            assert hits.counts.tolist() == [0] * len(rules) and hits.labels.size == 0


# ---- 2. routes

@pytest.mark.parametrize("no_ids_scan", [0, 1])
@pytest.mark.parametrize("seed", range(2))
def test_scan_routes(route, seed, no_ids_scan):
    """The three scan routes, with the slot bits set inside the scan and -- AM_NO_IDS_SCAN -- folded from the records; one haystack whose row is full after its first
    bytes, with text behind it."""
    needles, hays = pool_case(200 + seed, n_hay=280, max_frags=6, alphabet="abAB12" if seed else None)
    rng = random.Random(seed)
    n_slots = max(1, len(needles) - 2)
    slots = [rng.randrange(n_slots) for _ in needles]
    slots[:n_slots] = range(n_slots)                        # every slot has a needle
    rules = ref.random_rules(rng, n_slots, 12) + [[[x] for x in range(n_slots)], [[x | N for x in range(n_slots)]]]
    hays[9] = "".join(needles) + " " + " ".join(needles) + hays[10]
    am.debug_set("AM_NO_IDS_SCAN", no_ids_scan)
    try:
        _, fired, _, _ = run_and_check(needles, slots, n_slots, rules, hays, route=route, what=(seed, no_ids_scan))
        assert fired[-2, 9] and not fired[-1, 9]
    finally:
        am.debug_set("AM_NO_IDS_SCAN", -1)


@pytest.mark.parametrize("route", [ROUTES["default"], ROUTES["suffix_filter"]])      # (the empty needle: no DFA section, no table walk)
def test_a_dictionary_with_the_empty_needle(route):
    """The dense route: whatever the reference's fold does with the empty needle holds here."""
    needles, hays = pool_case(11, n_hay=150, max_frags=6)
    needles = needles + [""]
    n = len(needles)
    rules = ref.random_rules(random.Random(4), n, 10) + [[[n - 1]], [[(n - 1) | N]], [[0], [n - 1]]]
    run_and_check(needles, range(n), n, rules, hays, route=route)
    run_and_check([""], [0], 1, [[[0]], [[0 | N]]], hays[:40], route=route, what="the empty needle alone")


# ---- 3. groups

@pytest.mark.parametrize("no_ids_scan", [0, 1])
def test_groups_of_bounded_row_memory(no_ids_scan):
    """AM_RULES_ROWS_MIB = 0: the smallest group, 64 haystacks, so 1 000 haystacks take 16 groups with a text of their own each; the same result as in one piece."""
    needles, hays = pool_case(31, n_hay=1000, max_frags=6)
    rng = random.Random(8)
    rules = ref.random_rules(rng, len(needles), 40) + [[]]
    expected = ref.expect(needles, range(len(needles)), len(needles), 0, rules, hays)
    rs = rule_set(0, needles, range(len(needles)), len(needles), rules)
    am.debug_set("AM_NO_IDS_SCAN", no_ids_scan)
    try:
        with Batch(hays) as b:
            whole = rs.eval_batch(b)
            check_hits(whole, expected, "one piece")
            am.api.check(lib().am_profile_reset())
            am.api.check(lib().am_profile_enable(1))
            am.debug_set("AM_RULES_ROWS_MIB", 0)
            try:
                grouped = rs.eval_batch(b)
            finally:
                am.debug_set("AM_RULES_ROWS_MIB", -1)
                am.api.check(lib().am_profile_enable(0))
            check_hits(grouped, expected, "groups")
            assert np.array_equal(whole.fired_words, grouped.fired_words) and np.array_equal(whole.labels, grouped.labels) and np.array_equal(whole.counts, grouped.counts)
            ms, n = C.c_double(0), C.c_uint64(0)
            am.api.check(lib().am_profile_read(b"rules_eval", C.byref(ms), C.byref(n)))
            assert n.value == 16
    finally:
        am.debug_set("AM_NO_IDS_SCAN", -1)


# ---- 4. am_select_rule

def test_select_rule_fired_and_first():
    needles, hays = pool_case(5, n_hay=200, max_frags=6)
    rng = random.Random(12)
    rules = ref.random_rules(rng, len(needles), 4, negate=0.2) + [[[0], [1 | N]]]
    _, fired, labels, _ = ref.expect(needles, range(len(needles)), len(needles), 0, rules, hays)
    rs = rule_set(0, needles, range(len(needles)), len(needles), rules)
    with Batch(hays) as b:
        hits = rs.eval_batch(b)
        seen = np.zeros(len(hays), int)
        for r in range(len(rules)):
            for invert in (False, True):
                want = {False: np.flatnonzero(fired[r] != invert).tolist(), True: np.flatnonzero((labels == r) != invert).tolist()}
                for first in (False, True):
                    s = hits.select(r, first=first, invert=invert, batch=b)
                    assert s.indices.tolist() == want[first], (r, first, invert)
                    if r in (0, len(rules) - 1):           # am_batch_from_selection on it: every byte and offset
                        check_texts(b, s, hays, want[first], (r, first, invert))
            seen[hits.select(r, first=True, batch=b).indices] += 1
        # the FIRST selections over all rules and "no rule fires" are a partition of the batch
        none = np.flatnonzero(labels == NONE)
        assert 0 < len(none) < len(hays)
        flags = np.zeros(len(hays), np.uint8)
        flags[none] = 1
        seen[am.api.select_flags(b, flags).indices] += 1
        assert seen.tolist() == [1] * len(hays)


def test_select_rule_on_a_batch_of_lines():
    """lines -> category -> batch per category, without leaving the device."""
    rng = random.Random(3)
    words = ["nike", "shoe", "kids", "adidas", "puma", "sock", "red", "blue"]
    lines = [" ".join(rng.choice(words) for _ in range(rng.randint(0, 6))) for _ in range(400)]
    rs = am.RuleSet(am.IGNORE_CASE, [am.Rule(all_of=["nike", "shoe"], none_of=["kids"]), am.Rule(any_of=["Adidas", "PUMA"]), am.Rule.cnf([["sock", am.Not("red")], ["blue"]])])
    expected = ref.expect(rs.needles, rs.slots, rs.n_slots, 1, ref.rules_of(rs.rule_off, rs.clause_off, rs.literals), lines)
    with Batch(["\n".join(lines)]) as doc:
        lb, _ = am.Splitter("\n").lines_batch(doc)
        try:
            hits = rs.eval_batch(lb)
            check_hits(hits, expected)
            for r in range(3):
                want = np.flatnonzero(expected[2] == r).tolist()
                assert want
                s = hits.select(r, first=True, batch=lb)
                check_texts(lb, s, lines, want, ("category", r))
                nb = s.batch(lb)
                try:
                    again = rs.eval_batch(nb)                              # a category's batch goes into the next stage
                    assert again.labels.tolist() == [r] * len(want)
                finally:
                    lib().am_batch_destroy(nb)
        finally:
            lib().am_batch_destroy(lb)
    fired, labels, counts = rs.eval_host_mirror(lines)
    assert np.array_equal(fired, expected[1]) and np.array_equal(labels, expected[2]) and np.array_equal(counts, expected[3])


# ---- 5. identities

@pytest.mark.parametrize("seed", range(2))
def test_one_clause_is_contains_any_and_unit_clauses_are_contains_all(seed):
    needles, hays = pool_case(60 + seed, n_hay=300, n_needles=3 if seed else None, max_frags=6)
    n = len(needles)
    rules = [[list(range(n))], [[x] for x in range(n)]]
    for case in (0, 1):
        ns = lowered(needles) if case else needles
        rs = rule_set(case, ns, range(n), n, rules)
        any_flags, all_flags = np.zeros(len(hays), np.uint8), np.zeros(len(hays), np.uint8)
        ids = am.api.ValuesTable(rs.automaton)
        with Batch(hays) as b:
            hits = rs.eval_batch(b)
            am.api.check(lib().am_contains_any_batch(rs.automaton.device, case, b, any_flags.ctypes.data))
            am.api.check(lib().am_contains_all_batch(ids.handle, case, b, all_flags.ctypes.data))
        assert hits.fired[0].tolist() == any_flags.astype(bool).tolist() == [sel.pred_any(ns, case)(h.encode()) for h in hays]
        assert hits.fired[1].tolist() == all_flags.astype(bool).tolist() == [sel.pred_all(ns, case)(h.encode()) for h in hays]
        assert hits.fired[1].any() and not hits.fired[1].all()


# ---- 6. errors, lifetimes, names

def test_the_hits_belong_to_their_batch():
    out = C.c_void_p(1)
    rs = am.RuleSet(0, [am.Rule(any_of=["ab"]), am.Rule(none_of=["c"])])
    with Batch(["ab", "c", "abc"]) as b, Batch(["ab", "c"]) as fewer, Batch(["ab", "c", "abcd"]) as longer:
        hits = rs.eval_batch(b)
        for other in (fewer, longer):
            assert lib().am_select_rule(hits.handle, 0, 0, 0, other, C.byref(out)) == am.AM_ERR_INVALID and not out.value
            assert b"haystack count and size" in lib().am_last_error()
            out.value = 1
        assert lib().am_select_rule(hits.handle, 2, 0, 0, b, C.byref(out)) == am.AM_ERR_INVALID and not out.value
        assert hits.select(0, batch=b).indices.tolist() == [0, 2] and hits.select(1, first=True, batch=b).indices.tolist() == []
    import torch
    if torch.cuda.device_count() > 1:                      # handles on different devices
        s = am.api._Slices(["ab"])
        torch.cuda.set_device(1)
        try:
            far = C.c_void_p()
            am.api.check(lib().am_batch_upload(s.arr, s.n, C.byref(far)))
        finally:
            torch.cuda.set_device(0)
        out.value = 1
        assert lib().am_rules_eval_batch(rs.handle, 0, far, C.byref(out)) == am.AM_ERR_INVALID and not out.value and b"different devices" in lib().am_last_error()
        lib().am_batch_destroy(far)
    # free and destroy in either order
    bh = Batch(["ab", "c", "abc"])
    b = bh.__enter__()
    hits = rs.eval_batch(b)
    s = hits.select(1, batch=b)
    bh.__exit__()
    assert hits.fired.astype(int).tolist() == [[1, 0, 1], [1, 0, 0]] and hits.labels.tolist() == [0, NONE, 0] and hits.counts.tolist() == [2, 1]      # the batch is gone
    assert s.indices.tolist() == [0]
    del hits
    bh = Batch(["ab"])
    b = bh.__enter__()
    hits = rs.eval_batch(b)
    h = hits.handle
    hits._h = None
    lib().am_rule_hits_free(h)                              # the hits before their batch
    bh.__exit__()
    before = am.api.libam().am_debug_device_buffer_bytes()
    other = am.RuleSet(0, [am.Rule(any_of=["x"])])
    with Batch(["x"]) as b:
        assert other.eval_batch(b).counts.tolist() == [1]
    del other
    assert am.api.libam().am_debug_device_buffer_bytes() <= before      # a rule set, its hits and its batch leave nothing behind


def test_the_refusals_that_need_real_handles():
    """A literal whose slot is >= n_slots, plain and negated; a case_mode and a rule number on a real rule set; *out is NULL after each."""
    out = C.c_void_p(1)

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and not out.value and word in lib().am_last_error(), (rc, out.value, lib().am_last_error())
        out.value = 1

    rs = am.RuleSet(am.IGNORE_CASE, [am.Rule(all_of=["nike", "shoe"], none_of=["kids"]), am.Rule(any_of=["adidas", "puma"])])
    assert rs.n_slots == 4
    t = am.api.ValuesTable(rs.automaton, n_needles=rs.n_slots)
    one = np.asarray([0, 1], np.uint64)
    for lit in (4, 4 | N, 0x7FFFFFFF):
        lits = np.asarray([lit], np.uint32)
        refused(lib().am_rules_create(t.handle, one.ctypes.data, one.ctypes.data, lits.ctypes.data, 1, C.byref(out)), b"slot >= n_slots")
    lits = np.asarray([3 | N], np.uint32)                   # the last slot is fine
    out.value = None
    am.api.check(lib().am_rules_create(t.handle, one.ctypes.data, one.ctypes.data, lits.ctypes.data, 1, C.byref(out)))
    lib().am_rules_destroy(out)
    hays = ["Nike shoe", "nike kids shoe", "PUMA", ""]
    with Batch(hays) as b:
        out.value = 1
        refused(lib().am_rules_eval_batch(rs.handle, 5, b, C.byref(out)), b"case_mode")
        hits = rs.eval_batch(b)
        refused(lib().am_select_rule(hits.handle, 2, 0, 0, b, C.byref(out)), b"rule is not below")
        refused(lib().am_select_rule(hits.handle, 0, 7, 0, b, C.byref(out)), b"which")
        assert hits.fired.astype(int).tolist() == [[1, 0, 0, 0], [0, 0, 1, 0]] and hits.labels.tolist() == [0, NONE, 1, NONE] and hits.counts.tolist() == [1, 1]


def test_two_threads_on_one_batch():
    """Calls on the SAME batch from two threads, each on a stream of its own, serialise on the batch's workspaces: a rule-set evaluation in one piece and containsAny
    scans of the same batch side by side, every result equal to the definition."""
    import threading
    needles, hays = pool_case(44, n_hay=600, max_frags=6)
    n = len(needles)
    rules = ref.random_rules(random.Random(2), n, 20) + [[[x] for x in range(n)]]
    expected = ref.expect(needles, range(n), n, 0, rules, hays)
    want_any = [sel.pred_any(needles, 0)(h.encode()) for h in hays]
    rs = rule_set(0, needles, range(n), n, rules)
    other = am.Automaton(needles[:2])
    want_other = [sel.pred_any(needles[:2], 0)(h.encode()) for h in hays]
    with Batch(hays) as b:
        rs.eval_batch(b)                                    # (the images are on the device before the threads start)
        got, errors = {"hits": [], "any": []}, []

        def evaluate():
            try:
                for _ in range(12):
                    got["hits"].append(rs.eval_batch(b))
            except Exception as e:                          # noqa: BLE001 -- reported below
                errors.append(e)

        def scan():
            try:
                for k in range(24):
                    flags = np.zeros(len(hays), np.uint8)
                    a = other if k % 2 else rs.automaton
                    am.api.check(lib().am_contains_any_batch(a.device, 0, b, flags.ctypes.data))
                    got["any"].append((k % 2, flags.astype(bool).tolist()))
            except Exception as e:                          # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=evaluate), threading.Thread(target=scan)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for hits in got["hits"]:
            check_hits(hits, expected, "beside a scan")
        for odd, flags in got["any"]:
            assert flags == (want_other if odd else want_any)


def test_the_launches_have_names():
    needles, hays = pool_case(3)
    rs = rule_set(0, needles, range(len(needles)), len(needles), [[[0]], [[1 | N]]])
    am.api.check(lib().am_profile_reset())
    am.api.check(lib().am_profile_enable(1))
    try:
        with Batch(hays) as b:
            hits = rs.eval_batch(b)
            hits.select(0, batch=b)
            hits.select(1, first=True, batch=b)
    finally:
        am.api.check(lib().am_profile_enable(0))
    for k, want in ((b"rules_eval", 1), (b"rule_flags", 2), (b"select_plan", 2)):
        ms, n = C.c_double(0), C.c_uint64(0)
        am.api.check(lib().am_profile_read(k, C.byref(ms), C.byref(n)))
        assert n.value == want, k
