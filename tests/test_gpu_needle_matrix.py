"""am_count_matrix* on the device against the oracle: row i of the matrix = Map.toAscList of the fold `Map.insertWith (+) v 1` that the reference's runWithCase
(Automaton.hs:442-553) runs over haystack i.  Expected values are np.unique(val[val < n], return_counts=True) over oracle.Machine.run_list per haystack, or
arithmetic; never another path of the library.  Every comparison is on the offsets and on the entries' bytes."""
import ctypes as C
import functools
import itertools
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from alfred_margaret_amd import synth
from oracle import oracle
from tests.helpers import fragment_case

pytestmark = pytest.mark.gpu

DT = am.api.NEEDLE_COUNT_DTYPE
LIMITS = am.api.needle_matrix_limits


class Batch:
    """am_batch_upload of some texts, destroyed on exit."""

    def __init__(self, hays):
        self.s = am.api._Slices(hays)
        self.h = C.c_void_p()

    def __enter__(self):
        am.api.check(am.api.libam().am_batch_upload(self.s.arr, self.s.n, C.byref(self.h)))
        return self.h

    def __exit__(self, *exc):
        am.api.libam().am_batch_destroy(self.h)


def matrix_of_rows(rows):
    """(offsets, entries) of [(needles ascending, counts)] per haystack."""
    offs = np.zeros(len(rows) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r[0]) for r in rows], dtype=np.uint64)
    ents = np.zeros(int(offs[-1]), DT)
    at = 0
    for i, (v, c) in enumerate(rows):
        k = len(v)
        ents["needle"][at:at + k], ents["count"][at:at + k], ents["haystack"][at:at + k] = v, c, i
        at += k
    return offs, ents


def oracle_matrix(o, case, hays, n):
    rows = []
    for h in hays:
        _, val = o.run_list(case, h)
        rows.append(np.unique(val[val < n], return_counts=True))
    return matrix_of_rows(rows)


def same(got, exp, what=None):
    assert got[0].dtype == np.uint64 and got[1].dtype == DT, what
    assert got[0].tolist() == exp[0].tolist(), what
    assert got[1].tobytes() == exp[1].tobytes(), what


def all_forms(a, case, hays, n):
    """The one-shot form, the batch form, the fold over a held am_run_batch result and the host mirror: four matrices that must be one."""
    lib = am.api.libam()
    t = am.ValuesTable(a, n)
    got = [t.count_matrix_texts(case, hays)]
    with Batch(hays) as b:
        got.append(t.count_matrix_batch(case, b))
        m = C.c_void_p()
        am.api.check(lib.am_run_batch(a.device, case, b, C.byref(m)))
        try:
            got.append(t.count_matrix(m, len(hays)))
        finally:
            lib.am_matches_free(m)
    got.append(a.count_matrix_host_mirror(case, hays, n))
    return got


def check_case(needles, hays, case, kernel, values=None, n=None):
    n = len(needles) if n is None else n
    exp = oracle_matrix(oracle.Machine(needles, values), case, hays, n)
    a = am.Automaton(needles, values)
    a.set_kernel(kernel)
    for form, got in enumerate(all_forms(a, case, hays, n)):
        same(got, exp, (form, kernel, case, needles, hays, values, n))
    assert not (exp[1]["count"] == 0).any()
    return exp


ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield request.param
    am.debug_set("AM_DFA", -1)


@pytest.mark.parametrize("seed", range(4))
def test_fragment_pool(route, seed):
    rng = random.Random(7300 + seed)
    seen_empty = 0
    for i in range(10):
        needles, hays = fragment_case(rng)
        if i % 3 == 0:
            needles = needles + [needles[0]]               # a needle listed twice: two handles, both count
        if i % 4 == 1:
            hays = hays + [""]
        if i % 5 == 2 and route != "table_walk" and "" not in needles:
            needles = needles + [""]                       # the empty needle: once per position
        if "" in needles or not any(needles):
            if route == "table_walk":
                continue                                   # the empty needle: no DFA section (the dense route reports those)
            seen_empty += 1
        for case in (0, 1):
            ns = [oracle.lower_utf8(x).decode() for x in needles] if (case and rng.random() < 0.8) else needles
            check_case(ns, hays, case, ROUTES[route])
    assert route == "table_walk" or seen_empty >= 1


def test_suffix_chains_and_handles(route):
    k = ROUTES[route]
    needles = ["tshirt", "shirts", "shirt", "hirt", "irt", "t"]
    hays = ["short tshirts and shirts", "", "tshirtshirtshirts TSHIRT", "hirt" * 50, "no needle here: zzz"]
    for case in (0, 1):
        offs, ents = check_case(needles, hays, case, k)
        assert offs[1] == offs[2] and int(offs[4]) == int(offs[5]) == len(ents)      # the empty haystack and the one without a needle: empty rows
        # the caller's own handles, some of them >= n_needles: skipped, they appear in no row
        offs, ents = check_case(needles, hays, case, k, values=[3, 900, 0, 4, 2 ** 32 - 1, 1], n=4)
        assert set(ents["needle"].tolist()) == {0, 1, 3}   # (handle 2 belongs to no needle)
        # the same handle for two needles: one entry whose count is the sum
        offs, ents = check_case(needles, hays, case, k, values=[0, 1, 0, 1, 2, 2], n=3)
        row3 = ents[int(offs[3]):int(offs[4])]
        assert row3["needle"].tolist() == [1, 2] and row3["count"].tolist() == [50, 100]      # "hirt" x 50: hirt -> 1; irt, t -> 2


def test_empty_shapes(route):
    a = am.Automaton(["ab", "b"])
    a.set_kernel(ROUTES[route])
    for case in (0, 1):
        for hays in ([], [""], ["", "", ""]):
            for got in all_forms(a, case, hays, 2):
                same(got, (np.zeros(len(hays) + 1, np.uint64), np.zeros(0, DT)), (case, hays))
        # first, last and several middle haystacks without a match: equal neighbouring offsets
        hays = ["zz", "ab", "", "q", "xx", "bab", "ab", "", "zzz"]
        exp = matrix_of_rows([((), ()), ((0, 1), (1, 1)), ((), ()), ((), ()), ((), ()), ((0, 1), (1, 2)), ((0, 1), (1, 1)), ((), ()), ((), ())])
        assert exp[0].tolist() == [0, 0, 2, 2, 2, 2, 4, 6, 6, 6]
        for got in all_forms(a, case, hays, 2):
            same(got, exp, case)
        # no values: n_hay empty rows
        for got in all_forms(a, case, hays, 0):
            same(got, (np.zeros(len(hays) + 1, np.uint64), np.zeros(0, DT)), case)


@pytest.mark.parametrize("pieces", [1, 4096])
def test_every_key_hot(route, pieces):
    """a, aa, aaa over 4 MiB of 'a': every add meets one of three keys per haystack.  A piece of L bytes has the row [(0, L), (1, L - 1), (2, L - 2)], zero counts absent."""
    n = 4 << 20
    text = np.full(n, ord("a"), np.uint8)
    cut = [n * i // pieces for i in range(pieces + 1)]
    if pieces > 1:
        cut[1:4] = [1, 3, 6]                               # pieces of 1, 2 and 3 bytes: one, two and three entries
    lens = [cut[i + 1] - cut[i] for i in range(pieces)]
    assert min(lens) >= 1 and sum(lens) == n
    exp = matrix_of_rows([(list(range(min(3, ln))), [ln - d for d in range(min(3, ln))]) for ln in lens])
    if pieces > 1:
        assert exp[0][:4].tolist() == [0, 1, 3, 6]
    hays = [text[cut[i]:cut[i + 1]] for i in range(pieces)]
    a = am.Automaton(["a", "aa", "aaa"])
    a.set_kernel(ROUTES[route])
    t = am.ValuesTable(a)
    same(t.count_matrix_texts(0, hays), exp)
    with Batch(hays) as b:
        same(t.count_matrix_batch(1, b), exp)
        m = C.c_void_p()
        am.api.check(am.api.libam().am_run_batch(a.device, 0, b, C.byref(m)))
        try:
            same(t.count_matrix(m, pieces), exp)
        finally:
            am.api.libam().am_matches_free(m)


def test_a_count_beyond_32_bits_in_one_entry():
    """300 needles "a" under handle 0 over 16 MiB of 'a': one row, one entry, 300 * 2^24 = 5 033 164 800.  This is where a 32-bit on-chip counter wraps."""
    n = 16 << 20
    o = oracle.Machine(["a"] * 300, [0] * 300)
    _, val = o.run_list(0, "aaaa")
    assert len(val) == 1200 and not val.any()
    a = am.Automaton(["a"] * 300, [0] * 300)
    exp = matrix_of_rows([([0], [300 * n])])
    assert int(exp[1]["count"][0]) == 5033164800
    hays = [np.full(n, ord("a"), np.uint8)]
    same(am.ValuesTable(a, 1).count_matrix_texts(0, hays), exp)
    same(a.count_matrix_host_mirror(1, hays, 1), exp)


@functools.lru_cache(maxsize=None)
def wide_needles():
    abc = "abcdefghijklmnopqrstuvwxyz0123456789"
    ns = ["".join(t) for t in itertools.islice(itertools.product(abc, repeat=3), 0, None, 5)][:9000]
    assert len(ns) == len(set(ns)) == 9000
    return ns


@pytest.mark.parametrize("case", [0, 1])
@pytest.mark.parametrize("limit", ["wave_row", "lds_row", "lds_slots"])
def test_row_widths_at_the_limits(limit, case):
    """Rows of C - 1, C, C + 1 and min(3C + 5, 9000) distinct needles for each limit C of the design, every wide row between two narrow rows and an empty one; and the
    same batch with the wide rows' needles in descending order in the text: the order of a row cannot come from the order of arrival."""
    ns = wide_needles()
    cap = LIMITS()[limit]
    rng = random.Random(cap + case)
    hays, rows = [], []
    for descending in (False, True):
        for k in (cap - 1, cap, cap + 1, min(3 * cap + 5, 9000)):
            ids = sorted(rng.sample(range(9000), k), reverse=descending)
            if k == 9000:
                assert len("|".join(ns)) == 35999
            hays += ["|" + ns[7] + "|", "|".join(ns[i] for i in ids), "", "||" + ns[8999] + "|" + ns[3]]
            rows += [([7], [1]), (sorted(ids), [1] * k), ((), ()), ([3, 8999], [1, 1])]
    exp = matrix_of_rows(rows)
    a = am.Automaton(ns)
    t = am.ValuesTable(a)
    if limit == "wave_row" and case == 0:                  # the expectation is arithmetic; the oracle agrees with it
        same(oracle_matrix(oracle.Machine(ns), 0, hays[:8], 9000), matrix_of_rows(rows[:8]))
    if case:
        hays = [h.upper() for h in hays]
    with Batch(hays) as b:
        same(t.count_matrix_batch(case, b), exp, (limit, case))
    same(t.count_matrix_texts(case, hays), exp, (limit, case))


@pytest.mark.parametrize("case", [0, 1])
def test_many_tiny_rows(case):
    """20 000 haystacks of 0-40 bytes: more rows than a tile has records, tiles that span dozens of haystacks, empty rows everywhere."""
    rng = random.Random(20000)
    hays = ["".join(rng.choice("ab1 \n") for _ in range(rng.randrange(41))) for _ in range(20000)]
    ns = ["ab", "b", "a1", "12", "AB"]
    exp = oracle_matrix(oracle.Machine(ns), case, hays, len(ns))
    assert (np.diff(exp[0].astype(np.int64)) == 0).sum() > 500 and len(exp[1]) > 30000
    a = am.Automaton(ns)
    for form, got in enumerate(all_forms(a, case, hays, len(ns))):
        same(got, exp, form)


@functools.lru_cache(maxsize=None)
def natural_reduced():
    """The natural workload at the size test_synthetic_workload_reduced uses (1 MiB in 100-KiB haystacks), IgnoreCase, with the oracle's matrix."""
    w = synth.WORKLOADS["natural_100k_10GiB"]
    needles = synth.needles_for("natural_100k_10GiB")
    n_cells, hay_cells = 1024, 100
    text = synth.haystacks_host(needles, w["mixed"], 0, n_cells, natural=bool(w.get("natural")))
    hays = [text[i * hay_cells * 1024:(i + 1) * hay_cells * 1024] for i in range(n_cells // hay_cells)]
    o = oracle.Machine(needles)
    return needles, hays, o, oracle_matrix(o, am.IGNORE_CASE, hays, len(needles))


@functools.lru_cache(maxsize=None)
def natural_split():
    """... its first haystack cut at byte 33 333: a group's text does not start on a 16-byte boundary of the batch."""
    needles, hays, o, _ = natural_reduced()
    hays = [hays[0][:33333], hays[0][33333:]] + hays[1:]
    return hays, oracle_matrix(o, am.IGNORE_CASE, hays, len(needles))


def identities(a, t, case, b, got):
    """matrix summed over its rows = am_count_by_needle_batch; row sums = am_count_batch (every handle is < n)."""
    offs, ents = got
    n_hay = len(offs) - 1
    by_needle = np.zeros(t.n_needles, np.uint64)
    np.add.at(by_needle, ents["needle"], ents["count"])
    assert np.array_equal(by_needle, t.count_by_needle_batch(case, b))
    per = np.zeros(max(n_hay, 1), np.uint64)
    am.api.check(am.api.libam().am_count_batch(a.device, case, b, per.ctypes.data, None))
    rows = np.zeros(n_hay, np.uint64)
    np.add.at(rows, ents["haystack"], ents["count"])
    assert np.array_equal(rows, per[:n_hay])


def test_natural_text_and_its_lines():
    needles, hays, o, exp = natural_reduced()
    assert len(exp[1]) > 1000 and int(exp[1]["count"].max()) > 50      # many entries, a few of them hot
    a = am.Automaton(needles)
    t = am.ValuesTable(a)
    for k in (0, 2):
        a.set_kernel(k)
        with Batch(hays) as b:
            got = t.count_matrix_batch(am.IGNORE_CASE, b)
            same(got, exp, k)
            identities(a, t, am.IGNORE_CASE, b, got)
    a.set_kernel(0)
    same(a.count_matrix(am.IGNORE_CASE, hays), exp)
    # document -> lines -> matrix, without leaving HBM
    sp = am.Splitter("\n")
    docs = [bytes(d).replace(b". ", b".\n") for d in hays[:3]]      # (synth's text has no line ends of its own: the blank after every full stop becomes one)
    lines = [ln for d in docs for ln in d.split(b"\n")]
    assert len(lines) > 1000
    exp_lines = oracle_matrix(o, am.IGNORE_CASE, lines, len(needles))
    with Batch(docs) as b:
        lb, doc_offs = sp.lines_batch(b)
        try:
            assert int(doc_offs[-1]) == len(lines)
            got = t.count_matrix_batch(am.IGNORE_CASE, lb)
            same(got, exp_lines)
            identities(a, t, am.IGNORE_CASE, lb, got)
        finally:
            am.api.libam().am_batch_destroy(lb)


def fold_launches(fn):
    """(result of fn(), launches of k_mx_combine it made)"""
    lib = am.api.libam()
    am.api.check(lib.am_profile_enable(1))
    am.api.check(lib.am_profile_reset())
    try:
        r = fn()
        ms, n = C.c_double(0), C.c_uint64(0)
        am.api.check(lib.am_profile_read(b"mx_combine", C.byref(ms), C.byref(n)))
    finally:
        lib.am_profile_enable(0)
    return r, int(n.value)


def test_bounded_record_memory():
    """AM_HIST_RECORDS_MIB = 1: 65 536 records in HBM at a time: the batch is counted and then scanned in groups of whole haystacks, a group's rows appended to the
    result with the haystack index and the offsets rebased.  The middle haystack alone is over the budget: a group of one, scanned whole."""
    lens = [1, 0, 30000, 7, 25000, 12000, 200000, 3, 40000, 0, 21845, 21846, 9]
    hays = []
    for i, ln in enumerate(lens):
        h = np.full(ln, ord("a"), np.uint8)
        if i in (3, 8):
            h[:] = ord("b")                                # no needle in these
        hays.append(h)
    exp = matrix_of_rows([((), ()) if i in (3, 8) else (list(range(min(3, ln))), [ln - d for d in range(min(3, ln))]) for i, ln in enumerate(lens)])
    a = am.Automaton(["a", "aa", "aaa"])
    t = am.ValuesTable(a)
    with Batch(hays) as b:
        free, n_free = fold_launches(lambda: t.count_matrix_batch(0, b))
        am.debug_set("AM_HIST_RECORDS_MIB", 1)
        forced, n_forced = fold_launches(lambda: t.count_matrix_batch(0, b))
        am.debug_set("AM_HIST_RECORDS_MIB", -1)
    same(free, exp)
    same(forced, exp)
    assert forced[1]["haystack"].tolist() == sorted(forced[1]["haystack"].tolist()) and int(forced[1]["haystack"][-1]) == 12      # across the seams
    assert n_free == 1 and n_forced >= 5, (n_free, n_forced)
    needles, _, _, _ = natural_reduced()
    hays, exp = natural_split()
    a = am.Automaton(needles)
    t = am.ValuesTable(a)
    with Batch(hays) as b:
        free = t.count_matrix_batch(am.IGNORE_CASE, b)
        am.debug_set("AM_HIST_RECORDS_MIB", 1)
        forced, n_forced = fold_launches(lambda: t.count_matrix_batch(am.IGNORE_CASE, b))
    same(free, exp)
    same(forced, exp)
    assert n_forced >= 3, n_forced


@pytest.mark.parametrize("segment_kib", [16, 250])
def test_one_shot_form_in_segments(segment_kib):
    """AM_RUN_SEGMENTS = k: host slices go up in segments of k KiB (whole haystacks); a segment's rows are built in HBM while the next goes up, and appended."""
    needles, _, _, _ = natural_reduced()
    hays, exp = natural_split()
    a = am.Automaton(needles)
    t = am.ValuesTable(a)
    with Batch(hays) as b:
        in_one = t.count_matrix_batch(am.IGNORE_CASE, b)
    am.debug_set("AM_RUN_SEGMENTS", segment_kib)
    got, launches = fold_launches(lambda: t.count_matrix_texts(am.IGNORE_CASE, hays))
    same(got, in_one)
    same(got, exp)
    assert launches >= 3, launches
    if segment_kib != 16:
        return
    # small texts, several per segment; empty ones among them
    rng = random.Random(99)
    small = []
    for _ in range(40):
        small += fragment_case(rng, allow_empty_needle=False)[1]
    ns = ["ab", "b", "a1", "12", "AB"]
    am.debug_set("AM_RUN_SEGMENTS", 1)
    for case in (0, 1):
        same(am.Automaton(ns).count_matrix(case, small), oracle_matrix(oracle.Machine(ns), case, small, len(ns)), case)


def test_held_results():
    lib = am.api.libam()
    needles, _, _, _ = natural_reduced()
    hays, exp = natural_split()
    a = am.Automaton(needles)
    t = am.ValuesTable(a)
    with Batch(hays) as b:
        m = C.c_void_p()
        am.api.check(lib.am_run_batch(a.device, am.IGNORE_CASE, b, C.byref(m)))
        try:
            assert lib.am_matches_device_data(m)
            same(t.count_matrix(m, len(hays)), exp)
            more = t.count_matrix(m, len(hays) + 2)        # haystacks the result does not know: empty rows
            assert more[0].tolist() == exp[0].tolist() + [int(exp[0][-1])] * 2 and more[1].tobytes() == exp[1].tobytes()
            x = C.c_void_p(5)
            assert lib.am_matches_count_matrix(m, t.handle, len(hays) - 1, C.byref(x)) == am.AM_ERR_INVALID and x.value is None
            assert b"n_hay" in lib.am_last_error()
        finally:
            lib.am_matches_free(m)
    # a result assembled on the host (am_run in segments: AM_RUN_SEGMENTS = k > 0 forces them, k KiB each) has no records in HBM
    am.debug_set("AM_RUN_SEGMENTS", 64)
    s = am.api._Slices(hays)
    m = C.c_void_p()
    am.api.check(lib.am_run(a.device, am.IGNORE_CASE, s.arr, s.n, C.byref(m)))
    try:
        assert lib.am_matches_size(m) > 0 and not lib.am_matches_device_data(m)
        x = C.c_void_p(5)
        assert lib.am_matches_count_matrix(m, t.handle, len(hays), C.byref(x)) == am.AM_ERR_UNSUPPORTED
        msg = lib.am_last_error()
        assert b"am_matches_count_matrix" in msg and b"assembled on the host" in msg and x.value is None
    finally:
        lib.am_matches_free(m)


def test_two_runs_give_the_same_bytes():
    needles, hays, _, exp = natural_reduced()
    a = am.Automaton(needles)
    t = am.ValuesTable(a)
    with Batch(hays) as b:
        one = t.count_matrix_batch(am.IGNORE_CASE, b)
        two = t.count_matrix_batch(am.IGNORE_CASE, b)
        x = t.count_matrix_batch(am.IGNORE_CASE, b, raw=True)      # the raw handle: the result stays in HBM
        try:
            assert am.api.libam().am_needle_matrix_device_offsets(x) and am.api.libam().am_needle_matrix_device_data(x)
            assert am.api.libam().am_needle_matrix_size(x) == len(exp[1]) and am.api.libam().am_needle_matrix_haystacks(x) == len(hays)
        finally:
            am.api.libam().am_needle_matrix_free(x)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
    same(one, exp)
