"""am_count_by_needle* on the device against the oracle: counts[v] = how often the reference's runWithCase (Automaton.hs:442-553) hands `Match _ v` to its fold
function over the whole batch.  Expected values are np.bincount over oracle.Machine.run_list, or arithmetic; never another path of the library."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from alfred_margaret_amd import synth
from oracle import oracle
from tests.helpers import fragment_case

pytestmark = pytest.mark.gpu


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


def oracle_counts(o, case, hays, n):
    out = np.zeros(n, np.uint64)
    for h in hays:
        _, val = o.run_list(case, h)
        v = val[val < n].astype(np.int64)
        out += np.bincount(v, minlength=n).astype(np.uint64)
    return out


def batch_total(a, case, b):
    total = C.c_uint64(0)
    am.api.check(am.api.libam().am_count_batch(a.device, case, b, None, C.byref(total)))
    return int(total.value)


def all_forms(a, case, hays, n):
    """The one-shot form, the batch form, the fold over a held am_run_batch result and the host mirror: four vectors that must be one."""
    lib = am.api.libam()
    t = am.ValuesTable(a, n)
    got = [t.count_by_needle_texts(case, hays)]
    with Batch(hays) as b:
        got.append(t.count_by_needle_batch(case, b))
        m = C.c_void_p()
        am.api.check(lib.am_run_batch(a.device, case, b, C.byref(m)))
        try:
            got.append(t.count_by_needle(m))
        finally:
            lib.am_matches_free(m)
    got.append(a.count_by_needle_host_mirror(case, hays, n))
    return got


def check_case(needles, hays, case, kernel, values=None, n=None):
    n = len(needles) if n is None else n
    o = oracle.Machine(needles, values)
    exp = oracle_counts(o, case, hays, n)
    a = am.Automaton(needles, values)
    a.set_kernel(kernel)
    for form, got in enumerate(all_forms(a, case, hays, n)):
        assert got.dtype == np.uint64 and got.tolist() == exp.tolist(), (form, kernel, case, needles, hays, values, n)
    if values is None:                                     # every handle is < n: the count identity (benchmark/haskell/app/Main.hs:67-76)
        assert int(exp.sum()) == sum(o.count_matches(case, h) for h in hays)
    return exp


ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield request.param
    am.debug_set("AM_DFA", -1)


@pytest.mark.parametrize("seed", range(4))
def test_fragment_pool_needle_counts(route, seed):
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


def test_suffix_chains_and_handles_beyond_the_table(route):
    k = ROUTES[route]
    needles = ["tshirt", "shirts", "shirt", "hirt", "irt", "t"]
    hays = ["short tshirts and shirts", "", "tshirtshirtshirts TSHIRT", "hirt" * 50, "no needle here: zzz"]
    for case in (0, 1):
        exp = check_case(needles, hays, case, k)
        assert exp[5] > exp[0] > 0                         # states with several values: every value of a list counts
        # the caller's own handles, some of them >= n_needles: skipped
        values = [3, 900, 0, 4, 2 ** 32 - 1, 1]
        exp = check_case(needles, hays, case, k, values=values, n=4)
        assert exp[1] > 0 and exp[2] == 0                  # (handle 2 belongs to no needle)
        # the same handle for two needles: their counts add up
        check_case(needles, hays, case, k, values=[0, 1, 0, 1, 2, 2], n=3)


def test_empty_batches(route):
    a = am.Automaton(["ab", "b"])
    a.set_kernel(ROUTES[route])
    for case in (0, 1):
        for hays in ([], [""], ["", "", ""]):
            for got in all_forms(a, case, hays, 2):
                assert got.tolist() == [0, 0], (case, hays)


@pytest.mark.parametrize("pieces", [1, 4096])
def test_every_id_hot(route, pieces):
    """a, aa, aaa over 16 MiB of 'a': every add of every workgroup meets one of three ids.  A piece of L bytes holds L, L - 1, L - 2 of them."""
    n = 16 << 20
    text = np.full(n, ord("a"), np.uint8)
    cut = [n * i // pieces for i in range(pieces + 1)]
    hays = [text[cut[i]:cut[i + 1]] for i in range(pieces)]
    exp = [sum(max(0, (cut[i + 1] - cut[i]) - d) for i in range(pieces)) for d in range(3)]
    if pieces == 1:
        assert exp == [n, n - 1, n - 2]
    a = am.Automaton(["a", "aa", "aaa"])
    a.set_kernel(ROUTES[route])
    t = am.ValuesTable(a)
    assert t.count_by_needle_texts(0, hays).tolist() == exp
    with Batch(hays) as b:
        assert t.count_by_needle_batch(1, b).tolist() == exp


@functools.lru_cache(maxsize=None)
def natural_reduced():
    """The natural workload at the size test_synthetic_workload_reduced uses (1 MiB in 100-KiB haystacks), IgnoreCase, with the oracle's counts."""
    w = synth.WORKLOADS["natural_100k_10GiB"]
    needles = synth.needles_for("natural_100k_10GiB")
    n_cells, hay_cells = 1024, 100
    text = synth.haystacks_host(needles, w["mixed"], 0, n_cells, natural=bool(w.get("natural")))
    hays = [text[i * hay_cells * 1024:(i + 1) * hay_cells * 1024] for i in range(n_cells // hay_cells)]
    exp = oracle_counts(oracle.Machine(needles), am.IGNORE_CASE, hays, len(needles))
    return needles, hays, exp


def test_zipf_text_against_the_oracle():
    needles, hays, exp = natural_reduced()
    assert int(exp.sum()) > 100000 and int(exp.max()) > 50 * int(np.median(exp[exp > 0]))      # skewed: a few ids take most adds
    a = am.Automaton(needles)
    t = am.ValuesTable(a)
    for k in (0, 2):
        a.set_kernel(k)
        with Batch(hays) as b:
            got = t.count_by_needle_batch(am.IGNORE_CASE, b)
            assert np.array_equal(got, exp), k
            assert int(got.sum()) == batch_total(a, am.IGNORE_CASE, b)
    assert np.array_equal(a.count_by_needle(am.IGNORE_CASE, hays), exp)


def hist_launches(fn):
    """(result of fn(), launches of k_needle_hist it made)"""
    lib = am.api.libam()
    am.api.check(lib.am_profile_enable(1))
    am.api.check(lib.am_profile_reset())
    try:
        r = fn()
        ms, n = C.c_double(0), C.c_uint64(0)
        am.api.check(lib.am_profile_read(b"needle_hist", C.byref(ms), C.byref(n)))
    finally:
        lib.am_profile_enable(0)
    return r, int(n.value)


def test_groups_of_haystacks_give_the_same_counts():
    """AM_HIST_RECORDS_MIB = 1: 65 536 records in HBM at a time, so the batch is counted and then scanned in groups of whole haystacks.  The middle haystack alone
    is over the budget (200 000 bytes of 'a' = 600 000 values): a group of one, scanned whole.  Haystacks without a match are not scanned again."""
    lens = [1, 0, 30000, 7, 25000, 12000, 200000, 3, 40000, 0, 21845, 21846, 9]
    hays = []
    for i, ln in enumerate(lens):
        h = np.full(ln, ord("a"), np.uint8)
        if i in (3, 8):
            h[:] = ord("b")                                # no needle in these
        hays.append(h)
    exp = [sum(max(0, ln - d) for i, ln in enumerate(lens) if i not in (3, 8)) for d in range(3)]
    a = am.Automaton(["a", "aa", "aaa"])
    t = am.ValuesTable(a)
    with Batch(hays) as b:
        free, n_free = hist_launches(lambda: t.count_by_needle_batch(0, b))
        am.debug_set("AM_HIST_RECORDS_MIB", 1)
        forced, n_forced = hist_launches(lambda: t.count_by_needle_batch(0, b))
        am.debug_set("AM_HIST_RECORDS_MIB", -1)
    assert free.tolist() == exp and forced.tolist() == exp
    assert n_free == 1 and n_forced >= 5, (n_free, n_forced)
    # natural text, where a group's text does not start on a 16-byte boundary of the batch
    needles, hays, _ = natural_reduced()
    hays = [hays[0][:33333], hays[0][33333:]] + hays[1:]
    exp = oracle_counts(oracle.Machine(needles), am.IGNORE_CASE, hays, len(needles))
    a = am.Automaton(needles)
    t = am.ValuesTable(a)
    with Batch(hays) as b:
        free = t.count_by_needle_batch(am.IGNORE_CASE, b)
        am.debug_set("AM_HIST_RECORDS_MIB", 1)
        forced, n_forced = hist_launches(lambda: t.count_by_needle_batch(am.IGNORE_CASE, b))
    assert np.array_equal(free, exp) and np.array_equal(forced, exp) and n_forced >= 3, n_forced


def test_fold_over_a_held_result():
    lib = am.api.libam()
    needles, hays, exp = natural_reduced()
    a = am.Automaton(needles)
    t = am.ValuesTable(a)
    with Batch(hays) as b:
        m = C.c_void_p()
        am.api.check(lib.am_run_batch(a.device, am.IGNORE_CASE, b, C.byref(m)))
        try:
            assert lib.am_matches_device_data(m)
            assert np.array_equal(t.count_by_needle(m), exp)
        finally:
            lib.am_matches_free(m)
    # a result assembled on the host (am_run in segments: AM_RUN_SEGMENTS = k > 0 forces them, k KiB each) has no records in HBM
    am.debug_set("AM_RUN_SEGMENTS", 64)
    s = am.api._Slices(hays)
    m = C.c_void_p()
    am.api.check(lib.am_run(a.device, am.IGNORE_CASE, s.arr, s.n, C.byref(m)))
    try:
        assert lib.am_matches_size(m) > 0 and not lib.am_matches_device_data(m)
        out = np.zeros(len(needles), np.uint64)
        assert lib.am_matches_count_by_needle(m, t.handle, out.ctypes.data) == am.AM_ERR_UNSUPPORTED
        msg = lib.am_last_error()
        assert b"am_matches_count_by_needle" in msg and b"assembled on the host" in msg and not out.any()
    finally:
        lib.am_matches_free(m)


@pytest.mark.parametrize("segment_kib", [16, 250])
def test_one_shot_form_in_segments(segment_kib):
    """AM_RUN_SEGMENTS = k: host slices go up in segments of k KiB (whole haystacks), folded in HBM while the next is uploaded."""
    needles, hays, exp = natural_reduced()
    a = am.Automaton(needles)
    t = am.ValuesTable(a)
    with Batch(hays) as b:
        in_one = t.count_by_needle_batch(am.IGNORE_CASE, b)
    am.debug_set("AM_RUN_SEGMENTS", segment_kib)
    got, launches = hist_launches(lambda: t.count_by_needle_texts(am.IGNORE_CASE, hays))
    assert np.array_equal(got, in_one) and np.array_equal(got, exp)
    assert launches >= 3, launches
    # small texts, several per segment; empty ones among them
    rng = random.Random(99)
    small = []
    for _ in range(40):
        small += fragment_case(rng, allow_empty_needle=False)[1]
    ns = ["ab", "b", "a1", "12", "AB"]
    am.debug_set("AM_RUN_SEGMENTS", 1)
    for case in (0, 1):
        assert am.Automaton(ns).count_by_needle(case, small).tolist() == oracle_counts(oracle.Machine(ns), case, small, len(ns)).tolist()


def test_periodic_flush_of_the_lds_counts():
    """AM_HIST_FLUSH_TILES = 1: every workgroup of k_needle_hist flushes and clears its LDS counts after every tile (by itself: after 2 048 tiles, which no
    test-sized batch reaches), with the hot ids keeping their slots across the flushes.  The counts are the same."""
    n = 4 << 20
    hays = [np.full(n, ord("a"), np.uint8)]
    a = am.Automaton(["a", "aa", "aaa"])
    t = am.ValuesTable(a)
    am.debug_set("AM_HIST_FLUSH_TILES", 1)
    assert t.count_by_needle_texts(0, hays).tolist() == [n, n - 1, n - 2]
    needles, hays, exp = natural_reduced()
    a = am.Automaton(needles)
    for tiles in (1, 3):
        am.debug_set("AM_HIST_FLUSH_TILES", tiles)
        assert np.array_equal(a.count_by_needle(am.IGNORE_CASE, hays), exp), tiles


def test_a_state_with_more_values_than_a_record_adds_to_lds(route):
    """1 100 copies of one needle under distinct handles: its state's list is longer than the 1 024 values a record may add to a workgroup's LDS table, the rest go
    to HBM directly.  Every handle counts every occurrence."""
    needles = ["ab"] * 1100 + ["b", "abab"]
    hays = ["abab" * 300, "", "xxabx", "b" * 77]
    for case in (0, 1):
        exp = check_case(needles, hays, case, ROUTES[route])
        assert exp[0] == exp[1099] == 601 and exp[1100] == 678 and exp[1101] == 599
