"""Scores on the device (am_weights_* / am_score* / am_scores_top_k / am_select_top_k / am_select_score, csrc/am_score.hip) against the definition.  Every check
compares every score with what tests/score_reference.py says -- built over the oracle's fold and Python integers, or arithmetic where a haystack is a run of one
letter -- never with another path of the library.  Shapes sit on the real seams: the 64 records a wavefront of the fold takes at a time, the records it owns in a
tile, the tile, and the block of the top-k histogram (am_score_geometry)."""
import ctypes as C
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import score_reference as ref, words_reference as wref
from tests.helpers import fragment_case
from tests.test_gpu_select import Batch, check_texts, lib, lowered, pool_case

pytestmark = pytest.mark.gpu

ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}
KELVIN, ANGSTROM = "\u212a", "\u212b"                    # lower-case to k and å: the byte length changes
A3 = ["a", "aa", "aaa"]                                    # value lists of 1 to 3 over a run of a's
A3_WEIGHTS = [[1, 10, 100], [2 ** 62, 1, 0], [-1, 0, ref.INT64_MIN]]


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield request.param
    am.debug_set("AM_DFA", -1)


class Scorer:
    """An automaton on a route with its values table; weights over it."""

    def __init__(self, needles, route="default", values=None, n=None):
        self.a = am.Automaton(needles, values)
        self.a.set_kernel(ROUTES[route])
        self.n = len(needles) if n is None else n
        self.t = am.ValuesTable(self.a, self.n)

    def weights(self, cols):
        return am.Weights(self.t, cols)


def run_matches(a, case, b):
    m = C.c_void_p()
    am.api.check(lib().am_run_batch(a.device, case, b, C.byref(m)))
    return m


def all_forms(sc, case, hays, cols):
    """The one-shot form, the batch form, the fold over a held am_run_batch result and the host mirror: four arrays that must be one."""
    w = sc.weights(cols)
    got = [w.score_texts(case, hays).scores]
    with Batch(hays) as b:
        x = w.score_batch(case, b)
        assert (x.n_cols, x.n_hay) == (len(cols), len(hays)) and bool(lib().am_scores_device_data(x.handle)) == (len(hays) > 0)
        got.append(x.scores)
        m = run_matches(sc.a, case, b)
        try:
            got.append(w.score_matches(m, len(hays)).scores)
        finally:
            lib().am_matches_free(m)
    got.append(sc.a.score_host_mirror(case, hays, cols, sc.n))
    return got


def check_forms(sc, case, hays, cols, exp, what=None):
    for form, got in enumerate(all_forms(sc, case, hays, cols)):
        assert got.dtype == np.int64 and got.shape == exp.shape, (what, form)
        if not np.array_equal(got, exp):
            c, h = np.argwhere(got != exp)[0]
            raise AssertionError((what, "form", form, "column", int(c), "haystack", int(h), int(got[c, h]), int(exp[c, h])))


def a3_scores(lens, cols=A3_WEIGHTS):
    """The scores of a, aa, aaa over runs of `lens` a's (a run of L holds L, L - 1, L - 2 of them); -1: a haystack of b's, nothing."""
    out = np.zeros((len(cols), len(lens)), np.int64)
    for i, ln in enumerate(lens):
        for c, col in enumerate(cols):
            out[c, i] = ref.wrap(sum(max(0, ln - d) * col[d] for d in range(3)))
    return out


def a3_hays(lens):
    return [np.full(abs(ln), ord("a") if ln >= 0 else ord("b"), np.uint8) for ln in lens]


# ---- 1. fragment pools: four forms, three routes, both case modes

@pytest.mark.parametrize("seed", range(4))
def test_fragment_pool_scores(route, seed):
    rng = random.Random(7400 + seed)
    seen_empty = 0
    for i in range(10):
        needles, hays = fragment_case(rng)
        if i % 3 == 0:
            needles = needles + [needles[0]]               # a needle listed twice: two handles, both add
        if i % 4 == 1:
            hays = hays + [""]
        if i % 5 == 2 and route != "table_walk" and "" not in needles:
            needles = needles + [""]                       # the empty needle: once per position
        if "" in needles or not any(needles):
            if route == "table_walk":
                continue                                   # the empty needle: no DFA section (the dense route reports those)
            seen_empty += 1
        values, n = None, len(needles)
        if i % 4 == 2:                                     # handles of the caller's own: two needles under one, some beyond the table
            n = max(1, len(needles) - 2)
            values = [rng.randrange(n + 2) for _ in needles]
            values[0] = values[-1] = 0
        cols = ref.random_weights(rng, n, (1, 3, 8)[i % 3])
        for case in (0, 1):
            ns = lowered(needles) if (case and rng.random() < 0.8) else needles
            check_forms(Scorer(ns, route, values, n), case, hays, cols, ref.expect(ns, values, n, case, cols, hays), (seed, i, case, ns, values, hays))
    assert route == "table_walk" or seen_empty >= 1


def test_suffix_chains_and_degenerate_sizes(route):
    needles = ["tshirt", "shirts", "shirt", "hirt", "irt", "t"]
    hays = ["short tshirts and shirts", "", "tshirtshirtshirts TSHIRT", "hirt" * 50, "no needle here: zzz"]
    cols = [[1, 1, 1, 1, 1, 1], [3, -5, 2 ** 40, 7, -2 ** 62, 11]]
    for case in (0, 1):
        exp = ref.expect(needles, None, 6, case, cols, hays)
        assert exp[0, 2] > 6                               # states with several values: every value of a list adds
        check_forms(Scorer(needles, route), case, hays, cols, exp, case)
        # a column of ones, every handle below n: am_count_batch's counts
        o = oracle.Machine(needles)
        assert exp[0].tolist() == [o.count_matches(case, h) for h in hays]
    # no value handle at all: all-zero scores; no haystacks: an empty result
    sc = Scorer(needles, route, n=0)
    for got in all_forms(sc, 0, hays, [[], []]):
        assert got.shape == (2, 5) and not got.any()
    sc = Scorer(needles, route)
    w = sc.weights(cols)
    assert w.score_texts(0, []).scores.shape == (2, 0)
    with Batch([]) as b:
        x = w.score_batch(1, b)
        assert x.scores.shape == (2, 0) and x.n_hay == 0 and not lib().am_scores_device_data(x.handle)
        assert x.top_k(3).size == 0 and x.select_top_k(3, batch=b).size == 0 and x.select(0, 0, batch=b).size == 0
    for got in all_forms(sc, 1, ["", "", ""], cols):
        assert got.shape == (2, 3) and not got.any()


# ---- 2. run seams: where a run of equal haystacks ends among the 64 records of a step, the records of a wavefront, the tile

def seam_patterns():
    tile, _ = am.api.score_geometry()
    wave = tile // 4
    return {
        "step": [63, 1, 64, 64, 65, 63, 2, 1, 1, 62, 130, 61, 3],                       # runs that end at record 63 / 64 / 65 of a step and of a wavefront's first step
        "wavefront": [wave - 1, 1, wave, wave + 1, wave - 2, 3, 2 * wave - 1, 2, 1],    # ... of the records a wavefront owns
        "tile": [tile - 1, 1, tile, tile + 1, tile - 2, 3, 2 * tile - 1, 2, 1, 7],      # ... of a tile
        "three tiles": [5, 3 * tile + 17, 9, 2 * tile, 1],                               # a run through three tiles, a run of exactly two
        "every lane": [1] * (2 * tile),                                                  # every lane its own run
        "gaps": [0, -5, 3, 0, 0, -2, 70, -1, 64, 0, -300, 1, 0, 2 * tile + 3, -9, 0],    # no match in between, empty ones, the first and the last empty
        "one record": [1],
        "short": [2, 0, 1],
    }


@pytest.mark.parametrize("pattern", sorted(seam_patterns()))
def test_run_seams(route, pattern):
    lens = seam_patterns()[pattern]
    hays = a3_hays(lens)
    exp = a3_scores([max(ln, 0) for ln in lens])
    if sum(abs(ln) for ln in lens) < 3000:                  # the arithmetic is the oracle's
        assert np.array_equal(exp, ref.expect(A3, None, 3, 0, A3_WEIGHTS, [bytes(h) for h in hays]))
    sc = Scorer(A3, route)
    for case in (0, 1):
        check_forms(sc, case, hays, A3_WEIGHTS, exp, (pattern, case))
    one = [[1, 10, 100]]
    check_forms(sc, 0, hays, one, exp[:1], (pattern, "one column"))


@pytest.mark.parametrize("n_cols", [2, 4, 5, 7])
def test_column_counts_on_both_sides_of_an_instantiation(n_cols):
    """k_score is compiled for 1, 4 and 8 columns and launched with the smallest that holds the weights: the last count of one and the first of the next, every
    column with weights of its own, over runs that end inside a step, at a wavefront's records and at a tile."""
    tile, _ = am.api.score_geometry()
    cols = [[c + 1, 10 ** c, -(7 ** c) - c] for c in range(n_cols)]
    lens = [63, 1, 64, 65, tile // 4 + 1, 0, tile - 1, 1, tile + 1, -4, 2]
    exp = a3_scores([max(ln, 0) for ln in lens], cols)
    assert len(set(map(tuple, exp.tolist()))) == n_cols                  # no two columns alike: a column read for another one shows
    sc = Scorer(A3)
    for case in (0, 1):
        check_forms(sc, case, a3_hays(lens), cols, exp, (n_cols, case))


def test_one_document_through_every_workgroup(route):
    """One haystack of 3 MiB of a's: three million records of one run, several tiles for every workgroup of the persistent grid; a second haystack behind it."""
    lens = [3 << 20, 5]
    hays = a3_hays(lens)
    exp = a3_scores(lens)
    w = Scorer(A3, route).weights(A3_WEIGHTS)
    with Batch(hays) as b:
        assert np.array_equal(w.score_batch(0, b).scores, exp)
        assert np.array_equal(w.score_batch(1, b).scores, exp)


# ---- 3. the wrap

def test_sums_wrap_modulo_two_to_the_64(route):
    sc = Scorer(["a"], route)
    cols = [[2 ** 62], [ref.INT64_MIN], [ref.INT64_MAX]]
    hays = ["aaaaa", "aa", "a", ""]
    exp = np.asarray([[2 ** 62, ref.INT64_MIN, 2 ** 62, 0], [ref.INT64_MIN, 0, ref.INT64_MIN, 0], [ref.wrap(5 * ref.INT64_MAX), -2, ref.INT64_MAX, 0]], np.int64)
    assert np.array_equal(exp, ref.expect(["a"], None, 1, 0, cols, hays))
    for case in (0, 1):
        check_forms(sc, case, hays, cols, exp, case)


# ---- 4. groups of bounded record memory, segments of the upload

def launches(name, fn):
    """(result of fn(), launches of the kernel `name` it made)"""
    am.api.check(lib().am_profile_enable(1))
    am.api.check(lib().am_profile_reset())
    try:
        r = fn()
        ms, n = C.c_double(0), C.c_uint64(0)
        am.api.check(lib().am_profile_read(name, C.byref(ms), C.byref(n)))
    finally:
        lib().am_profile_enable(0)
    return r, int(n.value)


def test_groups_and_segments_give_the_same_scores():
    """AM_HIST_RECORDS_MIB = 1: 65 536 records in HBM at a time, so a batch of about 160 000 records in 40 haystacks is counted and then scanned in groups of whole
    haystacks, and a group's scores land at its first haystack.  AM_RUN_SEGMENTS = 16: the one-shot form goes up in segments of 16 KiB."""
    rng = random.Random(41)
    needles = ["a", "ab", "ba", "aab", "bb"]
    hays = ["".join(rng.choice("ab") for _ in range(rng.randint(2500, 5500))) for _ in range(40)]
    hays[7] = ""
    hays[8] = "c" * 3000                                   # no needle: not scanned again
    hays[23] = "a" * 9000
    cols = ref.random_weights(rng, len(needles), 3)
    exp = ref.expect(needles, None, len(needles), 0, cols, hays)
    sc = Scorer(needles)
    w = sc.weights(cols)
    with Batch(hays) as b:
        free, n_free = launches(b"score", lambda: w.score_batch(0, b).scores)
        am.debug_set("AM_HIST_RECORDS_MIB", 1)
        forced, n_forced = launches(b"score", lambda: w.score_batch(0, b).scores)
        am.debug_set("AM_HIST_RECORDS_MIB", -1)
    assert np.array_equal(free, exp) and np.array_equal(forced, exp)
    assert n_free == 1 and n_forced >= 3, (n_free, n_forced)
    am.debug_set("AM_RUN_SEGMENTS", 16)
    seg, n_seg = launches(b"score", lambda: w.score_texts(0, hays).scores)
    assert np.array_equal(seg, exp) and n_seg >= 3, n_seg
    am.debug_set("AM_HIST_RECORDS_MIB", 1)                  # segments, and groups inside a segment
    am.debug_set("AM_RUN_SEGMENTS", 64)
    assert np.array_equal(w.score_texts(0, hays).scores, exp)
    am.debug_set("AM_RUN_SEGMENTS", -1)
    # the whole-word form in groups: the predicate reads the group's own text and offsets
    t = am.SpanTable(sc.a, word_bytes=b"b")
    ww = am.Weights(t.values, cols)
    some = hays[:24]
    expw = ref.expect_words(needles, len(needles), 0, cols, some, frozenset(b"b"))
    with Batch(some) as b:
        got, n_words = launches(b"score_words", lambda: t.score_batch(0, b, ww).scores)
    assert np.array_equal(got, expw) and n_words >= 2 and not np.array_equal(expw, exp[:, :24])
    # small texts, several per segment; empty ones among them
    small = []
    for _ in range(40):
        small += fragment_case(rng, allow_empty_needle=False)[1]
    ns = ["ab", "b", "a1", "12", "AB"]
    am.debug_set("AM_RUN_SEGMENTS", 1)
    for case in (0, 1):
        assert np.array_equal(am.Automaton(ns).score(case, small, [[1, 2, 3, 4, 5]]), ref.expect(ns, None, 5, case, [[1, 2, 3, 4, 5]], small))


# ---- 5. whole words

def check_words(needles, hays, cls, route, cases=(0, 1), n_cols=3, seed=0):
    rng = random.Random(seed)
    a = am.Automaton(needles)
    a.set_kernel(ROUTES[route])
    t = am.SpanTable(a, word_bytes=sorted(cls))
    cols = ref.random_weights(rng, len(needles), n_cols)
    w = am.Weights(t.values, cols)
    out = []
    for case in cases:
        exp = ref.expect_words(needles, len(needles), case, cols, hays, cls)
        with Batch(hays) as b:
            got = t.score_batch(case, b, w).scores
        if not np.array_equal(got, exp):
            c, h = np.argwhere(got != exp)[0]
            raise AssertionError((needles, case, "column", int(c), "haystack", int(h), hays[h], int(got[c, h]), int(exp[c, h])))
        out.append(exp)
    return out


def test_whole_words(route):
    needles = ["he", "the", "she", "art", "a"]
    hays = ["the he she", "he", "", "she the", "theshe he", "a art a", "he-she_he", "the", " he ", "he he", "xhe", "hex"]
    for cls in (wref.DEFAULT_CLASS, wref.LOWER_CLASS, frozenset(b"t"), wref.EMPTY_CLASS, wref.FULL_CLASS):
        check_words(needles, hays, cls, route)
    # a column of ones is the haystack's whole-word occurrences; the front end; a table without a class is the plain form
    a = am.Automaton(needles)
    a.set_kernel(ROUTES[route])
    ones = [1] * len(needles)
    assert a.score(0, ["the he she", "he"], ones).tolist() == [[5, 1]] and a.score(0, ["the he she", "he"], ones, whole_words=True).tolist() == [[3, 1]]
    assert a.score(0, ["the he she", "he"], ones, whole_words=b"t").tolist() == [[4, 1]]
    t = am.SpanTable(a)
    cols = [[1, 20, 300, 4000, 50000]]
    with Batch(hays) as b:
        assert np.array_equal(t.score_batch(1, b, am.Weights(t.values, cols)).scores, ref.expect(needles, None, 5, 1, cols, hays))
    # spans at the start and at the end of their haystacks: the last byte before and the first byte after a haystack are no neighbours, nor is the padding
    text = "ab ba bab a b aba " * 9
    seams = [text[n % 7:n % 7 + n] for n in range(131)] + [text[5:5 + n] for n in range(131)]
    exp = check_words(["ab", "ba", "a", "bab"], seams, wref.DEFAULT_CLASS, route, cases=(0,), n_cols=1)[0]
    assert np.count_nonzero(exp) > 100
    check_words(["ab", "a", "b"], ["xab", "ab", "", "abx", "a", "b", "x ab", "cd ab", "  ab ab"], wref.DEFAULT_CLASS, route)
    # IgnoreCase: the neighbours of the span the text gives, not of the needle's length
    check_words(["k", "åk"], [" " + KELVIN + " ", "a" + KELVIN + "b", KELVIN, KELVIN + " k", "k" + KELVIN, "-" + KELVIN + "-k-K", ANGSTROM + KELVIN + " " + ANGSTROM + "k"],
                wref.DEFAULT_CLASS, route, cases=(1,))


@pytest.mark.parametrize("seed", range(2))
def test_whole_words_fragment_pool(route, seed):
    """The pool's alphabets hold no separator of the default class, so every case also gets its haystacks joined by a blank and by a hyphen."""
    rng = random.Random(7500 + seed)
    for i in range(8):
        needles, hays = fragment_case(rng, allow_empty_needle=False)
        needles = [x for x in needles if x]
        if not needles:
            continue
        hays = hays + [" ".join(hays), "-".join(reversed(hays))]
        cls = (wref.DEFAULT_CLASS, wref.LOWER_CLASS)[i % 2]
        check_words(needles, hays, cls, route, cases=(0,), n_cols=(1, 3, 8)[i % 3], seed=i)
        check_words(lowered(needles), hays, cls, route, cases=(1,), n_cols=(1, 3, 8)[i % 3], seed=i)


# ---- 6. the identities of the header

def test_identities(route):
    needles, hays = pool_case(300 + sorted(ROUTES).index(route), n_hay=280, max_frags=8, alphabet="abAB12")
    n = len(needles)
    rng = random.Random(5)
    cols = [[1] * n] + ref.random_weights(rng, n, 2)
    for case in (0, 1):
        needles = lowered(needles) if case else needles
        sc = Scorer(needles, route)
        w = sc.weights(cols)
        with Batch(hays) as b:
            scores = w.score_batch(case, b).scores
            counts = np.zeros(len(hays), np.uint64)
            total = C.c_uint64(0)
            am.api.check(lib().am_count_batch(sc.a.device, case, b, counts.ctypes.data, C.byref(total)))
            by_needle = sc.t.count_by_needle_batch(case, b)
            offs, ents = sc.t.count_matrix_batch(case, b)
        assert np.array_equal(scores, ref.expect(needles, None, n, case, cols, hays))
        assert scores[0].tolist() == counts.tolist() and int(counts.sum()) > 100                    # a column of ones is am_count_batch's counts_out
        for c, col in enumerate(cols):
            assert int(scores[c].astype(np.uint64).sum(dtype=np.uint64)) == sum(int(by_needle[v]) * col[v] for v in range(n)) % 2 ** 64      # sum over the haystacks
            for i in range(len(hays)):                                                              # the matrix's row i times the column
                row = ents[int(offs[i]):int(offs[i + 1])]
                assert int(scores[c, i]) == ref.wrap(sum(int(e["count"]) * col[int(e["needle"])] for e in row)), (c, i)


# ---- 7. top-k

TOPK_COLUMNS = [[1, 2 ** 32], [1, 2 ** 56], [-1, -2 ** 40], [2 ** 61, -2 ** 61], [0, 0], [0, 5], [-3, 3], [ref.INT64_MIN, 1]]
TOPK_SIZES = [1, 2, 255, 256, 257, "block - 1", "block", "block + 1", "3 * block + 5"]


def topk_batch(n_hay):
    """haystack i = a x c_i + b x d_i: scores c_i * w_a + d_i * w_b, keys that differ in chosen bytes and signs; every other haystack has no b."""
    rng = random.Random(n_hay)
    cs = [rng.randrange(4) for _ in range(n_hay)]
    ds = [0 if i % 2 else rng.randrange(1, 4) for i in range(n_hay)]
    hays = ["a" * c + "b" * d for c, d in zip(cs, ds)]
    exp = np.zeros((len(TOPK_COLUMNS), n_hay), np.int64)
    for c, (wa, wb) in enumerate(TOPK_COLUMNS):
        for i in range(n_hay):
            exp[c, i] = ref.wrap(cs[i] * wa + ds[i] * wb)
    return hays, exp


@pytest.mark.parametrize("n_hay", TOPK_SIZES)
def test_top_k(n_hay):
    _, block = am.api.score_geometry()
    n = n_hay if isinstance(n_hay, int) else {"block - 1": block - 1, "block": block, "block + 1": block + 1, "3 * block + 5": 3 * block + 5}[n_hay]
    hays, exp = topk_batch(n)
    if n <= 257:
        assert np.array_equal(exp, ref.expect(["a", "b"], None, 2, 0, TOPK_COLUMNS, hays))
    w = Scorer(["a", "b"]).weights(TOPK_COLUMNS)
    with Batch(hays) as b:
        x = w.score_batch(0, b)
        assert np.array_equal(x.scores, exp)
        for c in range(len(TOPK_COLUMNS)):
            for k in sorted({0, 1, n - 1, n, n + 7, n // 2, n // 4 + 1}):
                for largest in (True, False):
                    want = ref.top_k(exp[c], k, largest)
                    got = x.top_k(k, column=c, largest=largest)
                    assert got.dtype == am.api.SCORED_DTYPE and [(int(s), int(h)) for s, h in zip(got["score"], got["haystack"])] == want, (n, c, k, largest)
                    assert not got["reserved"].any()
                    s = x.select_top_k(k, column=c, largest=largest, batch=b)
                    idx = sorted(h for _, h in want)
                    assert s.indices.tolist() == idx, (n, c, k, largest)
                    if c in (1, 4, 5) and k in (1, n - 1, n // 2):
                        check_texts(b, s, hays, idx, (n, c, k, largest))
    assert len(set(exp[4].tolist())) == 1 and (n < 4 or np.count_nonzero(exp[5] == 0) >= n // 2)      # all equal; half of them equal: the cut falls inside a tie group


def test_top_k_refusals_and_a_held_result():
    hays, exp = topk_batch(300)
    sc = Scorer(["a", "b"])
    w = sc.weights(TOPK_COLUMNS[:2])
    out = C.c_void_p(1)
    with Batch(hays) as b, Batch(hays[:299]) as shorter, Batch(hays[:299] + ["bbbbbbbb"]) as longer:
        x = w.score_batch(0, b)
        row, n_out = np.zeros(4, am.api.SCORED_DTYPE), C.c_uint64(9)
        assert lib().am_scores_top_k(x.handle, 2, 3, 1, row.ctypes.data, C.byref(n_out)) == am.AM_ERR_INVALID and n_out.value == 0 and b"column" in lib().am_last_error()
        assert lib().am_scores_top_k(x.handle, 0, 3, 1, None, C.byref(n_out)) == am.AM_ERR_INVALID and b"out is null" in lib().am_last_error()
        assert lib().am_scores_top_k(x.handle, 0, 0, 1, None, C.byref(n_out)) == am.AM_OK and n_out.value == 0      # k == 0 gives nothing
        for call in (lambda: lib().am_select_top_k(x.handle, 2, 3, 1, b, C.byref(out)), lambda: lib().am_select_score(x.handle, 2, 0, 1, 0, b, C.byref(out))):
            out.value = 1
            assert call() == am.AM_ERR_INVALID and not out.value and b"column" in lib().am_last_error()
        for other in (shorter, longer):                    # another haystack count; the same count and other bytes
            for call in (lambda: lib().am_select_top_k(x.handle, 0, 3, 1, other, C.byref(out)), lambda: lib().am_select_score(x.handle, 0, 0, 1, 0, other, C.byref(out))):
                out.value = 1
                assert call() == am.AM_ERR_INVALID and not out.value and b"not made from a batch" in lib().am_last_error()
        # a span table over other needle ids
        t = am.SpanTable(sc.a, word_bytes=True)
        out.value = 1
        assert lib().am_score_spans_batch(t.handle, w.handle, 0, b, C.byref(out)) == am.AM_ERR_INVALID and not out.value and b"same needle ids" in lib().am_last_error()
        # a held result: n_hay must be above the last record's haystack; its scores select from the batch by the haystack count
        m = run_matches(sc.a, 0, b)
        try:
            out.value = 1
            assert lib().am_matches_score(m, w.handle, 299, C.byref(out)) == am.AM_ERR_INVALID and not out.value and b"largest haystack index" in lib().am_last_error()
            held = w.score_matches(m, 300)
            assert np.array_equal(held.scores, exp[:2])
            assert held.select_top_k(5, column=1, batch=b).indices.tolist() == sorted(h for _, h in ref.top_k(exp[1], 5))
        finally:
            lib().am_matches_free(m)
    # a result assembled on the host (am_run in segments) has no records in HBM
    am.debug_set("AM_RUN_SEGMENTS", 1)
    s = am.api._Slices(hays)
    m = C.c_void_p()
    am.api.check(lib().am_run(sc.a.device, 0, s.arr, s.n, C.byref(m)))
    try:
        assert lib().am_matches_size(m) > 0 and not lib().am_matches_device_data(m)
        out.value = 1
        assert lib().am_matches_score(m, w.handle, 300, C.byref(out)) == am.AM_ERR_UNSUPPORTED and not out.value
        assert b"am_matches_score" in lib().am_last_error() and b"assembled on the host" in lib().am_last_error()
    finally:
        lib().am_matches_free(m)
    # more columns than the maximum, none at all
    for bad in ([[1, 2]] * 9, np.zeros((0, 2), np.int64)):
        with pytest.raises(am.AmError) as e:
            sc.weights(bad)
        assert e.value.code == am.AM_ERR_INVALID


# ---- 8. range select, a selection of a selection

def test_range_select():
    _, block = am.api.score_geometry()
    n = block + 77
    hays, exp = topk_batch(n)
    sc = Scorer(["a", "b"])
    w = sc.weights(TOPK_COLUMNS)
    with Batch(hays) as b:
        x = w.score_batch(0, b)
        for c, lo, hi in [(0, 2, 2 ** 32 + 1), (0, 2 ** 33, 2 ** 34), (2, -2 ** 41, -2), (2, 0, 0), (3, ref.INT64_MIN, -1), (7, ref.INT64_MIN, ref.INT64_MIN), (5, 5, 10),
                          (1, ref.INT64_MIN, ref.INT64_MAX), (1, 5, 4), (0, ref.INT64_MAX, ref.INT64_MIN), (4, 1, 9), (6, -3, 3)]:
            for invert in (False, True):
                idx = ref.in_range(exp[c], lo, hi, invert)
                s = x.select(lo, hi, column=c, invert=invert, batch=b)
                assert s.indices.tolist() == idx, (c, lo, hi, invert)
                if c in (0, 1, 4):
                    check_texts(b, s, hays, idx, (c, lo, hi, invert))
        assert x.select(ref.INT64_MIN, ref.INT64_MAX, column=1, batch=b).size == n and x.select(5, 4, column=1, batch=b).size == 0      # everything; lo > hi: nothing
        assert x.select(1, 9, column=4, batch=b).size == 0 and x.select(1, 9, column=4, invert=True, batch=b).size == n                 # nothing kept; inverted
        # a selection of a selection: the haystacks with a b, their batch scored again, the five best of those -- indices compose through the two arrays
        first = x.select(1, ref.INT64_MAX, column=5, batch=b)
        idx1 = ref.in_range(exp[5], 1, ref.INT64_MAX)
        assert first.indices.tolist() == idx1 and 0 < len(idx1) < n
        nb = first.batch(b)
        try:
            y = w.score_batch(0, nb)
            assert np.array_equal(y.scores, exp[:, idx1])
            second = y.select_top_k(5, column=0, batch=nb)
            want = sorted(h for _, h in ref.top_k(exp[0, idx1], 5))
            assert second.indices.tolist() == want
            check_texts(nb, second, [hays[i] for i in idx1], want, "second")
            assert [idx1[i] for i in second.indices.tolist()] == sorted(idx1[h] for h in want)
            third = y.select(0, 2 ** 33, column=0, invert=True, batch=nb)
            assert third.indices.tolist() == ref.in_range(exp[0, idx1], 0, 2 ** 33, True)
        finally:
            lib().am_batch_destroy(nb)


# ---- 9. determinism, leaks

def test_runs_agree_and_nothing_is_left_in_hbm(route):
    needles, hays = pool_case(77, n_hay=400, max_frags=10, alphabet="abAB12")
    cols = ref.random_weights(random.Random(2), len(needles), 8)
    sc = Scorer(needles, route)
    exp = ref.expect(needles, None, len(needles), 1, cols, hays)

    def everything():
        w = sc.weights(cols)
        with Batch(hays) as b:
            x, y = w.score_batch(1, b), w.score_batch(1, b)
            one = w.score_texts(1, hays)
            assert x.scores.tobytes() == exp.tobytes() and y.scores.tobytes() == exp.tobytes() and one.scores.tobytes() == exp.tobytes()
            tops = [x.top_k(17, column=c).tobytes() for c in range(8)]
            assert tops == [y.top_k(17, column=c).tobytes() for c in range(8)]
            s1, s2 = x.select_top_k(40, column=3, batch=b), x.select(-2 ** 30, 2 ** 30, column=2, batch=b)
            assert s1.size == 40 and s1.indices.tolist() == y.select_top_k(40, column=3, batch=b).indices.tolist()
            nb = s2.batch(b)
            lib().am_batch_destroy(nb)
        return tops

    first = everything()                                    # (the first call also makes what stays: the automaton's image, the calling thread's one-shot batch)
    start = int(lib().am_debug_device_buffer_bytes())
    assert everything() == first
    assert int(lib().am_debug_device_buffer_bytes()) == start      # weights, scores, selections and their batch: freed, nothing left in HBM
