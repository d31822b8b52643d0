"""Whole-word matching on the device (am_span_table_create_words, am_count_spans_by_needle*, csrc/am_words.h) against the definition.  Every check compares the bytes of
(offsets, spans), the rewritten texts or the counts of the one-shot form, the batch form and the host mirror with what tests/words_reference.py says -- spans_reference
over the oracle, filtered by the whole-word rule, then selected -- or with literals, never with another path of the library."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers, spans_reference as ref, words_reference as wref

pytestmark = pytest.mark.gpu

ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}
MODES = (ref.ALL, ref.LEFTMOST_LONGEST)
A_RING, KELVIN, ANGSTROM, SHARP_S, DOTTED_I = "\u00c5", "\u212a", "\u212b", "\u1e9e", "\u0130"
REPLS = ["", "!", "<" + "r" * 15 + ">"]                    # 0, 1 and 17 bytes


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield ROUTES[request.param]
    am.debug_set("AM_DFA", -1)


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


class Batch:
    def __init__(self, hays):
        self.s = am.api._Slices(hays)
        self.h = C.c_void_p()

    def __enter__(self):
        am.api.check(am.api.libam().am_batch_upload(self.s.arr, self.s.n, C.byref(self.h)))
        return self.h

    def __exit__(self, *exc):
        am.api.libam().am_batch_destroy(self.h)


def as_arrays(rows):
    """Rows of (start, len, handle) per haystack as the (offsets, spans) arrays of the C ABI."""
    offs = np.zeros(len(rows) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    spans = np.zeros(int(offs[-1]), am.api.SPAN_DTYPE)
    flat = [(s, n, h, v) for h, r in enumerate(rows) for s, n, v in r]
    if flat:
        spans[:] = flat
    return offs, spans


def same(got, exp):
    return got[0].tobytes() == exp[0].tobytes() and got[1].tobytes() == exp[1].tobytes()


def first_difference(got, exp):
    if got[0].tolist() != exp[0].tolist():
        return "offsets", got[0].tolist()[:12], exp[0].tolist()[:12]
    for k, (g, e) in enumerate(zip(got[1].tolist(), exp[1].tolist())):
        if g != e:
            return k, g, e
    return len(got[1]), len(exp[1])


def take(b):
    try:
        return am.api.batch_to_bytes(b)[1]
    finally:
        am.api.libam().am_batch_destroy(b)


class Words:
    """An automaton on a route, its oracle twin, a span table with the word class `cls` (a set of byte values) and replacements: handle v stands for by_handle[v]."""

    def __init__(self, needles, route, cls=wref.DEFAULT_CLASS, values=None, by_handle=None, n=None):
        self.by_handle = list(needles) if by_handle is None else by_handle
        self.n, self.cls = n, cls
        self.a = am.Automaton(needles, values)
        self.a.set_kernel(route)
        self.o = oracle.Machine(needles, values)
        self.lengths = tuple(x[:len(self.by_handle)] for x in am.api.needle_lengths(self.by_handle))
        self.t = am.SpanTable(self.a, n, lengths=self.lengths, word_bytes=sorted(cls))
        assert self.t.word_bytes == wref.flags(cls)
        self.nn = self.t.n_needles
        self.repls = [_b(REPLS[v % 3] + (str(v) if v % 3 else "")) for v in range(self.nn)]
        self.r = am.SubstTable(self.t, self.repls)

    def expected(self, case, mode, hays):
        return as_arrays(wref.spans(self.o, case, mode, self.by_handle, hays, self.cls, self.n))

    def triples(self, case, hays):
        """The fold steps of the DEVICE scan: what the host mirror folds."""
        return self.a.run_batch_with_case(case, hays)

    def check(self, case, mode, hays, exp=None):
        """am_spans == am_spans_batch == the host mirror == the definition, byte for byte, twice; returns the arrays."""
        exp = self.expected(case, mode, hays) if exp is None else exp
        for run in range(2):
            one = self.t.spans_texts(case, hays, mode)
            assert same(one, exp), ("am_spans", case, mode, run, first_difference(one, exp))
            with Batch(hays) as b:
                got = self.t.spans_batch(case, b, mode)
                assert same(got, exp), ("am_spans_batch", case, mode, run, first_difference(got, exp))
        got = am.api.spans_fold_host(case, mode, self.triples(case, hays), hays, self.lengths[0][:self.nn], self.lengths[1][:self.nn], word_bytes=sorted(self.cls))
        assert same(got, exp), ("host mirror", case, mode, first_difference(got, exp))
        return exp

    def check_counts(self, case, hays):
        """am_count_spans_by_needle == ..._batch == the bincount of the definition's AM_SPANS_ALL rows, twice."""
        exp = wref.counts(self.o, case, self.by_handle, hays, self.cls, self.nn)
        for run in range(2):
            assert self.t.count_by_needle_texts(case, hays).tolist() == exp, ("am_count_spans_by_needle", case, run)
            with Batch(hays) as b:
                assert self.t.count_by_needle_batch(case, b).tolist() == exp, ("am_count_spans_by_needle_batch", case, run)
        return exp

    def check_substitute(self, case, hays):
        """am_substitute == am_substitute_batch == am_batch_substitute over a separately made spans result == the host mirror == the definition, twice."""
        exp = wref.substitute(self.o, case, self.by_handle, hays, self.repls, self.cls, self.n)
        for run in range(2):
            assert self.r.substitute_texts(case, hays) == exp, ("am_substitute", case, run)
            with Batch(hays) as b:
                assert take(self.r.substitute_batch(case, b, raw=True)) == exp, ("am_substitute_batch", case, run)
                x = self.t.spans_batch(case, b, ref.LEFTMOST_LONGEST, raw=True)
                try:
                    assert take(self.r.splice(b, x, raw=True)) == exp, ("am_batch_substitute", case, run)
                finally:
                    am.api.libam().am_spans_free(x)
        got = am.api.substitute_fold_host(case, self.triples(case, hays), hays, self.lengths[0][:self.nn], self.lengths[1][:self.nn], self.repls, word_bytes=sorted(self.cls))
        assert got == exp, ("host mirror", case)
        return exp

    def check_all(self, hays, cases=(0, 1)):
        for case in cases:
            for mode in MODES:
                self.check(case, mode, hays)
            self.check_counts(case, hays)
            self.check_substitute(case, hays)


# ---- 1. the fragment pool

@pytest.mark.parametrize("limit", [-1, 1])
@pytest.mark.parametrize("seed", range(2))
def test_fragment_pool(route, seed, limit):
    """The pool of the span tests under the default class and the a-z class (digits, capitals and non-ASCII bytes separate), once more with every chain of three sent
    to the doubling rounds.  The pool's alphabets hold no separator of the default class, so every case also gets its haystacks joined by a blank and by a hyphen.  A
    table with the EMPTY class gives the bytes of a plain table on the same batch."""
    am.debug_set("AM_SPANS_CHAIN_LIMIT", limit)
    rng = random.Random(7300 + seed)
    for i in range(6):
        needles, hays = helpers.fragment_case(rng)
        if i % 3 == 0:
            needles = needles + [needles[0]]               # a needle listed twice: two handles, the smaller one wins leftmost-longest
        if i % 4 == 2 and "" not in needles:
            needles = needles + [""]                       # the empty needle: zero-length spans, whole words where both neighbours separate
        if "" in needles and route == ROUTES["table_walk"]:
            continue                                       # the empty needle: no DFA section (the dense route reports those)
        hays = hays + [" ".join(hays), "-".join(reversed(hays)) + " " + needles[0]]
        for cls in (wref.DEFAULT_CLASS, wref.LOWER_CLASS):
            Words(needles, route, cls).check_all(hays)
        empty, plain = Words(needles, route, wref.EMPTY_CLASS), am.SpanTable(am.Automaton(needles))
        with Batch(hays) as b:
            for case in (0, 1):
                for mode in MODES:
                    assert same(empty.t.spans_batch(case, b, mode), plain.spans_batch(case, b, mode)), (case, mode)
                assert empty.t.count_by_needle_batch(case, b).tolist() == plain.count_by_needle_batch(case, b).tolist()


# ---- 2. the examples of include/am.h

EXAMPLES = [
    (["he", "the"], "the he she", {ref.ALL: [(0, 3, 1), (4, 2, 0)], ref.LEFTMOST_LONGEST: [(0, 3, 1), (4, 2, 0)]}),
    (["ab", "ab c"], "ab cd", {ref.ALL: [(0, 2, 0)], ref.LEFTMOST_LONGEST: [(0, 2, 0)]}),
    (["c++"], "c++ is", {ref.ALL: [(0, 3, 0)], ref.LEFTMOST_LONGEST: [(0, 3, 0)]}),
    (["ab"], "ab xab abx ab", {ref.ALL: [(0, 2, 0), (11, 2, 0)], ref.LEFTMOST_LONGEST: [(0, 2, 0), (11, 2, 0)]}),
]


def test_examples(route):
    for needles, text, want in EXAMPLES:
        d = Words(needles, route)
        for mode, rows in want.items():
            d.check(0, mode, [text], exp=as_arrays([rows]))
        d.check_all([text, "", text + text, text + " " + text])
    a = am.Automaton(["ab", "ab c"])
    a.set_kernel(route)
    assert a.spans(0, ["ab cd"], leftmost_longest=True)[1].tolist() == [(0, 4, 0, 1)]                      # the plain table takes `ab c` ...
    assert a.spans(0, ["ab cd"], leftmost_longest=True, whole_words=True)[1].tolist() == [(0, 2, 0, 0)]    # ... the class is applied BEFORE the selection
    assert a.substitute(0, ["ab cd"], ["X", "Y"]) == [b"Yd"] and a.substitute(0, ["ab cd"], ["X", "Y"], whole_words=True) == [b"X cd"]
    a = am.Automaton(["he", "the"])
    a.set_kernel(route)
    assert a.count_by_needle(0, ["the he she", "he"]).tolist() == [4, 1]
    assert a.count_whole_words(0, ["the he she", "he"]).tolist() == [2, 1]
    assert a.count_whole_words(0, ["the he she", "he"], word_bytes=b"t").tolist() == [3, 1]                # only t is a word byte: the he of `the` goes
    assert a.spans(0, ["the he she"], whole_words=b"s")[1].tolist() == [(0, 3, 0, 1), (1, 2, 0, 0), (4, 2, 0, 0)]


# ---- 3. haystack seams

def test_haystack_seams_in_one_batch(route):
    """The last byte of the haystack before and the first byte of the one after are never neighbours, nor is the padding behind the text."""
    d = Words(["ab", "a", "b"], route)
    hays = ["xab", "ab", "", "abx", "a", "b"]
    rows = [[], [(0, 2, 0)], [], [], [(0, 1, 1)], [(0, 1, 2)]]
    for case in (0, 1):
        for mode in MODES:
            d.check(case, mode, hays, exp=as_arrays(rows))
    d.check_all(hays)
    assert d.check_counts(0, hays) == [1, 1, 1]
    hays = ["x ab", "cd ab", "  ab ab"]                                  # 16 bytes in all, a match ends at the last one: kept, nothing behind it is a neighbour
    assert sum(len(h) for h in hays) == 16
    exp = d.check(0, ref.ALL, hays)
    assert exp[1].tolist()[-1] == (5, 2, 2, 0) and len(exp[1]) == 4
    d.check_all(hays)
    d.check_all([h * 2 for h in hays] + ["ab" * 8, "ab"])                # 32 + 16 + 2
    text = "ab ba bab a b aba " * 9
    hays = [text[n % 7:n % 7 + n] for n in range(131)] + [text[5:5 + n] for n in range(131)]      # 262 haystacks of 0 to 130 bytes: more than one workgroup of records
    d = Words(["ab", "ba", "a", "bab"], route)
    exp = d.expected(0, ref.ALL, hays)
    assert len(exp[1]) > 1000 and len(exp[1]) < len(as_arrays(ref.spans(d.o, 0, ref.ALL, d.by_handle, hays))[1]) // 2
    ends = exp[1]["start"] + exp[1]["len"]
    at_end = [h for h in range(len(hays)) if exp[0][h] < exp[0][h + 1] and int(ends[int(exp[0][h + 1]) - 1]) == len(hays[h])]
    at_start = [h for h in range(len(hays)) if exp[0][h] < exp[0][h + 1] and int(exp[1]["start"][int(exp[0][h])]) == 0]
    assert len(at_end) > 20 and len(at_start) > 20 and any(h + 1 in at_start for h in at_end)
    d.check_all(hays)


# ---- 4. IgnoreCase: the neighbours of the span the text gives, not of the needle's length

def test_ignore_case_widths(route):
    d = Words(["k"], route)
    assert d.check(1, ref.ALL, [" " + KELVIN + " ", "a" + KELVIN + "b"])[1].tolist() == [(1, 3, 0, 0)]      # the left neighbour is three bytes before the end
    d.check_all([" " + KELVIN + " ", "a" + KELVIN + "b", KELVIN, KELVIN + " k", "k" + KELVIN, "-" + KELVIN + "-k-K"])
    low_i = oracle.lower_utf8(DOTTED_I).decode()
    d = Words(["i", low_i, "k"] if low_i != "i" else ["i", "k"], route)
    d.check_all([" " + DOTTED_I + " ", "a" + DOTTED_I + "b", DOTTED_I + " i " + low_i, "i" + DOTTED_I, " I-" + DOTTED_I + "-" + KELVIN])
    long_needle = "kåßx" * 75                                            # 300 code points, 450 bytes; its upper-case form is 750 bytes
    upper = (KELVIN + ANGSTROM + SHARP_S + "X") * 75
    d = Words([long_needle, "ßx", "x"], route)
    hays = [" " + upper + " ", "a" + upper + " ", " " + upper + "a", "a" + upper + "a", "-" + long_needle + "_", "_" + upper + "-", upper, upper + " " + long_needle]
    exp = d.check(1, ref.LEFTMOST_LONGEST, hays)
    assert exp[0].tolist() == [0, 1, 1, 1, 1, 1, 1, 2, 4] and exp[1][0].tolist() == (1, 750, 0, 0) and exp[1][3].tolist() == (751, 450, 7, 0)
    d.check_all(hays)


# ---- 5. the empty needle, handles, empty shapes

def test_empty_needle_and_shapes(route):
    if route != ROUTES["table_walk"]:                                    # the empty needle: no DFA section (the dense route reports those)
        d = Words(["", "a", "-"], route)
        hays = ["banana", " a ", "", "a- b", "-", "a--", "- -"]
        exp = d.check(0, ref.ALL, hays)
        plain = as_arrays(ref.spans(d.o, 0, ref.ALL, d.by_handle, hays))
        # a zero-length span is a row where both neighbours separate or do not exist, as (2, 0) of "a- b", and is dropped after an a
        zero, zero_plain = int((exp[1]["len"] == 0).sum()), int((plain[1]["len"] == 0).sum())
        assert (2, 0, 3, 0) in exp[1].tolist() and 0 < zero < zero_plain, (zero, zero_plain)
        d.check_all(hays)
    needles = ["ab", "ab", "cd", "abcd", "b", "xyz"]
    values = [0, 1, 0, 2, 3, 9]
    by_handle = ["ab", "ab", "abcd", "b"]                                # "ab" and "cd" share handle 0; handle 9 has no length: always skipped
    hays = ["ab cd ab", "", "xyz cd cdab", "b b ab xyz", "xyz", "abcd b"]
    for n in (4, 3, 1, 0):
        d = Words(needles, route, values=values, by_handle=by_handle[:max(n, 1)] if n else by_handle[:1], n=n)
        d.check_all(hays)
        if n == 0:
            offs, spans = d.t.spans_texts(0, hays, ref.ALL)
            assert offs.tolist() == [0] * 7 and len(spans) == 0          # n_needles = 0: empty rows
            assert len(d.t.count_by_needle_texts(0, hays)) == 0
    d = Words(needles, route, values=values, by_handle=by_handle)
    for mode in MODES:
        offs, spans = d.t.spans_texts(0, [], mode)                       # n_hay = 0
        assert offs.tolist() == [0] and len(spans) == 0
        offs, spans = d.t.spans_texts(1, ["qqq", "", "zzzz"], mode)      # a batch without a match
        assert offs.tolist() == [0, 0, 0, 0] and len(spans) == 0
        offs, spans = d.t.spans_texts(0, ["xaby", "abcdx"], mode)        # matches, none of them a whole word
        assert offs.tolist() == [0, 0, 0] and len(spans) == 0
    assert d.t.count_by_needle_texts(0, []).tolist() == [0, 0, 0, 0] and d.t.count_by_needle_texts(1, ["", ""]).tolist() == [0, 0, 0, 0]
    assert d.r.substitute_texts(0, []) == [] and d.r.substitute_texts(0, ["xaby", ""]) == [b"xaby", b""]
    d.check_all(["qqq", "", "zzzz"])


# ---- 6. term counts

WORDS = ["he", "the", "she", "art", "party", "a", "k", "he she", "c++", "ab"]


@functools.lru_cache(maxsize=None)
def natural():
    """40 haystacks of ~16 KiB of words and separators, every one beginning and ending with the needle `he`: a predicate that looked across a haystack seam (or a
    group seam) would see a word byte there and drop a match.  ~0.4 values per byte."""
    rng = random.Random(606)
    pool = WORDS + ["The", "SHE", "cart", "K", KELVIN, "hex", "c++x", "_a", "a1", "é", "théâtre"]
    hays = []
    for _ in range(40):
        parts = ["he"]
        size = 2
        while size < 16000:
            parts += [rng.choice([" ", " ", ", ", "\n", "-", ""]), rng.choice(pool)]
            size += len(parts[-1]) + len(parts[-2])
        hays.append("".join(parts) + " he")
    o = oracle.Machine(WORDS)
    return hays, {case: np.array(wref.counts(o, case, WORDS, hays, wref.DEFAULT_CLASS), np.uint64) for case in (0, 1)}


def launches(name, fn):
    lib = am.api.libam()
    am.api.check(lib.am_profile_enable(1))
    am.api.check(lib.am_profile_reset())
    try:
        r = fn()
        ms, n = C.c_double(0), C.c_uint64(0)
        am.api.check(lib.am_profile_read(name, C.byref(ms), C.byref(n)))
    finally:
        lib.am_profile_enable(0)
    return r, int(n.value)


def test_counts_are_the_bincount_of_the_rows(route):
    hays, exp = natural()
    part = hays[:4] + ["", "he"]
    d = Words(WORDS, route)
    for case in (0, 1):
        rows = d.t.spans_texts(case, part, ref.ALL)[1]
        got = d.check_counts(case, part)
        assert got == np.bincount(rows["needle"], minlength=len(WORDS)).tolist() and sum(got) > 5000          # more than one kHistTile of records
        am.debug_set("AM_HIST_FLUSH_TILES", 1)
        assert d.t.count_by_needle_texts(case, part).tolist() == got
        am.debug_set("AM_HIST_FLUSH_TILES", -1)
    plain = am.SpanTable(d.a)
    values = am.ValuesTable(d.a)
    with Batch(part) as b:
        for case in (0, 1):
            assert plain.count_by_needle_batch(case, b).tolist() == values.count_by_needle_batch(case, b).tolist()
            assert plain.count_by_needle_texts(case, part).tolist() == values.count_by_needle_batch(case, b).tolist()
            assert sum(plain.count_by_needle_batch(case, b).tolist()) > 2 * sum(d.t.count_by_needle_batch(case, b).tolist())      # most raw matches are infix hits


def test_counts_in_groups_of_haystacks():
    """AM_HIST_RECORDS_MIB = 1: 65 536 records in HBM at a time, so the batch is scanned and folded in groups of whole haystacks, each a sub-batch with a text and
    offsets of its own and haystack indices that count from its first one.  Every haystack begins and ends with a needle that is a whole word only if nothing of the
    neighbouring haystack is looked at."""
    hays, exp = natural()
    d = Words(WORDS, 0)
    with Batch(hays) as b:
        for case in (1, 0):
            free, n_free = launches(b"needle_hist_words", lambda: d.t.count_by_needle_batch(case, b))
            am.debug_set("AM_HIST_RECORDS_MIB", 1)
            forced, n_forced = launches(b"needle_hist_words", lambda: d.t.count_by_needle_batch(case, b))
            am.debug_set("AM_HIST_FLUSH_TILES", 1)
            again = d.t.count_by_needle_batch(case, b)
            am.debug_set("AM_HIST_FLUSH_TILES", -1)
            am.debug_set("AM_HIST_RECORDS_MIB", -1)
            assert np.array_equal(free, exp[case]) and np.array_equal(forced, exp[case]) and np.array_equal(again, exp[case]), case
            assert n_free == 1 and n_forced >= 3, (n_free, n_forced)
    assert int(exp[0][0]) >= 80 and int(exp[1][6]) > int(exp[0][6])      # `he` at both ends of 40 haystacks; K and U+212A count for k under IgnoreCase


# ---- 7. substitute

def test_substitute_whole_words(route):
    hays, _ = natural()
    part = [h[:3000] for h in hays[:4]] + ["", "the he she", "ab cd", "he"]
    needles = WORDS + ["ab c"]
    d = Words(needles, route)
    assert sorted({len(_b(REPLS[k])) for k in range(3)}) == [0, 1, 17]
    for case in (0, 1):
        exp = d.check_substitute(case, part)
        if case == 0:
            assert exp == wref.regex_substitute(needles, part, d.repls)
        assert exp[-3] == d.repls[1] + b" " + d.repls[7] and exp[-2] == d.repls[9] + b" cd"          # `he she` is the longest whole word at 4
        # the result is counted again: the replacements are new text like any other
        o = oracle.Machine(needles)
        assert d.t.count_by_needle_texts(case, exp).tolist() == wref.counts(o, case, needles, exp, wref.DEFAULT_CLASS)
    plain = am.SubstTable(am.SpanTable(d.a), d.repls)
    assert plain.substitute_texts(0, ["ab cd"]) == [d.repls[10] + b"d"]  # the plain table splices `ab c`


# ---- 8. reproducible

def test_runs_agree(route):
    hays, _ = natural()
    part = [h[:5000] for h in hays[:6]]
    d = Words(WORDS, route)
    for case in (0, 1):
        for mode in MODES:
            first, again = d.t.spans_texts(case, part, mode), d.t.spans_texts(case, part, mode)
            assert same(first, again) and len(first[1]) > 1000, (case, mode)
        assert d.t.count_by_needle_texts(case, part).tolist() == d.t.count_by_needle_texts(case, part).tolist()
        assert d.r.substitute_texts(case, part) == d.r.substitute_texts(case, part)
        offs, spans = d.t.spans_texts(case, part, ref.ALL)
        for h in range(len(part)):
            e = (spans["start"] + spans["len"])[int(offs[h]):int(offs[h + 1])].astype(np.int64)
            assert (np.diff(e) >= 0).all()                               # start + len is non-decreasing per haystack
