"""Per-needle exact case on the device (am_span_table_create_cased, csrc/am_cased.h, span_of<IC, WORDS, EXACT> of csrc/am_words.h) against the definition.  Every
check compares the bytes of (offsets, spans), counts or texts with what tests/cased_reference.py says -- spans_reference over the oracle's fold steps, filtered by the
exact rule with Python slicing, then by the word class, then selected -- or with literals, never with another path of the library."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import cased_reference as cref, near_reference as nref, postings_reference as pref, spans_reference as ref, words_reference as wref

pytestmark = pytest.mark.gpu

ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}
MODES = (ref.ALL, ref.LEFTMOST_LONGEST)
KELVIN, A_RING, ANGSTROM, DOTTED_I = cref.KELVIN, cref.A_RING, cref.ANGSTROM, cref.DOTTED_I
CLASSES = {"none": None, "default": wref.DEFAULT_CLASS, "aA": frozenset(b"aA")}


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
        k = next(i for i, (g, e) in enumerate(zip(got[0].tolist(), exp[0].tolist())) if g != e)
        return "offsets", k, got[0].tolist()[k - 1:k + 3], exp[0].tolist()[k - 1:k + 3]
    for k, (g, e) in enumerate(zip(got[1].tolist(), exp[1].tolist())):
        if g != e:
            return k, g, e
    return len(got[1]), len(exp[1])


def take(b):
    try:
        return am.api.batch_to_bytes(b)[1]
    finally:
        am.api.libam().am_batch_destroy(b)


class Dict:
    """An automaton over lower-cased needles on a route, its oracle twin and a span table with spellings (and a word class where given)."""

    def __init__(self, needles, exact, route, cls=None):
        self.needles, self.exact, self.cls = list(needles), list(exact), cls
        self.a = am.Automaton(self.needles)
        self.a.set_kernel(route)
        self.o = oracle.Machine(self.needles)
        self.t = am.SpanTable(self.a, word_bytes=None if cls is None else sorted(cls), exact=self.exact)
        assert self.t.exact == cref.spellings(self.exact)
        self.n = self.t.n_needles

    def expected(self, case, mode, hays):
        return as_arrays(cref.spans(self.o, case, mode, self.needles, hays, self.exact, self.cls))

    def check_batch(self, case, mode, b, exp, what=None):
        got = self.t.spans_batch(case, b, mode)
        assert same(got, exp), ("am_spans_batch", what, case, mode, first_difference(got, exp))

    def check(self, case, mode, hays, exp=None):
        """am_spans == am_spans_batch == the definition, byte for byte; returns the arrays."""
        exp = self.expected(case, mode, hays) if exp is None else exp
        one = self.t.spans_texts(case, hays, mode)
        assert same(one, exp), ("am_spans", case, mode, first_difference(one, exp))
        with Batch(hays) as b:
            self.check_batch(case, mode, b, exp)
        return exp


# ---- 1. the worked examples of include/am.h

def test_worked_examples(route):
    for needles, exact, text, want in cref.EXAMPLES:
        d = Dict(needles, exact, route)
        for mode, rows in want.items():
            d.check(1, mode, [text], exp=as_arrays([rows]))
            d.check(1, mode, [text, "", text], exp=as_arrays([rows, [], rows]))
            d.check(1, mode, ["", text + text, text])                  # (against the definition: the examples back to back)
    c = am.Cased(["US", "Apple", "nike"], exact=[1, 1, 0])
    c.automaton.set_kernel(route)
    assert c.highlight(["us, US and NIKE's apple"], "<b>", "</b>") == [b"us, <b>US</b> and <b>NIKE</b>'s apple"]
    assert c.spans(["us, US and NIKE's apple"])[1].tolist() == [(4, 2, 0, 0), (11, 4, 0, 2)]
    assert c.count_by_needle(["us, US and NIKE's apple", "Apple apple US"]).tolist() == [2, 1, 1]
    assert c.grep(["us", "an apple", "an Apple", "nIkE"])[0].tolist() == [2, 3]
    assert c.substitute(["US us Nike"], ["<0>", "<1>", "<2>"]) == [b"<0> us <2>"]
    assert c.extract(["the US and us"], before=1, after=1) == [[b" US "]]
    assert c.score(["US us", "apple Apple nike"], [1, 10, 100]).tolist() == [[1, 110]]
    assert c.doc_freq(["US", "us US", "Nike us"]).tolist() == [2, 0, 1]
    with c.postings(["US us", "US"]) as p:
        assert p.offsets.tolist() == [0, 2, 2, 2] and p.spans.tolist() == [(0, 2, 0, 0), (0, 2, 1, 0)]
    assert c.near(["US buys nike", "us buys nike"], {"land": ["US"], "brand": ["nike"]}, [("land", "brand", 10)]) == [[[(0, 2, 8, 4, 6)]], [[]]]
    # filter, then select -- and with the default class both predicates must hold
    c = am.Cased(["AB C", "ab"], exact={"AB C"})
    c.automaton.set_kernel(route)
    assert c.spans(["ab c"], leftmost_longest=True)[1].tolist() == [(0, 2, 0, 1)]
    c = am.Cased(["US", "nike"], exact=[1, 0])
    c.automaton.set_kernel(route)
    assert c.spans(["bonUS US nikes NIKE"])[1].tolist() == [(3, 2, 0, 0), (6, 2, 0, 0), (9, 4, 0, 1), (15, 4, 0, 1)]
    assert c.spans(["bonUS US nikes NIKE"], whole_words=True)[1].tolist() == [(6, 2, 0, 0), (15, 4, 0, 1)]


# ---- 2. differential: 200 texts in one batch, a third of the handles with a spelling

@functools.lru_cache(maxsize=None)
def differential(seed):
    (needles, exact, hays), = cref.seeded(9100 + seed, oracle.lower_utf8, 1, n_hay=200, n_needles=9, share=1 / 3)
    return needles, exact, hays


@functools.lru_cache(maxsize=None)
def differential_expected(seed, case, mode, cls):
    needles, exact, hays = differential(seed)
    return as_arrays(cref.spans(oracle.Machine(needles), case, mode, needles, hays, exact, CLASSES[cls]))


@pytest.mark.parametrize("seed", range(3))
def test_differential(route, seed):
    """Haystack seams are dense: 200 texts of 0 to 120 bytes, back to back.  Both case modes, both span modes, no class, the default class and {a, A}."""
    needles, exact, hays = differential(seed)
    kept = 0
    with Batch(hays) as b:
        for cls in sorted(CLASSES):
            d = Dict(needles, exact, route, CLASSES[cls])
            for case in (0, 1):
                for mode in MODES:
                    exp = differential_expected(seed, case, mode, cls)
                    d.check_batch(case, mode, b, exp, (seed, cls))
                    kept += len(exp[1])
    plain = as_arrays(ref.spans(oracle.Machine(needles), 1, ref.ALL, needles, hays))
    assert kept > 500 and len(differential_expected(seed, 1, ref.ALL, "none")[1]) < len(plain[1])       # rows are kept and rows are dropped


# ---- 3. comparator edges on the device

def _spelling(n):
    """n upper-case letters, another sequence for every n."""
    return "".join(chr(65 + (i * 7 + n * 3 + i // 5) % 26) for i in range(n))


@functools.lru_cache(maxsize=None)
def edges(last_is_identical):
    """A spelling of each length 1 to 40 at each residue 0 to 15 of the batch text: per placement one haystack with an identical copy and one with a copy that differs
    in its last byte only (the other case of the letter: the IgnoreCase scan still matches), each behind dots that bring it to the residue and in front of 0 or 1 more;
    a haystack that ends in the middle of a spelling while the next one begins with the rest; and the pair once more at the very end of the last haystack."""
    lengths = list(range(1, 41))
    needles = [_spelling(n).lower() for n in lengths]
    exact = [_spelling(n) for n in lengths]
    hays, total = [], 0

    def place(copy, residue, tail):
        nonlocal total
        pad = (residue - total) % 16
        hays.append("." * pad + copy + tail)
        total += len(hays[-1])

    for n in lengths:
        s = _spelling(n)
        for residue in range(16):
            place(s, residue, "." * (residue & 1))
            place(s[:-1] + s[-1].lower(), residue, "." * ((residue >> 1) & 1))
    s = _spelling(20)
    place(s[:9], 5, "")
    hays.append(s[9:])                                     # the rest of it: neighbouring haystacks never complete each other
    s = _spelling(33)
    differing = s[:-1] + s[-1].lower()
    hays.append("..." + (differing + s if last_is_identical else s + differing))
    rows = {(case, mode): as_arrays(cref.spans(oracle.Machine(needles), case, mode, needles, hays, exact)) for case in (0, 1) for mode in MODES}
    return needles, exact, hays, rows


@pytest.mark.parametrize("last_is_identical", [True, False])
def test_comparator_edges(route, last_is_identical):
    needles, exact, hays, rows = edges(last_is_identical)
    text = "".join(hays)
    starts = np.cumsum([0] + [len(h) for h in hays])
    exp = rows[(1, ref.ALL)]
    # what the batch holds, said by the definition: every (length, residue) placement is a row, the text ends with a spelling
    placed = {(int(s["len"]), int(starts[int(s["haystack"])] + s["start"]) % 16) for s in exp[1]}
    assert all((n, r) in placed for n in range(1, 41) for r in range(16))
    last = exp[1][-1]
    assert (int(last["haystack"]) == len(hays) - 1 and int(last["start"] + last["len"]) == len(hays[-1])) == last_is_identical and len(text) == int(starts[-1])
    assert not any(int(s["haystack"]) == len(hays) - 2 and int(s["len"]) == 20 for s in exp[1])
    d = Dict(needles, exact, route)
    with Batch(hays) as b:
        for key, e in rows.items():
            d.check_batch(key[0], key[1], b, e, "edges")
    assert len(rows[(0, ref.ALL)][1]) == 0                               # lower-cased needles, upper-case spellings: under AM_CASE_SENSITIVE no span is a row


# ---- 4. widths

def test_widths(route):
    low_i = oracle.lower_utf8(DOTTED_I).decode()
    text = " ".join(["k", "K", KELVIN, "å", A_RING, ANGSTROM, "i", "I", DOTTED_I, low_i, "kk", KELVIN + "K", "x"])
    hays = [text, KELVIN, "K", "k" + KELVIN + "K" + A_RING + ANGSTROM + "å", DOTTED_I + low_i + DOTTED_I, ""]
    for k_as, a_as, i_as in (("K", A_RING, DOTTED_I), (KELVIN, ANGSTROM, low_i), ("k", "å", None), (None, ANGSTROM, DOTTED_I)):
        needles, exact = ["k", "å", low_i], [k_as, a_as, i_as]
        for cls in (None, wref.DEFAULT_CLASS):
            d = Dict(needles, exact, route, cls)
            for case in (0, 1):
                for mode in MODES:
                    d.check(case, mode, hays)
    d = Dict(["k"], ["K"], route)
    assert d.check(1, ref.ALL, ["K k " + KELVIN])[1].tolist() == [(0, 1, 0, 0)]                  # U+212A is dropped: its len is 3, not 1
    d = Dict(["k"], [KELVIN], route)
    assert d.check(1, ref.ALL, ["K k " + KELVIN])[1].tolist() == [(4, 3, 0, 0)]                  # ... and with exact = U+212A the keeps and the drops swap
    d = Dict(["å"], [ANGSTROM], route)
    assert d.check(1, ref.ALL, ["å" + A_RING + ANGSTROM])[1].tolist() == [(4, 3, 0, 0)]
    d = Dict(["å"], [A_RING], route)
    assert d.check(1, ref.ALL, ["å" + A_RING + ANGSTROM])[1].tolist() == [(2, 2, 0, 0)]


# ---- 5. long spellings

def _long_spelling(n):
    rng = random.Random(n)
    return "".join(rng.choice("ABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(n))


@functools.lru_cache(maxsize=None)
def long_case():
    lengths = (17, 257, 66000)
    exact = [_long_spelling(n) for n in lengths] + [None]
    needles = [s.lower() for s in exact[:-1]] + ["z9"]
    hays = []
    for k, s in enumerate(exact[:-1]):
        hays += ["." * (k + 1) + s + "z9", "z9." + s[0].lower() + s[1:], "Z9" + s[:-1] + s[-1].lower() + s[:5]]
    rows = {(case, mode): as_arrays(cref.spans(oracle.Machine(needles), case, mode, needles, hays, exact)) for case in (0, 1) for mode in MODES}
    return needles, exact, hays, rows


def test_long_spellings(route):
    """17, 257 and 66 000 bytes: identical, differing in the first byte, differing in the last byte -- three haystacks per length."""
    needles, exact, hays, rows = long_case()
    exp = rows[(1, ref.ALL)]
    assert [(int(s["len"]), int(s["haystack"])) for s in exp[1] if s["needle"] < 3] == [(17, 0), (257, 3), (66000, 6)] and len(exp[1]) == 3 + 9
    d = Dict(needles, exact, route)
    with Batch(hays) as b:
        for key, e in rows.items():
            d.check_batch(key[0], key[1], b, e, "long")


# ---- 6. the consumers of the table agree with its rows

WORDS = ["us", "apple", "nike", "k", "who", "us", "ab c", "ab", "it"]
SPELLED = ["US", "Apple", None, KELVIN, "WHO", None, "AB C", None, "IT"]


@functools.lru_cache(maxsize=None)
def natural():
    """40 haystacks of ~16 KiB of words in several casings and separators, every one beginning and ending with a needle that is exact: a predicate that read
    beyond its haystack (or its group) would be seen.  More than 65 536 records under AM_IGNORE_CASE."""
    rng = random.Random(931)
    pool = ["US", "us", "Us", "Apple", "apple", "APPLE", "nike", "NIKE", "k", "K", KELVIN, "WHO", "who", "ab c", "AB C", "Ab", "it", "IT", "bonUS", "ITem", "x"]
    hays = []
    for _ in range(40):
        parts, size = ["US"], 2
        while size < 16000:
            parts += [rng.choice([" ", " ", ", ", "\n", "-", ""]), rng.choice(pool)]
            size += len(_b(parts[-1])) + len(parts[-2])
        hays.append("".join(parts) + " IT")
    return hays


@functools.lru_cache(maxsize=None)
def natural_rows(n_hay, cls):
    hays = natural()[:n_hay]
    o = oracle.Machine(WORDS)
    return {mode: cref.spans(o, 1, mode, WORDS, hays, SPELLED, CLASSES[cls]) for mode in MODES}


WEIGHTS = [[1, 10, 100, 1000, 7, -3, 5, 2, 1 << 40]]


def consumers(d, b, rows_all):
    n_hay = len(rows_all)
    counts = d.t.count_by_needle_batch(1, b).tolist()
    scores = d.t.score_batch(1, b, am.Weights(d.t.values, WEIGHTS)).scores.tolist()
    kept = d.t.select_batch(1, b).indices.tolist()
    exp_counts = np.bincount([v for r in rows_all for _, _, v in r], minlength=d.n).tolist()
    exp_scores = [[sum(WEIGHTS[0][v] for _, _, v in r) for r in rows_all]]
    assert counts == exp_counts, ("counts", counts, exp_counts)
    assert scores == exp_scores, ("scores", next(h for h in range(n_hay) if scores[0][h] != exp_scores[0][h]))
    assert kept == [h for h in range(n_hay) if rows_all[h]], "select"


@pytest.mark.parametrize("cls", ["none", "default"])
def test_consumers_agree(route, cls):
    hays = [h[:2500] for h in natural()[:6]] + ["", "us", "US", "bonUS"]
    o = oracle.Machine(WORDS)
    rows = {mode: cref.spans(o, 1, mode, WORDS, hays, SPELLED, CLASSES[cls]) for mode in MODES}
    d = Dict(WORDS, SPELLED, route, CLASSES[cls])
    repls = ["<%d>" % v if v % 2 else "" for v in range(d.n)]
    with Batch(hays) as b:
        for mode in MODES:
            d.check_batch(1, mode, b, as_arrays(rows[mode]))
        consumers(d, b, rows[ref.ALL])
        assert take(am.SubstTable(d.t, repls).substitute_batch(1, b, raw=True)) == cref.substitute(o, 1, WORDS, hays, repls, SPELLED, CLASSES[cls])
        exp = cref.highlight(o, 1, WORDS, hays, "<b>", "</b>", SPELLED, CLASSES[cls])
        assert take(am.SubstTable(d.t, [["<b>", am.MATCH, "</b>"]] * d.n).substitute_batch(1, b, raw=True)) == exp
        for mode in MODES:
            offsets, data, source, doc_freq = pref.postings(rows[mode], d.n)
            with d.t.postings_batch(1, b, mode) as p:
                assert p.offsets.tolist() == offsets and p.spans.tolist() == data and p.source.tolist() == source and p.doc_freq.tolist() == doc_freq, ("postings", mode)
        masks = [1, 2, 2, 3, 1, 0, 2, 1, 3]
        queries = [(0, 1, 12, False), (1, 0, 40, True)]
        x = am.Near(d.t, masks, queries).near_batch(1, b)
        offsets, pairs, _, counts = nref.near(rows[ref.LEFTMOST_LONGEST], masks, queries)
        assert x.offsets.tolist() == offsets and [tuple(int(v) for v in p) for p in x.pairs.tolist()] == pairs and x.counts.tolist() == counts and len(pairs) > 10


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


@pytest.mark.parametrize("cls", ["none", "default"])
def test_consumers_in_groups_of_haystacks(cls):
    """AM_HIST_RECORDS_MIB = 1: 65 536 records in HBM at a time, so the batch is scanned and folded in groups of whole haystacks, each a sub-batch with a text and
    offsets of its own.  The counts, the scores and the select's flags read the text of the group they run in."""
    hays = natural()
    rows = natural_rows(len(hays), cls)[ref.ALL]
    d = Dict(WORDS, SPELLED, 0, CLASSES[cls])
    with Batch(hays) as b:
        _, n_free = launches(b"needle_hist_words", lambda: consumers(d, b, rows))
        am.debug_set("AM_HIST_RECORDS_MIB", 1)
        try:
            _, n_forced = launches(b"needle_hist_words", lambda: consumers(d, b, rows))
        finally:
            am.debug_set("AM_HIST_RECORDS_MIB", -1)
    assert n_free == 1 and n_forced >= 3, (n_free, n_forced)


# ---- 7. no spelling means nothing changes

def test_no_spelling_is_the_table_of_today(route):
    needles, _, hays = differential(0)
    lib = am.api.libam()
    a = am.Automaton(needles)
    a.set_kernel(route)
    lb, lc = am.api.needle_lengths(needles)
    none = np.zeros(len(needles) + 1, np.uint64)
    with Batch(hays) as b:
        for words, old in ((None, am.SpanTable(a)), (True, am.SpanTable(a, word_bytes=True))):
            tables = [am.SpanTable(a, word_bytes=words, exact=[None] * len(needles))]
            for offs in (None, none.ctypes.data):                        # exact_off == NULL, and offsets that give every handle an empty range
                t = am.SpanTable(a, word_bytes=words)
                lib.am_span_table_destroy(t._h)
                t._h = C.c_void_p()
                am.api.check(lib.am_span_table_create_cased(t.values.handle, lb.ctypes.data, lc.ctypes.data, 1 if words else 0, None, offs, None, C.byref(t._h)))
                tables.append(t)
            for t in tables:
                assert t.exact == [None] * len(needles) and t.word_bytes == old.word_bytes
                for case in (0, 1):
                    for mode in MODES:
                        assert same(t.spans_batch(case, b, mode), old.spans_batch(case, b, mode)), (words, case, mode)
                    assert t.count_by_needle_batch(case, b).tolist() == old.count_by_needle_batch(case, b).tolist()


# ---- 8. determinism and the case modes

def test_runs_agree_and_case_sensitive_is_a_constant_per_needle(route):
    needles, exact, hays = differential(1)
    d = Dict(needles, exact, route)
    with Batch(hays) as b:
        for case in (0, 1):
            for mode in MODES:
                first, again = d.t.spans_batch(case, b, mode), d.t.spans_batch(case, b, mode)
                assert same(first, again), (case, mode)
            assert d.t.count_by_needle_batch(case, b).tolist() == d.t.count_by_needle_batch(case, b).tolist()
    hays = ["us US nike NIKE Apple apple", "", "US"]
    upper = Dict(["us", "nike", "apple"], ["US", "NIKE", "Apple"], route)
    own = Dict(["us", "nike", "apple"], ["us", "nike", "apple"], route)
    plain = am.SpanTable(own.a)
    for mode in MODES:
        assert upper.check(0, mode, hays)[0].tolist() == [0, 0, 0, 0]                                # upper-case spellings of lower-cased needles: the empty result
        assert same(own.check(0, mode, hays), plain.spans_texts(0, hays, mode))                      # the needle's own spelling: the plain result
    assert own.check(1, ref.ALL, hays)[1].tolist() == [(0, 2, 0, 0), (6, 4, 0, 1), (22, 5, 0, 2)]
