"""Match spans on the device (am_spans / am_spans_batch, csrc/am_spans.hip) against the definition.  Every check compares the bytes of (offsets, spans) of the one-shot
form, the batch form and the host mirror with what tests/spans_reference.py says -- a few lines of Python over oracle.Machine.run_list and
oracle.skip_code_points_backwards, or literals -- never with another path of the library."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers, spans_reference as ref, spans_seam_cases as seams

pytestmark = pytest.mark.gpu

ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}
MODES = (ref.ALL, ref.LEFTMOST_LONGEST)
A_RING, KELVIN, ANGSTROM, SHARP_S = "\u00c5", "\u212a", "\u212b", "\u1e9e"


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


class Dictionary:
    """An automaton on a route, its oracle twin and its span table: handle v stands for by_handle[v]."""

    def __init__(self, needles, route, values=None, by_handle=None, n=None):
        self.by_handle = list(needles) if by_handle is None else by_handle
        self.n = n
        self.a = am.Automaton(needles, values)
        self.a.set_kernel(route)
        self.o = oracle.Machine(needles, values)
        self.lengths = am.api.needle_lengths(self.by_handle)
        self.lengths = tuple(x[:len(self.by_handle)] for x in self.lengths)
        self.t = am.SpanTable(self.a, n, lengths=self.lengths)

    def expected(self, case, mode, hays):
        return as_arrays(ref.spans(self.o, case, mode, self.by_handle, hays, self.n))

    def check(self, case, mode, hays, exp=None, mirror=True):
        """am_spans == am_spans_batch == the host mirror == the definition, byte for byte; returns the arrays."""
        exp = self.expected(case, mode, hays) if exp is None else exp
        one = self.t.spans_texts(case, hays, mode)
        assert same(one, exp), ("am_spans", case, mode, first_difference(one, exp))
        with Batch(hays) as b:
            assert same(self.t.spans_batch(case, b, mode), exp), ("am_spans_batch", case, mode)
        if mirror:
            got = self.a.spans_host_mirror(case, hays, mode == ref.LEFTMOST_LONGEST, n_values=self.t.n_needles, lengths=self.lengths)
            assert same(got, exp), ("host mirror", case, mode, first_difference(got, exp))
        return exp

    def check_all(self, hays, cases=(0, 1)):
        for case in cases:
            for mode in MODES:
                self.check(case, mode, hays)


def first_difference(got, exp):
    if got[0].tolist() != exp[0].tolist():
        return "offsets", got[0].tolist()[:12], exp[0].tolist()[:12]
    for k, (g, e) in enumerate(zip(got[1].tolist(), exp[1].tolist())):
        if g != e:
            return k, g, e
    return len(got[1]), len(exp[1])


# ---- 1. the fragment pool (+ 5b: the doubling rounds on small inputs)

@pytest.mark.parametrize("limit", [-1, 1])
@pytest.mark.parametrize("seed", range(4))
def test_fragment_pool(route, seed, limit):
    """TestInstances.hs's generator: needles and haystacks from one fragment pool, the empty needle and empty haystacks among them.  AM_SPANS_CHAIN_LIMIT = 1: the
    head's lane looks at one candidate, so every chain of three and more is finished by pointer doubling."""
    am.debug_set("AM_SPANS_CHAIN_LIMIT", limit)
    rng = random.Random(7300 + seed)
    seen_empty = 0
    for i in range(10):
        needles, hays = helpers.fragment_case(rng)
        if i % 3 == 0:
            needles = needles + [needles[0]]               # a needle listed twice: two handles, the smaller one wins leftmost-longest
        if i % 5 == 2 and "" not in needles:
            needles = needles + [""]                       # the empty needle: zero-length spans, never selected
        if "" in needles:
            if route == ROUTES["table_walk"]:
                continue                                   # the empty needle: no DFA section (the dense route reports those)
            seen_empty += 1
        Dictionary(needles, route).check_all(hays)
        lowered = [oracle.lower_utf8(x).decode() for x in needles]
        if lowered != needles:
            Dictionary(lowered, route).check_all(hays, cases=(1,))
    assert route == ROUTES["table_walk"] or seen_empty >= 1


# ---- 2. the examples of include/am.h and of the issue

EXAMPLES = [
    (["b", "abc", "abcd"], "abcd", 0, {ref.ALL: [(1, 1, 0), (0, 3, 1), (0, 4, 2)], ref.LEFTMOST_LONGEST: [(0, 4, 2)]}),
    (["abcdefgh", "cd", "gh", "hi"], "abcdefghi xcd", 0, {ref.LEFTMOST_LONGEST: [(0, 8, 0), (11, 2, 1)]}),
    (["a", "aa", "aaa"], "aaaaaaa", 0, {ref.LEFTMOST_LONGEST: [(0, 3, 2), (3, 3, 2), (6, 1, 0)]}),
    (["ab", "ab"], "abab", 0, {ref.ALL: [(0, 2, 1), (0, 2, 0), (2, 2, 1), (2, 2, 0)], ref.LEFTMOST_LONGEST: [(0, 2, 0), (2, 2, 0)]}),
    (["", "a"], "banana", 0, {ref.ALL: [(1, 1, 1), (2, 0, 0), (3, 1, 1), (4, 0, 0), (5, 1, 1), (6, 0, 0)], ref.LEFTMOST_LONGEST: [(1, 1, 1), (3, 1, 1), (5, 1, 1)]}),
    (["åb"], ANGSTROM + "B" + A_RING + "b", 1, {ref.ALL: [(0, 4, 0), (4, 3, 0)], ref.LEFTMOST_LONGEST: [(0, 4, 0), (4, 3, 0)]}),
]


def test_examples(route):
    for needles, text, case, want in EXAMPLES:
        if "" in needles and route == ROUTES["table_walk"]:
            continue                                       # the empty needle: no DFA section
        d = Dictionary(needles, route)
        for mode, rows in want.items():
            d.check(case, mode, [text], exp=as_arrays([rows]))
        d.check_all([text, "", text + text])
    a = am.Automaton(["b", "abc", "abcd"])
    offs, spans = a.spans(am.CASE_SENSITIVE, ["abcd", "xb"], leftmost_longest=True)
    assert offs.tolist() == [0, 1, 2] and spans.tolist() == [(0, 4, 0, 2), (1, 1, 1, 0)]
    assert a.spans(am.CASE_SENSITIVE, ["abcd"])[1].tolist() == [(1, 1, 0, 0), (0, 3, 0, 1), (0, 4, 0, 2)]


# ---- 3. IgnoreCase: a match is as wide as the text, not as the needle

def test_ignore_case_widths(route):
    d = Dictionary(["k", "kk", "åb"], route)
    text = "kK" + KELVIN + "k" + KELVIN + KELVIN + " " + A_RING + "b" + ANGSTROM + "B" + "å" + KELVIN + "b" + ANGSTROM + "b" + KELVIN
    exp = d.check(1, ref.LEFTMOST_LONGEST, [text, KELVIN, text[::-1]])
    assert sorted(set(exp[1]["len"].tolist())) == [2, 3, 4, 6]          # kk | a lone U+212A, å + b | U+212A + k, U+212B + B | U+212A twice
    d.check_all([text, KELVIN, text[::-1]])
    long_needle = "kåßx" * 75                                            # 300 code points, 450 bytes; its upper-case form is 750 bytes
    upper = (KELVIN + ANGSTROM + SHARP_S + "X") * 75
    d = Dictionary([long_needle, "ßx", "x"], route)
    hays = ["ab" + upper + long_needle + "k", upper[:-1], "x" + upper]
    exp = d.check(1, ref.LEFTMOST_LONGEST, hays)
    assert exp[1][0].tolist() == (2, 750, 0, 0) and exp[1][1].tolist() == (752, 450, 0, 0)
    d.check_all(hays)


# ---- 4. bitmap words and haystack seams

def test_bitmap_and_haystack_seams(route):
    """Haystacks of every length from 0 to 130 bytes in one batch, cut from "abab...": a match starts at the first byte and ends at the last byte of nearly every
    one, and the starts fall on both sides of the bitmap's word boundaries."""
    needles = ["ab", "ba", "a", "bab"]
    hays = [("ab" * 66)[:n] for n in range(131)]
    d = Dictionary(needles, route)
    exp = d.expected(0, ref.ALL, hays)
    base = np.cumsum([0] + [len(h) for h in hays])
    g = set((base[exp[1]["haystack"]] + exp[1]["start"].astype(np.int64)).tolist())
    assert {31, 32, 63, 64, 65} <= g
    ends = exp[1]["start"] + exp[1]["len"]
    for h in (5, 64, 129):                                               # ... ends at the last byte of one, starts at the first byte of the next
        assert int(ends[int(exp[0][h]):int(exp[0][h + 1])].max()) == len(hays[h]) and int(exp[1]["start"][int(exp[0][h + 1])]) == 0
    d.check_all(hays)
    d.check_all([h[1:] for h in hays])                                   # the same with "baba...": the seams move by one


# ---- 5. one chain through everything

CHAIN_BYTES = 3 * (1 << 17) + 1


@functools.lru_cache(maxsize=None)
def chain_expected():
    """`a, aa, aaa` over a run of a's: ALL from the oracle's fold steps (ASCII: start = pos - length in both case modes), leftmost-longest as a literal."""
    o = oracle.Machine(["a", "aa", "aaa"])
    pos, val = o.run_list(0, b"a" * CHAIN_BYTES)
    every = np.zeros(len(pos), am.api.SPAN_DTYPE)
    every["len"] = val.astype(np.uint64) + 1
    every["start"] = pos - every["len"]
    every["needle"] = val
    k = CHAIN_BYTES // 3
    ll = np.zeros(k + 1, am.api.SPAN_DTYPE)
    ll["start"] = 3 * np.arange(k + 1, dtype=np.uint64)
    ll["len"][:k], ll["needle"][:k] = 3, 2
    ll["len"][k], ll["needle"][k] = 1, 0
    return {ref.ALL: (np.array([0, len(every)], np.uint64), every), ref.LEFTMOST_LONGEST: (np.array([0, k + 1], np.uint64), ll)}


def test_one_long_chain(route):
    """1.18 M spans over 393 217 bytes; every candidate overlaps the next, so the whole text is one chain of 393 217 candidates whose kept path has 131 073."""
    d = Dictionary(["a", "aa", "aaa"], route)
    text = b"a" * CHAIN_BYTES
    exp = chain_expected()
    assert len(exp[ref.ALL][1]) == 3 * CHAIN_BYTES - 3
    for case in (0, 1):
        for mode in MODES:
            d.check(case, mode, [text], exp=exp[mode], mirror=(case == 0))
    with Batch([text]) as b:
        x = d.t.spans_batch(0, b, ref.LEFTMOST_LONGEST, raw=True)
        try:
            rounds = am.api.libam().am_spans_rounds(x)
            assert 1 <= rounds <= 19, rounds                             # ceil(log2 131 073) + 1
        finally:
            am.api.libam().am_spans_free(x)
        x = d.t.spans_batch(0, b, ref.ALL, raw=True)
        try:
            assert am.api.libam().am_spans_rounds(x) == 0 and am.api.libam().am_spans_size(x) == 3 * CHAIN_BYTES - 3
        finally:
            am.api.libam().am_spans_free(x)


# ---- 6. a long span hides later heads

def test_a_long_span_hides_what_it_covers(route):
    """abcdefgh covers cd and gh and overlaps hi: candidates inside a kept span start chains of their own only where nothing reaches them."""
    rng = random.Random(61)
    parts = []
    for _ in range(5000):
        parts.append(rng.choice(["abcdefghi", "abcdefgh", "bcdefghi", "cdghi", "abcdefg"]))
        parts.append(rng.choice(["", " ", "x", " x", "xcd", "gh hi", "h"]))
    text = "".join(parts)
    d = Dictionary(["abcdefgh", "cd", "gh", "hi"], route)
    exp = d.check(0, ref.LEFTMOST_LONGEST, [text, text[::-1], text[3:4000]])
    assert 5000 < len(exp[1]) < 20000
    d.check(1, ref.LEFTMOST_LONGEST, [text.upper(), text])
    d.check(0, ref.ALL, [text, text[3:4000]])
    x_rounds = []
    with Batch([text]) as b:
        x = d.t.spans_batch(0, b, ref.LEFTMOST_LONGEST, raw=True)
        x_rounds.append(am.api.libam().am_spans_rounds(x))
        am.api.libam().am_spans_free(x)
    assert x_rounds == [0]                                               # short chains: no doubling round


# ---- 7. handles, empty tables, empty batches

def test_handles_and_empty_shapes(route):
    needles = ["ab", "ab", "cd", "abcd", "b", "xyz"]
    values = [0, 1, 0, 2, 3, 9]
    by_handle = ["ab", "ab", "abcd", "b"]                                # "ab" and "cd" share handle 0; handle 9 has no length: always skipped
    hays = ["abcdab", "", "xyzcdcdab", "bbabxyz", "xyz"]
    for n in (4, 3, 1, 0):
        d = Dictionary(needles, route, values=values, by_handle=by_handle[:max(n, 1)] if n else by_handle[:1], n=n)
        d.check_all(hays)
        if n == 0:
            offs, spans = d.t.spans_texts(0, hays, ref.ALL)
            assert offs.tolist() == [0] * 6 and len(spans) == 0          # n_needles = 0: empty rows
    d = Dictionary(needles, route, values=values, by_handle=by_handle)
    for mode in MODES:
        offs, spans = d.t.spans_texts(0, [], mode)                       # n_hay = 0
        assert offs.tolist() == [0] and len(spans) == 0
        offs, spans = d.t.spans_texts(1, ["qqq", "", "zzzz"], mode)      # a batch without a match
        assert offs.tolist() == [0, 0, 0, 0] and len(spans) == 0
        offs, spans = d.t.spans_texts(0, ["", ""], mode)                 # nothing to scan
        assert offs.tolist() == [0, 0, 0] and len(spans) == 0
    d.check_all(["qqq", "", "zzzz"])


# ---- 8. reproducible, and consistent with the counts and the records

def test_runs_agree_and_sizes_match_the_counts(route):
    rng = random.Random(88)
    needles, _ = helpers.fragment_case(rng, allow_empty_needle=False)
    needles = sorted(set(needles)) + ["a", "ab"]
    hays = ["".join(rng.choice(needles + ["a", "b", "1", " "]) for _ in range(rng.randint(0, 400))) for _ in range(40)]
    d = Dictionary(needles, route)
    for case in (0, 1):
        for mode in MODES:
            first = d.t.spans_texts(case, hays, mode)
            again = d.t.spans_texts(case, hays, mode)
            assert same(first, again), (case, mode)
        offs, spans = d.t.spans_texts(case, hays, ref.ALL)
        assert len(spans) == int(d.a.count_by_needle(case, hays).sum()) and len(spans) > 100
        recs = d.a.run_records(case, hays)
        ends = set(zip(recs["haystack"].tolist(), recs["end_pos"].tolist()))
        assert set(zip(spans["haystack"].tolist(), (spans["start"] + spans["len"]).tolist())) == ends
        for h in range(len(hays)):
            e = (spans["start"] + spans["len"])[int(offs[h]):int(offs[h + 1])].astype(np.int64)
            assert (np.diff(e) >= 0).all()                               # start + len is non-decreasing per haystack


# ---- 9. document -> lines -> spans without leaving HBM

def test_spans_of_the_lines_of_a_document(route):
    rng = random.Random(99)
    words = ["tshirt", "shirt", "shirts", "hi", "his", "irt", "k", "kk"]
    lines = [" ".join(rng.choice(words + ["x", "Shirt", KELVIN]) for _ in range(rng.randint(0, 12))) for _ in range(300)]
    doc = "\n".join(lines)
    d = Dictionary(words, route)
    sp = am.Splitter("\n")
    with Batch([doc]) as b:
        nb, line_offs = sp.lines_batch(b)
        try:
            assert line_offs.tolist() == [0, len(lines)]
            for case in (0, 1):
                for mode in MODES:
                    got = d.t.spans_batch(case, nb, mode)
                    assert same(got, d.expected(case, mode, lines)), (case, mode)
        finally:
            am.api.libam().am_batch_destroy(nb)


# ---- 10. covers across the seams of the prefix maximum: a lane, a wavefront, a tile, the sweep of the tile maxima (tests/spans_seam_cases.py)

@functools.lru_cache(maxsize=None)
def seam_expected(group, name):
    """(offsets, spans) of the definition over the case's literal rows; shared by the routes and the case modes"""
    rows = seams.leftmost_longest(group, name)
    lens = [len(r) for r in rows]
    offs = np.zeros(len(rows) + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    flat = np.array([x for r in rows for x in r], np.uint64).reshape(-1, 3)
    spans = np.zeros(len(flat), am.api.SPAN_DTYPE)
    spans["start"], spans["len"], spans["needle"] = flat[:, 0], flat[:, 1], flat[:, 2]
    spans["haystack"] = np.repeat(np.arange(len(rows), dtype=np.uint32), lens)
    return offs, spans


def check_seam_case(d, group, name):
    c = seams.case(group, name)
    exp = seam_expected(group, name)
    covered = c.n - len(exp[1])
    assert covered >= 6 and int(exp[0][-1]) == len(exp[1])
    for case in (0, 1):
        # every span there is, as a set, against the literal rows: one per byte -- the model itself
        offs, every = d.t.spans_texts(case, c.hays, ref.ALL)
        assert offs.tolist() == np.cumsum([0] + [len(h) for h in c.hays]).tolist(), (name, case)
        every = every[np.lexsort((every["start"], every["haystack"]))]
        for field, want in (("start", c.start), ("len", c.length), ("needle", c.needle), ("haystack", c.haystack)):
            assert np.array_equal(every[field], want), (name, case, field)
        d.check(case, ref.LEFTMOST_LONGEST, c.hays, exp=exp, mirror=(case == 0))


@pytest.mark.parametrize("name", seams.NAMES)
def test_covers_across_lanes_wavefronts_and_tiles(route, name):
    """A cover that ends one candidate before a seam, at it, one and five behind it; one that reaches it over a whole tile; haystacks that begin at it; texts whose
    last tile holds only the trailing element of `kept`."""
    check_seam_case(Dictionary(seams.needles(seams.geometry()), route), "tiles", name)


@pytest.mark.parametrize("name", seams.NAMES)
def test_covers_across_the_sweep_of_the_tile_maxima(name):
    """More tiles than one sweep of k_spans_tiles_max: what lies behind the sweep seam is covered only through the carry."""
    check_seam_case(Dictionary(seams.needles(seams.geometry()), ROUTES["default"]), "sweep", name)
