"""Proximity on the device (am_near_* / am_select_near, csrc/am_near.hip) against the definition.  Every check compares the pairs, their offsets, the fired bitmaps
(the bits beyond n_hay included) and the counts with what tests/near_reference.py says -- brute force over the oracle's leftmost-longest spans, or over literal rows
where every span is one byte -- never with another path of the library.  Shapes sit on the real seams: the 64 spans of a bitmap word, the spans a workgroup step
takes, and the sweep of the word links (am_near_geometry)."""
import ctypes as C
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from tests import near_reference as ref, scan_cases as sc, words_reference as wref
from tests.helpers import fragment_case
from tests.test_gpu_select import Batch, check_texts, lib, lowered

pytestmark = pytest.mark.gpu

ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}
KELVIN, ANGSTROM = "\u212a", "\u212b"                    # lower-case to k and å: the byte length changes
ABC = ["a", "b", "c"]                                      # a: group 0, b: group 1, c: no group -- every span is one byte, span index = byte index
ABC_MASKS = [1, 2, 0]
ANY = ref.ANYWHERE


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield request.param
    am.debug_set("AM_DFA", -1)


def geometry():
    tile, word = am.api.near_geometry()
    return tile, word, 4 * tile * word                      # ..., the spans one sweep of the word links covers


class Prox:
    """An automaton on a route, its span table and a proximity handle over it."""

    def __init__(self, needles, masks, queries, route="default", word_bytes=None):
        self.a = am.Automaton(needles)
        self.a.set_kernel(ROUTES[route])
        self.t = am.SpanTable(self.a, word_bytes=word_bytes)
        self.masks, self.queries = list(masks), list(queries)
        self.near = am.Near(self.t, masks, queries)


def rows_of_spans(offs, spans):
    return [[(int(s["start"]), int(s["len"]), int(s["needle"])) for s in spans[int(offs[h]):int(offs[h + 1])]] for h in range(len(offs) - 1)]


def check_hits(x, rows, masks, queries, what=None):
    """One result against the definition: pairs, offsets, fired (every word: the bits beyond n_hay are zero in the definition), counts, the shapes."""
    offsets, pairs, fired, counts = ref.near(rows, masks, queries)
    n_hay, nq = len(rows), len(queries)
    if isinstance(x, am.NearHits):
        assert (x.n_hay, x.n_queries, x.hay_words) == (n_hay, nq, (n_hay + 63) // 64), what
        got = (x.offsets, x.pairs, x.fired_words, x.counts)
        assert np.array_equal(x.fired, np.asarray(fired, bool).reshape(nq, n_hay)), (what, "fired bits")
    else:
        got = x
    go, gp, gf, gc = got
    assert go.dtype == np.uint64 and go.tolist() == offsets, (what, "offsets", go.tolist()[:20], offsets[:20])
    gl = [tuple(int(v) for v in p) for p in gp.tolist()]
    if gl != pairs:
        k = next((j for j in range(min(len(gl), len(pairs))) if gl[j] != pairs[j]), min(len(gl), len(pairs)))
        raise AssertionError((what, "pair", k, gl[k:k + 3], pairs[k:k + 3], len(gl), len(pairs)))
    assert gf.shape == (nq, (n_hay + 63) // 64) and [[int(w) for w in row] for row in gf] == ref.fired_words(fired, n_hay), (what, "fired")
    assert gc.tolist() == counts, (what, "counts")
    return pairs


def all_forms(px, case, hays):
    """am_near, am_near_batch, am_near_spans over a held spans result and the host mirror over the library's spans: four results that must be one.  Also the spans."""
    x1, (o1, s1) = px.near.near_texts(case, hays, spans=True)
    with Batch(hays) as b:
        x2, (o2, s2) = px.near.near_batch(case, b, spans=True)
        raw = px.t.spans_batch(case, b, am.api.SPANS_LEFTMOST_LONGEST, raw=True)
        try:
            x3 = px.near.near_spans(raw)
        finally:
            lib().am_spans_free(raw)
    assert np.array_equal(o1, o2) and np.array_equal(s1, s2)
    return [x1, x2, x3, am.api.near_host(o1, s1, px.masks, px.queries)], (o1, s1)


def check_forms(px, case, hays, rows, what=None):
    forms, (so, sp) = all_forms(px, case, hays)
    assert rows_of_spans(so, sp) == rows, (what, "spans")
    for form, x in enumerate(forms):
        pairs = check_hits(x, rows, px.masks, px.queries, (what, "form", form))
    return pairs


def random_masks(rng, n, n_groups):
    return [0 if rng.random() < 0.2 else rng.getrandbits(32) & rng.getrandbits(32) & ((1 << n_groups) - 1) | (1 << rng.randrange(n_groups)) for _ in range(n)]


def random_queries(rng, n_groups, count):
    out = []
    for k in range(count):
        a = rng.randrange(n_groups)
        b = a if rng.random() < 0.25 else rng.randrange(n_groups)
        out.append((a, b, (0, 1, rng.randint(2, 6), ANY)[(k + rng.randrange(4)) % 4], rng.random() < 0.4))
    return out


# ---- 1. fragment pools: four forms, three routes, both case modes

@pytest.mark.parametrize("seed", range(3))
def test_fragment_pool_pairs(route, seed):
    rng = random.Random(9400 + seed)
    n_pairs = 0
    for i in range(8):
        needles, hays = fragment_case(rng)
        if i % 4 == 1:
            hays = hays + [""]
        if route == "table_walk" and ("" in needles or not any(needles)):
            continue                                       # the empty needle: no DFA section (the dense route reports those)
        n_groups = (1, 2, 3, 32)[i % 4]
        masks = random_masks(rng, len(needles), n_groups)
        queries = random_queries(rng, n_groups, rng.randint(1, 6))
        for case in (0, 1):
            ns = lowered(needles) if case else needles
            n_pairs += len(check_forms(Prox(ns, masks, queries, route), case, hays, ref.rows_of(ns, case, hays), (seed, i, case, ns, hays, masks, queries)))
    assert n_pairs >= 1


def test_spans_longer_than_their_needles(route):
    """K / Å under IgnoreCase: the Kelvin sign is three bytes and matches k, so gaps are measured from the span's own end."""
    needles = ["k", "å", "x"]
    hays = ["%s x %s" % (KELVIN, ANGSTROM), "x%sx%s%sK" % (KELVIN, ANGSTROM, ANGSTROM), "kk x", ""]
    rows = ref.rows_of(needles, 1, hays)
    assert rows[0] == [(0, 3, 0), (4, 1, 2), (6, 3, 1)]
    queries = [(0, 2, 1, False), (2, 1, 1, False), (2, 0, 0, False), (1, 1, ANY, False), (0, 1, 3, True)]
    pairs = check_forms(Prox(needles, [1, 2, 4], queries, route), 1, hays, rows, "kelvin")
    assert (0, 1, 1, 0, 0) in pairs and (1, 2, 1, 0, 1) in pairs and (0, 2, 3, 0, 4) in pairs


# ---- 2. seams: one-byte spans, so that the span index is the byte index

def abc_rows(hays):
    return [[(i, 1, "abc".index(ch)) for i, ch in enumerate(h)] for h in hays]


def seam_sizes(name):
    tile, word, sweep = geometry()
    return {"word - 2": word - 2, "word - 1": word - 1, "word": word, "tile - 1": tile - 1, "tile": tile, "3 * tile + 5": 3 * tile + 5, "sweep - 1": sweep - 1,
            "sweep": sweep, "2 * sweep + 3": 2 * sweep + 3}[name]


def seam_case(px, n, lead):
    """b c^n a behind `lead` c's, and its mirror image a c^n b in a second haystack that starts at the same residue: max_gap n gives one pair each, n - 1 none."""
    word = geometry()[1]
    lead2 = (lead - (lead + n + 2)) % word
    hays = ["c" * lead + "b" + "c" * n + "a", "c" * lead2 + "a" + "c" * n + "b"]
    x = px.near.near_texts(0, hays)
    pairs = check_hits(x, abc_rows(hays), px.masks, px.queries, (n, lead))
    a0, b0, a1 = lead + n + 1, lead, lead + n + 2 + lead2
    assert a1 % word == lead % word
    assert pairs == [(a0, b0, n, 0, 0), (a1, a1 + n + 1, n, 1, 0), (a1, a1 + n + 1, n, 1, 2)]
    assert x.counts.tolist() == [2, 0, 1, 0] and [int(w) for w in x.fired_words[:, 0]] == [3, 0, 2, 0]


@pytest.mark.parametrize("size", ["word - 2", "word - 1", "word", "tile - 1", "tile", "3 * tile + 5"])
def test_a_gap_across_words_and_tiles_at_every_residue(size):
    n = seam_sizes(size)
    px = Prox(ABC, ABC_MASKS, [(0, 1, n, False), (0, 1, n - 1, False), (0, 1, n, True), (0, 1, n - 1, True)])
    for lead in range(geometry()[1]):
        seam_case(px, n, lead)


@pytest.mark.parametrize("size", ["sweep - 1", "sweep", "2 * sweep + 3"])
def test_a_gap_across_the_sweeps_of_the_word_links(size):
    """The links of a row are taken in sweeps with a carry: a partner one sweep and more away comes through the carry."""
    n = seam_sizes(size)
    px = Prox(ABC, ABC_MASKS, [(0, 1, n, False), (0, 1, n - 1, False), (0, 1, n, True), (0, 1, n - 1, True)])
    for lead in (0, 1, 63):
        seam_case(px, n, lead)


@pytest.mark.parametrize("where", ["word", "3 * word", "tile", "tile + word"])
def test_partners_never_come_from_the_next_haystack(where):
    """Haystack 0 ends in b at span index k - 1, haystack 1 starts with a at index k: no pair, no fired bit, however large max_gap is."""
    tile, word, _ = geometry()
    k = {"word": word, "3 * word": 3 * word, "tile": tile, "tile + word": tile + word}[where]
    hays = ["c" * (k - 1) + "b", "a" + "c" * 5, "cc"]
    queries = [(0, 1, ANY, False), (1, 0, ANY, False), (1, 0, ANY, True), (0, 1, ANY, True)]
    px = Prox(ABC, ABC_MASKS, queries)
    x = px.near.near_texts(0, hays)
    assert check_hits(x, abc_rows(hays), px.masks, queries, where) == []
    assert x.pairs.shape == (0,) and not x.fired_words.any() and not x.counts.any() and x.offsets.tolist() == [0, 0, 0, 0]
    # ... and with a partner of its own in each haystack the seam is still not crossed
    hays = ["a" + "c" * (k - 2) + "b", "a" + "c" * 5 + "b"]
    pairs = check_hits(px.near.near_texts(0, hays), abc_rows(hays), px.masks, queries, where)
    assert [p[:3] for p in pairs if p[4] == 0] == [(0, k - 1, k - 2), (k, k + 6, 5)]


def test_fired_over_three_words_the_last_one_partial():
    hays = ["ab"] * 130
    hays[7] = hays[64] = hays[129 - 1] = "ba"
    queries = [(0, 1, 0, False), (0, 1, 0, True), (1, 0, ANY, True)]
    px = Prox(ABC, ABC_MASKS, queries)
    x = px.near.near_texts(0, hays)
    check_hits(x, abc_rows(hays), px.masks, queries)
    assert x.hay_words == 3 and int(x.fired_words[0, 2]) == 3 and int(x.fired_words[0, 0]) == 2 ** 64 - 1
    assert int(x.fired_words[1, 0]) == 2 ** 64 - 1 - (1 << 7) and int(x.fired_words[1, 1]) == 2 ** 64 - 2 and int(x.fired_words[1, 2]) == 2
    assert x.counts.tolist() == [130, 127, 3]


# ---- 3. ties and self

def test_a_tie_goes_to_the_left_across_a_word_seam():
    hays = ["bab" * 30]                                    # every a has a b touching it on both sides; the a at index 64 has its left partner in the word before
    px = Prox(ABC, ABC_MASKS, [(0, 1, 0, False), (0, 1, 0, True)])
    pairs = check_hits(px.near.near_texts(0, hays), abc_rows(hays), px.masks, px.queries)
    left = [p for p in pairs if p[4] == 0]
    assert len(left) == 30 and all(b == a - 1 and gap == 0 for a, b, gap, _, _ in left) and (64, 63, 0, 0, 0) in pairs
    assert all(b == a + 1 for a, b, _, _, q in pairs if q == 1)


def test_a_repeated_mention_is_never_its_own_partner():
    hays = ["a" * 200]
    px = Prox(ABC, ABC_MASKS, [(0, 0, 0, False), (0, 0, 0, True)])
    pairs = check_hits(px.near.near_texts(0, hays), abc_rows(hays), px.masks, px.queries)
    assert [p[:2] for p in pairs if p[4] == 0] == [(0, 1)] + [(i, i - 1) for i in range(1, 200)]
    assert [p[:2] for p in pairs if p[4] == 1] == [(i, i + 1) for i in range(199)]


# ---- 4. all 64 queries over all 32 groups

def test_sixty_four_queries_over_thirty_two_groups():
    rng = random.Random(9500)
    letters = [chr(ord("a") + i) for i in range(26)] + list("ABCDEF")
    masks = [rng.getrandbits(32) & rng.getrandbits(32) & rng.getrandbits(32) & rng.getrandbits(32) | (1 << i) for i in range(32)]      # every group has a member
    queries = [(q % 32, (q * 7 + q // 32) % 32, (0, 1, 3, 9, 40, ANY)[q % 6], q % 3 == 0) for q in range(64)]
    assert len(set(g for q in queries for g in q[:2])) == 32
    hays = ["".join(rng.choice(letters + [" ", ".", "-"]) for _ in range(rng.choice([0, 1, 63, 64, 65, 128, 200, 257]))) for _ in range(110)]
    assert 8000 <= sum(map(len, hays)) <= 16000
    px = Prox(letters, masks, queries)
    x = px.near.near_texts(0, hays)
    rows = ref.rows_of(letters, 0, hays)
    pairs = check_hits(x, rows, masks, queries)
    got = x.pairs
    keys = list(zip(got["haystack"].tolist(), got["a"].tolist(), got["query"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and len(pairs) > 2000
    assert x.counts.tolist() == np.bincount(got["query"], minlength=64).tolist() and np.count_nonzero(x.counts) >= 48


# ---- 4b. a dictionary whose needle -> mask table does not fit in LDS: k_near_bits reads it in HBM

BIG_ALPHABET = "defghijklmnopqrstuvwx"                     # 21 letters, none of a, b, c: 9261 three-letter words


def big_dictionary(n, seed):
    rng = random.Random(seed)
    words = ["".join((x, y, z)) for x in BIG_ALPHABET for y in BIG_ALPHABET for z in BIG_ALPHABET]
    rng.shuffle(words)
    assert len(set(words)) == len(words) >= n + 50
    return words[:n], words[n:n + 50], random_masks(rng, n, 4)


@pytest.mark.parametrize("beyond", [0, 1])
def test_a_mask_table_at_and_beyond_the_lds_limit(beyond):
    """kNearLdsNeedles needles: the last size whose masks are staged in LDS; one more: every mask is read from HBM.  Random masks over four groups, zeros among
    them, and tokens from all over the dictionary -- the last needle among them: a mask read at the wrong index gives other pairs."""
    n = sc.limits().near_lds_needles + beyond
    needles, strangers, masks = big_dictionary(n, 9700 + beyond)
    rng = random.Random(9710 + beyond)
    queries = random_queries(rng, 4, 6)
    hays = []
    for h in range(40):
        tokens = [needles[-1] if rng.random() < 0.02 else rng.choice(strangers) if rng.random() < 0.05 else rng.choice(needles) for _ in range(rng.randint(60, 140))]
        hays.append("".join(t + rng.choice([" ", " ", "", "  "]) for t in tokens))
    hays[3] = ""
    assert 12000 <= sum(map(len, hays)) <= 20000 and sum(h.count(needles[-1]) for h in hays) >= 20
    assert 0 in masks and len(set(masks)) >= 10
    px = Prox(needles, masks, queries)
    rows = ref.rows_of(needles, 0, hays)
    assert len(set(v for r in rows for _, _, v in r)) > 2000 and any(v == n - 1 for r in rows for _, _, v in r)
    pairs = check_forms(px, 0, hays, rows, ("mask table", n))
    assert len(pairs) > 500 and len(set(p[4] for p in pairs)) >= 4


def test_a_gap_across_a_tile_with_the_mask_table_in_hbm():
    tile = geometry()[0]
    extra, _, masks = big_dictionary(sc.limits().near_lds_needles + 1 - len(ABC), 9720)
    px = Prox(ABC + extra, ABC_MASKS + masks, [(0, 1, tile, False), (0, 1, tile - 1, False), (0, 1, tile, True), (0, 1, tile - 1, True)])
    assert len(px.masks) > sc.limits().near_lds_needles
    for lead in (0, 1, 63):
        seam_case(px, tile, lead)


# ---- 5. whole words

def test_whole_word_proximity():
    needles = ["he", "the", "said", "not"]
    hays = ["the he said not", "she said he did not", "he said; not the", "theatre he not", ""]
    masks, queries = [1, 1, 2, 4], [(0, 1, 1, False), (1, 2, ANY, True), (2, 0, 10, False)]
    px = Prox(needles, masks, queries, word_bytes=True)
    rows = wref.spans(ref.machine(needles), 0, wref.LEFTMOST_LONGEST, needles, hays, wref.DEFAULT_CLASS)
    assert rows[0] == [(0, 3, 1), (4, 2, 0), (7, 4, 2), (12, 3, 3)] and rows[1][0] == (4, 4, 2)      # he in the / she: no span, no anchor
    pairs = check_forms(px, 0, hays, rows, "words")
    assert (1, 2, 1, 0, 0) in pairs and not any(p[0] == 0 and p[4] == 0 for p in pairs)             # `the` is two bytes further from said than max_gap
    # the same texts without a class: other spans, other pairs
    plain = Prox(needles, masks, queries)
    assert check_forms(plain, 0, hays, ref.rows_of(needles, 0, hays), "plain") != pairs


# ---- 6. composition with the select

def test_the_fired_row_of_a_query_becomes_a_batch():
    rng = random.Random(9600)
    needles = ["nike", "shoe", "kids", "sale"]
    words = needles + ["and", "for", "the", "x"]
    hays = [" ".join(rng.choice(words) for _ in range(rng.randint(0, 8))) for _ in range(300)]
    masks, queries = [1, 2, 0, 4], [(0, 1, 5, False), (0, 2, 1, True), (1, 1, ANY, False)]
    px = Prox(needles, masks, queries)
    rows = ref.rows_of(needles, 0, hays)
    _, _, fired, _ = ref.near(rows, masks, queries)
    with Batch(hays) as b, Batch(hays[:-1]) as shorter, Batch(hays[:-1] + [hays[-1] + "x"]) as longer:
        x = px.near.near_batch(0, b)
        again = px.near.near_batch(0, b)
        check_hits(x, rows, masks, queries)
        assert x.pairs.tobytes() == again.pairs.tobytes() and x.fired_words.tobytes() == again.fired_words.tobytes()      # bit-identical from run to run
        for q in range(3):
            kept = [h for h in range(len(hays)) if fired[q][h]]
            assert 0 < len(kept) < len(hays)
            check_texts(b, x.select(q, batch=b), hays, kept, ("near", q))
            check_texts(b, x.select(q, batch=b, invert=True), hays, [h for h in range(len(hays)) if not fired[q][h]], ("near inverted", q))
        for bad in (lambda: x.select(3, batch=b), lambda: x.select(0, batch=shorter), lambda: x.select(0, batch=longer)):
            with pytest.raises(am.AmError) as e:
                bad()
            assert e.value.code == am.AM_ERR_INVALID
    # the front end: the pairs in readable form
    got = am.Automaton(needles).near(0, hays[:40], {"brand": ["nike"], "item": ["shoe"], "offer": ["sale"]}, [("brand", "item", 5), am.NearQuery("brand", "offer", 1, ordered=True), ("item", "item", ANY)])
    _, pairs40, _, _ = ref.near(rows[:40], masks, queries)
    assert got == ref.readable(rows[:40], pairs40, 3)


def test_calls_that_need_real_handles_are_refused():
    px = Prox(ABC, ABC_MASKS, [(0, 1, 1, False)])
    other = am.SpanTable(am.Automaton(["a", "b"]))
    out = C.c_void_p(1)
    with Batch(["abc", "cab"]) as b:
        for table, mode, word in ((px.t, am.api.SPANS_ALL, b"AM_SPANS_LEFTMOST_LONGEST"), (other, am.api.SPANS_LEFTMOST_LONGEST, b"number of needles")):
            raw = table.spans_batch(0, b, mode, raw=True)
            try:
                assert lib().am_near_spans(px.near.handle, raw, C.byref(out)) == am.AM_ERR_INVALID and not out.value and word in lib().am_last_error()
                out.value = 1
            finally:
                lib().am_spans_free(raw)


# ---- 7. empty shapes

def test_empty_shapes():
    hays = ["ab", "", "cc", "ba"]
    # no queries
    px = Prox(ABC, ABC_MASKS, [])
    for x in all_forms(px, 0, hays)[0]:
        check_hits(x, abc_rows(hays), ABC_MASKS, [])
    x = px.near.near_texts(0, hays)
    assert x.pairs.shape == (0,) and x.fired_words.shape == (0, 1) and x.counts.shape == (0,) and x.offsets.tolist() == [0] * 5
    # no haystacks
    px = Prox(ABC, ABC_MASKS, [(0, 1, ANY, False), (1, 0, 0, True)])
    for x in all_forms(px, 0, [])[0]:
        check_hits(x, [], ABC_MASKS, px.queries)
    x, (so, sp) = px.near.near_texts(1, [], spans=True)
    assert (x.n_hay, x.n_queries, x.hay_words) == (0, 2, 0) and x.offsets.tolist() == [0] and x.counts.tolist() == [0, 0] and so.tolist() == [0] and sp.shape == (0,)
    assert not lib().am_near_hits_device_data(x.handle) and not lib().am_near_hits_device_fired(x.handle)
    # haystacks without spans
    for x in all_forms(px, 0, ["", "zz", ""])[0]:
        check_hits(x, [[], [], []], ABC_MASKS, px.queries)
    # groups no needle belongs to, and a needle set whose masks are all zero
    px = Prox(ABC, ABC_MASKS, [(0, 5, ANY, False), (7, 0, ANY, False), (9, 9, ANY, False)])
    assert check_forms(px, 0, hays, abc_rows(hays)) == []
    px = Prox(ABC, [0, 0, 0], [(0, 1, ANY, False)])
    assert check_forms(px, 0, hays, abc_rows(hays)) == []
