"""Substitute with templates on the device (am_subst_table_create_templates, k_subst_tpl_count / k_subst_tpl_pieces of csrc/am_subst.hip) against the definition.  Every
check compares the bytes and the offsets of am_substitute, am_substitute_batch, am_batch_substitute over a separately made spans result and the host mirror with what
tests/template_reference.py says -- spans_reference over the oracle plus the splice with T(v, m), or literals -- never with another path of the library (one anchor
excepted, and said there).  Shapes sit on the gather's real seams (am_substitute_geometry) and on the exclusive sum's (am_select_geometry, csrc/am_scan.hip)."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers, spans_reference as ref, template_reference as tref, words_reference as wref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

M = am.MATCH
ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}
KELVIN, ANGSTROM, SHARP_S, DOTTED_I, DOT_ABOVE = "\u212a", "\u212b", "\u1e9e", "\u0130", "\u0307"
LITS = ["", "!", "x" * 15, "y" * 16, "z" * 17, "<" + "r" * 298 + ">"]      # lengths 0, 1, 15, 16, 17, 300
SHAPES = [lambda l: [], lambda l: [M], lambda l: [l[0]], lambda l: [l[0], M, l[1]], lambda l: [M, M], lambda l: [M, l[0], M],
          lambda l: [l[0] if k % 2 == 0 else M for k in range(64)]]       # 64 segments alternating


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield ROUTES[request.param]
    am.debug_set("AM_DFA", -1)


def geometry():
    return am.api.substitute_geometry()


def templates_for(n, salt):
    """One template per handle: the seven shapes and the six literal lengths take turns."""
    return [SHAPES[(v + salt) % len(SHAPES)]([LITS[(v + salt) % len(LITS)], LITS[(v * 5 + salt + 1) % len(LITS)] + str(v)]) for v in range(n)]


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


def take(b):
    """(offsets, texts) of a batch handle through the accessors; the handle is destroyed."""
    try:
        return am.api.batch_to_bytes(b)
    finally:
        am.api.libam().am_batch_destroy(b)


def with_offsets(texts):
    texts = [_b(t) for t in texts]
    return np.cumsum([0] + [len(t) for t in texts]).astype(np.uint64), texts


def same(got, exp, what):
    assert got[0].tolist() == exp[0].tolist(), (what, "offsets", got[0].tolist()[:8], exp[0].tolist()[:8])
    for i, (g, e) in enumerate(zip(got[1], exp[1])):
        if g != e:
            k = next((j for j in range(min(len(g), len(e))) if g[j] != e[j]), min(len(g), len(e)))
            raise AssertionError((what, "haystack", i, "byte", k, g[max(0, k - 8):k + 24], e[max(0, k - 8):k + 24]))
    assert len(got[1]) == len(exp[1]), what


class Tpl:
    """An automaton on a route, its oracle twin, its span table (cls: with that word class) and its templates: handle v stands for needles[v] and has templates[v]."""

    def __init__(self, needles, templates, route=0, n=None, cls=None):
        self.needles, self.n, self.cls = list(needles), n, cls
        self.a = am.Automaton(needles)
        self.a.set_kernel(route)
        self.o = oracle.Machine(needles)
        self.t = am.SpanTable(self.a, n, word_bytes=None if cls is None else bytes(sorted(cls)))
        self.templates = list(templates)[:self.t.n_needles]
        self.r = am.SubstTable(self.t, self.templates)

    def expected(self, case, hays):
        return with_offsets(tref.substitute(self.o, case, self.needles, hays, self.templates, self.n, self.cls))

    def one_shot(self, case, hays):
        s = am.api._Slices(hays)
        b = C.c_void_p()
        am.api.check(am.api.libam().am_substitute(self.r.handle, case, s.arr, s.n, C.byref(b)))
        return take(b)

    def check(self, case, hays, exp=None, mirror=True):
        """am_substitute == am_substitute_batch == am_batch_substitute over am_spans_batch's result == the host mirror == the definition; returns the expectation."""
        exp = self.expected(case, hays) if exp is None else with_offsets(exp)
        same(self.one_shot(case, hays), exp, ("am_substitute", case))
        with Batch(hays) as b:
            same(take(self.r.substitute_batch(case, b, raw=True)), exp, ("am_substitute_batch", case))
            x = self.t.spans_batch(case, b, ref.LEFTMOST_LONGEST, raw=True)
            try:
                same(take(self.r.splice(b, x, raw=True)), exp, ("am_batch_substitute", case))
            finally:
                am.api.libam().am_spans_free(x)
        if mirror and self.cls is None:
            got = self.a.substitute_templates_host_mirror(case, hays, self.templates, n_values=self.t.n_needles)
            same(with_offsets(got), exp, ("host mirror", case))
        return exp


# ---- 1. the fragment pool

@pytest.mark.parametrize("limit", [-1, 1])
@pytest.mark.parametrize("seed", range(2))
def test_fragment_pool(route, seed, limit):
    """The pool of the span tests with the seven template shapes and literals of 0, 1, 15, 16, 17 and 300 bytes; AM_SPANS_CHAIN_LIMIT = 1 sends every chain of three to
    the doubling rounds."""
    am.debug_set("AM_SPANS_CHAIN_LIMIT", limit)
    rng = random.Random(7600 + seed)
    for i in range(8):
        needles, hays = helpers.fragment_case(rng)
        if i % 3 == 0:
            needles = needles + [needles[0]]               # a needle listed twice, with a template of its own: the smaller handle's is used
        if i % 5 == 2 and "" not in needles:
            needles = needles + [""]                       # the empty needle inserts nothing
        if "" in needles and route == ROUTES["table_walk"]:
            continue                                       # the empty needle: no DFA section
        tpls = templates_for(len(needles), seed + i)
        d = Tpl(needles, tpls, route)
        for case in (0, 1):
            exp = d.check(case, hays)
            if case == 0:
                assert exp[1] == tref.regex_substitute(needles, hays, tpls)
        if i % 4 == 1 and len(needles) > 2:
            Tpl(needles, tpls, route, n=len(needles) - 2).check(1, hays)      # n below the largest handle


# ---- 2. two algebraic anchors

def test_match_alone_is_the_identity_and_a_literal_alone_the_plain_table(route):
    rng = random.Random(31)
    words = ["tshirt", "shirt", "shirts", "hi", "his", "irt", "k", "kk"]
    hays = [" ".join(rng.choice(words + ["x", "Shirt", KELVIN, "HIS"]) for _ in range(rng.randint(0, 60))) for _ in range(120)] + ["", "k"]
    ident = Tpl(words, [[M]] * len(words), route)
    for case in (0, 1):
        exp = ident.check(case, hays)
        assert exp[1] == [_b(h) for h in hays]             # [MATCH] everywhere: the input's bytes and offsets
    repls = ["TEE", "<shirt>", "", "hello there, ", "k", "shirt", "kk", "tshirts"]
    lit = Tpl(words, [[r] for r in repls], route)
    plain = am.SubstTable(lit.t, repls)                    # the one place where two paths of the library meet: the old table and its kernel
    assert lit.r.templates and not plain.templates
    for case in (0, 1):
        exp = lit.check(case, hays)
        same(with_offsets(plain.substitute_texts(case, hays)), exp, ("the plain table", case))


# ---- 3. IgnoreCase: the text's own spelling and width

def test_ignore_case_spelling_and_widths(route):
    d = Tpl(["nike"], [["<b>", M, "</b>"]], route)
    exp = d.check(1, ["NIKE Nike nike nIkE", "ni" + KELVIN + "e"])
    assert exp[1] == [b"<b>NIKE</b> <b>Nike</b> <b>nike</b> <b>nIkE</b>", b"<b>ni" + _b(KELVIN) + b"e</b>"]
    assert d.check(0, ["NIKE Nike nike nIkE"])[1] == [b"NIKE Nike <b>nike</b> nIkE"]
    d = Tpl(["k", "i", "i" + DOT_ABOVE], [["[", M, "]"], [M, "|", M], ["{", M, "}"]], route)
    text = "kK" + KELVIN + "-" + DOTTED_I + "iI" + KELVIN + KELVIN + DOTTED_I + "i" + DOT_ABOVE + DOTTED_I + DOT_ABOVE
    exp = d.check(1, [text, KELVIN, DOTTED_I + "x", text[::-1]])
    assert exp[1][1] == b"[" + _b(KELVIN) + b"]" and exp[1][2] == _b(DOTTED_I) + b"|" + _b(DOTTED_I) + b"x"      # a span of 3 and of 2 bytes for needles of 1
    d.check(0, [text, KELVIN])
    d = Tpl(["kx", "x"], [[M, M], ["(", M, ")"]], route)                  # the same needle at the same start: 2 bytes in one haystack, 4 in the other
    exp = d.check(1, ["kx.", KELVIN + "x.", "Kx", KELVIN + "X" + "kX"])
    assert exp[1][:2] == [b"kxkx.", _b(KELVIN + "x") * 2 + b"."]
    long_needle = "kåßx" * 75                                   # 300 code points, 450 bytes; its upper-case form is 750 bytes
    upper = (KELVIN + ANGSTROM + SHARP_S + "X") * 75
    d = Tpl([long_needle, "ßx", "x"], [["<", M, ">"], [], [M, "x" * 20]], route)
    exp = d.check(1, ["ab" + upper + long_needle + "k", upper[:-1], "x" + upper])
    assert exp[1][0] == b"ab<" + _b(upper) + b"><" + _b(long_needle) + b">k"


# ---- 4. piece ends at every destination residue

@pytest.mark.parametrize("tpl", [[M], ["<", M, ">"], [M, "=" * 33, M]], ids=["match", "wrapped", "twice"])
def test_piece_ends_at_every_destination_residue(tpl):
    G, T = geometry()
    hays = ["x" * n + "|" + "y" * m for n in range(2 * G + 2) for m in range(G + 2)]      # neighbouring haystacks share store groups
    d = Tpl(["|"], [tpl])
    exp = d.check(0, hays, mirror=False)
    assert exp[1][5] == tref.expand(tpl, b"|") + b"y" * 5
    ends = set(int(x) % G for x in exp[0])
    assert ends == set(range(G)) and int(exp[0][-1]) > 2 * T


# ---- 5. MATCH sources at every alignment, tile seams, long pieces

def test_match_sources_at_every_alignment():
    """Matches that start at each source offset mod 16 -- the last bytes of the batch among them -- copied by MATCH pieces beside literals of every length mod 16: reads
    stay inside the text's and the pool's padding."""
    needles = ["<%02d>" % i for i in range(40)]
    tpls = [[chr(65 + i % 26) * (1 + (i * 3) % 19), M] if i % 2 else [M, chr(97 + i % 26) * (i % 17), M] for i in range(40)]
    rng = random.Random(3)
    hays, residues, at = [], set(), 0
    for h in range(6):
        parts = []
        for k in range(40):
            parts.append("g" * rng.randint(1, 19))
            residues.add((at + sum(map(len, parts))) % 16)
            parts.append(needles[(k * 7 + h) % 40])
        parts.append("t" * (h + 1))
        hays.append("".join(parts))
        at += len(hays[-1])
    hays.append("tail" + needles[39])                                     # the batch ends with a match: the last MATCH piece reads the batch's last bytes
    assert residues == set(range(16))
    d = Tpl(needles, tpls)
    exp = d.check(0, hays)
    assert exp[1][-1] == b"tail" + b"N" * 4 + b"<39>"
    d.check(0, [hays[-1], needles[38]])                                   # ... and with [MATCH, lit, MATCH]: a haystack that is one match


def test_pieces_that_start_just_before_a_tile_seam():
    G, T = geometry()
    d = Tpl(["|+"], [["<=>", M, "#"]])
    for seam in (T, 2 * T):
        hays = ["x" * a + "|+" + "y" * 50 for a in range(seam - G - 5, seam + 1)]      # the literal starts at a, the MATCH piece at a + 3: both within G bytes before the seam
        for h in hays[::3]:
            d.check(0, [h], mirror=False)
        d.check(0, hays, mirror=False)


def test_a_match_longer_than_three_tiles():
    G, T = geometry()
    long = "q" * (3 * T + 4) + "!"                                        # a needle -- and so a MATCH piece -- of 3T + 5 bytes
    d = Tpl([long, "#"], [[M, "-", M], []])
    exp = d.check(0, ["ab" + long + "cd", "#" + long + "#" + long[1:], "|" * 3], mirror=False)
    assert exp[1][0] == b"ab" + _b(long) + b"-" + _b(long) + b"cd" and exp[1][1] == _b(long) + b"-" + _b(long) + _b(long[1:])
    d = Tpl(["a", "b"], [[M], ["", M, ""]])
    exp = d.check(0, ["x" + "ab" * T, "ab" * (T // 2) + "a"], mirror=False)             # every live piece is one byte: T of them in a tile
    assert exp[1][0] == b"x" + b"ab" * T


# ---- 6. runs of empty pieces and empty shapes

def test_runs_of_empty_pieces():
    d = Tpl(["ab"], [[]])
    exp = d.check(0, ["x", "ab" * 5000, "y", "ab" * 3 + "c" + "ab" * 700, ""])
    assert exp[1] == [b"x", b"", b"y", b"c", b""]
    d = Tpl(["ab"], [["", M, ""]])                                        # two empty pieces around every live one
    exp = d.check(0, ["x", "ab" * 5000, "", "ab" * 3 + "c" + "ab" * 700, "ab"])
    assert exp[1][1] == b"ab" * 5000 and exp[0].tolist() == [0, 1, 10001, 10001, 11408, 11410]
    d = Tpl(["a", "b"], [[], ["", "", M, ""] * 16])                       # 64 segments, 48 of them empty
    exp = d.check(0, ["ba", "a" * 70000, "ab", "", "a" * 17, "bb"], mirror=False)
    assert exp[1] == [b"b" * 16, b"", b"b" * 16, b"", b"", b"b" * 32]


def test_nothing_to_do():
    G, T = geometry()
    d = Tpl(["needle", "other"], [["<", M, ">"], [M, M]])
    hays = ["no match here " * 700, "", "x" * (T + 3), "needl"]
    exp = d.check(0, hays)                                                # no match at all: identical bytes and offsets
    assert exp[1] == [_b(h) for h in hays]
    for case in (0, 1):
        offs, texts = d.one_shot(case, [])                                # n_hay == 0
        assert offs.tolist() == [0] and texts == []
        exp = d.check(case, ["", "", ""])                                 # empty haystacks only
        assert exp[0].tolist() == [0, 0, 0, 0]
    with Batch([]) as b:
        offs, texts = take(d.r.substitute_batch(0, b, raw=True))
        assert offs.tolist() == [0] and texts == []
    d = Tpl(["needle", "other"], [], n=0)                                 # n_needles == 0: every handle is skipped, no template, no segment
    assert not d.r.templates
    r = C.c_void_p()
    off = np.zeros(1, np.uint64)
    am.api.check(am.api.libam().am_subst_table_create_templates(d.t.handle, off.ctypes.data, None, None, None, C.byref(r)))
    try:
        hays = ["a needle and another", ""]
        s = am.api._Slices(hays)
        b = C.c_void_p()
        am.api.check(am.api.libam().am_substitute(r, 0, s.arr, s.n, C.byref(b)))
        same(take(b), with_offsets(hays), "no needle")
    finally:
        am.api.libam().am_subst_table_destroy(r)


def test_ends(route):
    d = Tpl(["ab", "abc"], [["<", M, ">"], []], route)
    exp = d.check(0, ["abxx", "xxab", "ab", "abc", "xabcab", "abab", "b"])
    assert exp[1] == [b"<ab>xx", b"xx<ab>", b"<ab>", b"", b"x<ab>", b"<ab><ab>", b"b"]
    exp = d.check(1, ["ABxx", "xxaB", "Ab", "aBC", "xabCAB", "b"])
    assert exp[1] == [b"<AB>xx", b"xx<aB>", b"<Ab>", b"", b"x<AB>", b"b"]


# ---- 7. piece numbering across the exclusive sum's seams

def scan_seams():
    """The elements one workgroup of the exclusive sum takes (am_select_geometry) and those the single workgroup over the tile sums takes per sweep: kScanThreads tiles
    (csrc/am_scan.hip)."""
    _, block = am.api.select_geometry()
    src = open(os.path.join(ROOT, "alfred-margaret_amd", "csrc", "am_scan.hip")).read()
    threads, per = (int(re.search(r"\b%s = (\d+)" % k, src).group(1)) for k in ("kScanThreads", "kScanPer"))
    assert block == threads * per
    return block, threads * block


def numbered_case(cuts):
    """Span k is `a` (k even, template of no segment) or `b` (k odd, 64 segments), every fifth one behind a dot; haystack i holds the spans [cuts[i], cuts[i + 1])."""
    full = b"<b" * 32
    hays, exp = [], []
    for lo, hi in zip(cuts, cuts[1:]):
        ks = np.arange(lo, hi)
        text = np.where(ks % 2 == 0, ord("a"), ord("b")).astype(np.uint8)
        dots = ks % 5 == 0
        pieces = np.empty(2 * len(ks), dtype=object)
        pieces[0::2] = np.where(dots, b".", b"")
        pieces[1::2] = np.where(ks % 2 == 0, b"", full)
        exp.append(b"".join(pieces.tolist()))
        hay = np.empty(2 * len(ks), dtype=object)
        hay[0::2] = np.where(dots, b".", b"")
        hay[1::2] = [bytes([c]) for c in text.tolist()]
        hays.append(b"".join(hay.tolist()))
    return hays, exp


@pytest.mark.parametrize("seam", ["block", "sweep"])
def test_piece_numbering_across_the_scan_seams(seam):
    """Templates of 0 and 64 segments alternate, so pbase is no fixed stride; the first and the last span of a haystack sit at the seam, one before and one behind it."""
    block, sweep = scan_seams()
    at = block if seam == "block" else sweep
    cuts = [0, at - 1, at, at + 1, at + 2, 2 * at + 1 if seam == "block" else at + block + 3]
    hays, exp = numbered_case(cuts)
    d = Tpl(["a", "b"], [[], ["<", M] * 32])
    if seam == "block":
        assert exp == d.expected(0, hays)[1]                              # the literal expectation is the definition's
        d.check(0, hays, exp=exp)
        return
    with Batch(hays) as b:                                                # a million spans: the batch form and the splice, held to the literal expectation
        sp = C.c_void_p()
        out = C.c_void_p()
        am.api.check(am.api.libam().am_substitute_batch(d.r.handle, 0, b, C.byref(out), C.byref(sp)))
        try:
            assert am.api.libam().am_spans_size(sp) == cuts[-1] > sweep
            same(take(out), with_offsets(exp), "am_substitute_batch")
            same(take(d.r.splice(b, sp, raw=True)), with_offsets(exp), "am_batch_substitute")
        finally:
            am.api.libam().am_spans_free(sp)


# ---- 8. the output exceeds 2^32 bytes, the input does not

def test_output_beyond_four_gib():
    """ab -> [126 bytes, MATCH] over 2^25 ab's: 2^32 bytes, then a haystack of 257 bytes without a match: offsets [0, 2^32, 2^32 + 257].  No full readback: the bytes
    around 2^32 and both ends through am_batch_read_text, the rest through am_count_batch of `ab` on the result (every MATCH piece is one)."""
    import torch
    n_ab = 2 ** 25
    lit = b"x" * 125 + b"y"
    dev = torch.device("cuda:0")
    text = torch.empty((2 * n_ab + 257 + 31,), dtype=torch.uint8, device=dev)
    text[:2 * n_ab:2] = ord("a")
    text[1:2 * n_ab:2] = ord("b")
    text[2 * n_ab:2 * n_ab + 257] = ord("z")
    text[2 * n_ab + 257:] = 0
    offs = torch.tensor([0, 2 * n_ab, 2 * n_ab + 257], dtype=torch.int64, device=dev)
    d = Tpl(["ab"], [[lit, M]])
    lib = am.api.libam()
    b, out = C.c_void_p(), C.c_void_p()
    am.api.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), 2, 2 * n_ab + 257, C.byref(b)))
    try:
        am.api.check(lib.am_substitute_batch(d.r.handle, 0, b, C.byref(out), None))
        assert am.api.batch_offsets(out).tolist() == [0, 2 ** 32, 2 ** 32 + 257]
        assert lib.am_batch_total_bytes(out) == 2 ** 32 + 257 and lib.am_batch_haystacks(out) == 2
        got = am.api.batch_read_text(out, 2 ** 32 - 256, 512)
        assert got == (lit + b"ab") * 2 + b"z" * 256, got[200:300]
        assert am.api.batch_read_text(out, 0, 300) == ((lit + b"ab") * 3)[:300]
        assert am.api.batch_read_text(out, 2 ** 32 + 200, 57) == b"z" * 57
        ab = am.Automaton(["ab"])
        counts, tot = np.zeros(2, np.uint64), C.c_uint64(0)
        am.api.check(lib.am_count_batch(ab.device, 0, out, counts.ctypes.data, C.byref(tot)))
        assert counts.tolist() == [n_ab, 0] and tot.value == n_ab
    finally:
        if out.value:
            lib.am_batch_destroy(out)
        lib.am_batch_destroy(b)
        lib.am_release_device_memory()


# ---- 9. composition and determinism

def test_whole_word_templates():
    d = Tpl(["he", "the"], [["<b>", M, "</b>"], [M]], cls=wref.DEFAULT_CLASS)
    assert d.check(0, ["the he she", "he", "(he)the", "hehe he"])[1] == [b"the <b>he</b> she", b"<b>he</b>", b"(<b>he</b>)the", b"hehe <b>he</b>"]
    assert d.check(1, ["The HE sHe"])[1] == [b"The <b>HE</b> sHe"]
    a = am.Automaton(["he"])
    assert a.highlight(0, ["the he she"], "<b>", "</b>", whole_words=True) == [b"the <b>he</b> she"]
    assert a.highlight(0, ["the he she"], "<b>", "</b>") == [b"t<b>he</b> <b>he</b> s<b>he</b>"]


def test_the_result_feeds_the_next_device_stage(route):
    rng = random.Random(99)
    words = ["tshirt", "shirt", "shirts", "hi", "his", "irt", "k", "kk"]
    tpls = [["TEE"], ["<", M, ">"], [], [M, " there, ", M], ["k"], [M, M], ["kk"], ["[", M, "]", M]]
    hays = [" ".join(rng.choice(words + ["x", "Shirt", KELVIN]) for _ in range(rng.randint(0, 40))) for _ in range(200)]
    d = Tpl(words, tpls, route)
    second = Tpl(["shirt", "k", "TEE", "there"], [["S"], [], [M, "tee" * 7], ["(", M, ")"]], route)
    lib = am.api.libam()
    for case in (0, 1):
        exp = d.expected(case, hays)
        with Batch(hays) as b:
            nb = d.r.substitute_batch(case, b, raw=True)
            try:
                counts, flags = np.zeros(len(hays), np.uint64), np.zeros(len(hays), np.uint8)
                am.api.check(lib.am_count_batch(second.a.device, case, nb, counts.ctypes.data, None))      # scanned ...
                am.api.check(lib.am_contains_any_batch(second.a.device, case, nb, flags.ctypes.data))
                want = [len(second.o.run_list(case, t)[0]) for t in exp[1]]
                assert counts.tolist() == want and flags.tolist() == [int(w > 0) for w in want] and sum(want) > 100
                rows = ref.spans(second.o, case, ref.LEFTMOST_LONGEST, second.needles, exp[1])
                snippets = [t[s:s + n] for t, row in zip(exp[1], rows) for s, n, _ in row]
                xb, xoffs, _ = second.t.extract_batch(case, nb)                                           # ... extracted ...
                assert xoffs.tolist() == np.cumsum([0] + [len(r) for r in rows]).tolist()
                same(take(xb), with_offsets(snippets), ("extract", case))
                twice = with_offsets(tref.substitute(second.o, case, second.needles, exp[1], second.templates))
                same(take(second.r.substitute_batch(case, nb, raw=True)), twice, ("twice", case))          # ... and substituted a second time
            finally:
                lib.am_batch_destroy(nb)


def test_two_runs_give_identical_bytes():
    rng = random.Random(5)
    needles = ["ab", "abc", "b", "ca", "a"]
    tpls = [["1", M], [], [M, "three", M], ["4" * 20], [M] * 7]
    hays = ["".join(rng.choice("abc ") for _ in range(rng.randint(0, 9000))) for _ in range(30)]
    d = Tpl(needles, tpls)
    for case in (0, 1):
        first, again = d.one_shot(case, hays), d.one_shot(case, hays)
        same(again, first, "again")
        same(first, d.expected(case, hays), "definition")
    assert d.one_shot(0, hays)[1] == tref.regex_substitute(needles, hays, tpls)


def test_highlight_and_mask_agree_with_the_definition():
    rng = random.Random(8)
    needles = ["nike", "adidas", "k", "i", "shoe", "åb"]
    words = needles + ["NIKE", "Nike", "ADIDAS", KELVIN, DOTTED_I, "Shoe", "x", "ÅB", "åB"]
    hays = [" ".join(rng.choice(words) for _ in range(rng.randint(0, 40))) for _ in range(60)]
    a = am.Automaton(needles)
    o = oracle.Machine(needles)
    for case in (0, 1):
        assert a.highlight(case, hays, "<b>", "</b>") == tref.substitute(o, case, needles, hays, [["<b>", M, "</b>"]] * len(needles))
        assert a.highlight(case, hays, "[", "]", whole_words=True) == tref.substitute(o, case, needles, hays, [["[", M, "]"]] * len(needles), cls=wref.DEFAULT_CLASS)
        stars = [b"*" * len(n) for n in needles]                         # one per code point of the needle
        got = a.mask(case, hays)
        assert got == tref.substitute(o, case, needles, hays, stars)
        rows = ref.spans(o, case, ref.LEFTMOST_LONGEST, needles, hays)
        assert [len(g.decode()) for g in got] == [len(h) for h in hays]  # ... which is one per code point of the MATCH: the texts keep their length in code points
        assert a.mask(case, hays, "█", whole_words=True) == tref.substitute(o, case, needles, hays, ["█" * len(n) for n in needles], cls=wref.DEFAULT_CLASS)
        assert sum(len(r) for r in rows) > 200
    assert am.Automaton(["nike"]).highlight(am.IGNORE_CASE, ["NIKE shoe"], "<b>", "</b>") == [b"<b>NIKE</b> shoe"]
