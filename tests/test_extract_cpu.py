"""am_fragments_from_spans / am_extract_batch / am_extract (include/am.h "extract") without a device: the host mirror's sequential definition (amh_extract_fold,
host/spans.hpp extractFold) equals tests/extract_reference.py -- the definition in Python, a byte at a time -- and Python's `re` over str, whose slices count code
points; the merge rule at its edges; the entry points exist, are bound and check their arguments before any device work.

No span table can be made without a device (am_needle_ids_create needs one): the spans of the folds are the definition's own rows (tests/spans_reference.py over the
oracle), and the argument checks are seen with null handles, which every entry point checks last."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import extract_reference as xref, helpers, spans_reference as ref, words_reference as wref
from tests.conftest import ROOT

NAMES = ("am_fragments_from_spans", "am_extract_batch", "am_extract")
KELVIN = "\u212a"
WIDTHS = (0, 1, 2, 5, 1000)


def csr(rows):
    """(offsets, SPAN_DTYPE rows) of per-haystack lists of (start, len, handle)."""
    offs = np.zeros(len(rows) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    flat = np.zeros(int(offs[-1]), am.api.SPAN_DTYPE)
    k = 0
    for h, r in enumerate(rows):
        for s in r:
            flat[k] = (s[0], s[1], h, s[2] if len(s) > 2 else 0)
            k += 1
    return offs, flat


def fold(hays, rows, before, after, merged):
    """amh_extract_fold as (offsets, [(start, len)])."""
    offs, frags = am.api.extract_fold_host(*csr(rows), hays, before, after, merged)
    return offs.tolist(), [(int(f["start"]), int(f["len"])) for f in frags]


def check_fold(hays, rows, before, after, mode):
    want_offs, want, _ = xref.fragments(hays, rows, before, after, mode)
    assert fold(hays, rows, before, after, mode == xref.MERGED) == (want_offs, want), (hays, rows, before, after, mode)
    return want


def test_the_header_example_and_hand_written_cases():
    needles, hay = ["he", "the"], "the he she"
    o = oracle.Machine(needles)
    every = ref.spans(o, 0, ref.ALL, needles, [hay])
    ll = ref.spans(o, 0, ref.LEFTMOST_LONGEST, needles, [hay])
    assert [s[:2] for s in every[0]] == [(0, 3), (1, 2), (4, 2), (8, 2)] and [s[:2] for s in ll[0]] == [(0, 3), (4, 2), (8, 2)]
    assert check_fold([hay], every, 0, 0, xref.EACH) == [(0, 3), (1, 2), (4, 2), (8, 2)]
    assert check_fold([hay], every, 1, 1, xref.EACH) == [(0, 4), (0, 4), (3, 4), (7, 3)]
    assert check_fold([hay], ll, 2, 0, xref.EACH) == [(0, 3), (2, 4), (6, 4)]
    assert check_fold([hay], ll, 1000, 1000, xref.EACH) == [(0, 10)] * 3
    assert check_fold([hay], ll, 0, 0, xref.MERGED) == [(0, 3), (4, 2), (8, 2)]
    assert check_fold([hay], ll, 0, 1, xref.MERGED) == [(0, 7), (8, 2)]
    assert check_fold([hay], ll, 1, 1, xref.MERGED) == [(0, 10)]
    for b in WIDTHS:
        for a in WIDTHS:
            check_fold([hay], every, b, a, xref.EACH)
            check_fold([hay], ll, b, a, xref.EACH)
            check_fold([hay], ll, b, a, xref.MERGED)
            assert xref.regex_snippets(needles, [hay], b, a) == [xref.fragments([hay], ll, b, a, xref.EACH)[2]]


def test_code_points_of_one_to_four_bytes():
    left, right = "aé" + KELVIN + "\U0001f600", "\U0001f600" + KELVIN + "éa"
    hay = left + "x" + right
    rows = [[(10, 1, 0)]]
    want = {0: (10, 1), 1: (6, 9), 2: (3, 15), 3: (1, 19), 4: (0, 21), 5: (0, 21), 1000: (0, 21)}
    for n, w in want.items():
        assert check_fold([hay], rows, n, n, xref.EACH) == [w], n
        assert xref.regex_snippets(["x"], [hay], n, n) == [[hay.encode()[w[0]:w[0] + w[1]]]]
    # the Kelvin sign matched by k under AM_IGNORE_CASE: the span is three bytes
    o = oracle.Machine(["k"])
    hay = "é" + KELVIN + "éké"
    rows = ref.spans(o, 1, ref.LEFTMOST_LONGEST, ["k"], [hay])
    assert [s[:2] for s in rows[0]] == [(2, 3), (7, 1)]
    assert check_fold([hay], rows, 1, 1, xref.EACH) == [(0, 7), (5, 5)]
    assert check_fold([hay], rows, 1, 1, xref.MERGED) == [(0, 10)]
    assert check_fold([hay], rows, 0, 0, xref.MERGED) == [(2, 3), (7, 1)]
    for b in WIDTHS:
        for a in WIDTHS:
            check_fold([hay], rows, b, a, xref.EACH)
            check_fold([hay], rows, b, a, xref.MERGED)


def test_haystacks_without_a_start_byte_and_empty_haystacks():
    hays = [b"\x80" * 40, b"", b"\x80" * 17 + b"x" + b"\xbf" * 32]
    rows = [[(0, 0, 0), (20, 1, 0), (40, 0, 0)], [(0, 0, 0)], [(17, 1, 0)]]
    for b in WIDTHS:
        for a in WIDTHS:
            got = check_fold(hays, rows, b, a, xref.EACH)
            if b and a:
                assert got == [(0, 40)] * 3 + [(0, 0), (0, 50)]
    assert check_fold(hays, rows, 0, 0, xref.EACH) == [(0, 0), (20, 1), (40, 0), (0, 0), (17, 1)]
    assert fold([], [], 3, 3, True) == ([0], []) and fold([], [], 0, 0, False) == ([0], [])
    assert fold(["ab", "", "c"], [[], [], []], 2, 2, True) == ([0, 0, 0, 0], [])


def test_zero_length_spans_of_the_empty_needle():
    needles, hays = ["", "b"], ["abc", "", "é"]
    o = oracle.Machine(needles)
    rows = ref.spans(o, 0, ref.ALL, needles, hays)
    zero = [s[:2] for r in rows for s in r if s[1] == 0]
    assert zero and (1, 1) in [s[:2] for s in rows[0]]
    assert check_fold(hays, rows, 0, 0, xref.EACH) == [s[:2] for r in rows for s in r]         # zero-length fragments are kept
    for b in WIDTHS:
        for a in WIDTHS:
            check_fold(hays, rows, b, a, xref.EACH)


def test_the_merge_rule():
    hay = "ab..ab.ab"
    rows = [[(0, 2, 0), (4, 2, 0), (7, 2, 0)]]
    assert check_fold([hay], rows, 0, 0, xref.MERGED) == [(0, 2), (4, 2), (7, 2)]
    assert check_fold([hay], rows, 1, 0, xref.MERGED) == [(0, 2), (3, 6)]                      # [0, 2) | [3, 6) and [6, 9): 3 > 2 separates, 6 <= 6 joins
    # touching windows join, a gap of one byte separates
    assert xref.merged("ab.ab", [(0, 2), (3, 2)], 0, 1) == [(0, 5)]                             # [0, 3) and [3, 5): ws == we
    assert xref.merged("ab..ab", [(0, 2), (4, 2)], 0, 1) == [(0, 3), (4, 2)]                    # [0, 3) and [4, 6): one byte apart
    assert check_fold(["ab.ab"], [[(0, 2, 0), (3, 2, 0)]], 0, 1, xref.MERGED) == [(0, 5)]
    assert check_fold(["ab..ab"], [[(0, 2, 0), (4, 2, 0)]], 0, 1, xref.MERGED) == [(0, 3), (4, 2)]
    assert check_fold(["ab..ab"], [[(0, 2, 0), (4, 2, 0)]], 1, 1, xref.MERGED) == [(0, 6)]
    # a haystack that ends in a match, followed by one that begins with a match: two pieces, however wide the windows are
    hays = ["..ab", "ab..", "", "ab", "ab"]
    rows = [[(2, 2, 0)], [(0, 2, 0)], [], [(0, 2, 0)], [(0, 2, 0)]]
    want_offs, want, texts = xref.fragments(hays, rows, 1000, 1000, xref.MERGED)
    assert (want_offs, want) == ([0, 1, 2, 2, 3, 4], [(0, 4), (0, 4), (0, 2), (0, 2)]) and texts == [b"..ab", b"ab..", b"ab", b"ab"]
    assert fold(hays, rows, 1000, 1000, True) == (want_offs, want)
    with pytest.raises(am.AmError) as e:
        fold(["abcd"], [[(0, 3, 0), (1, 2, 0)]], 0, 0, True)                                   # overlapping rows: not a leftmost-longest result
    assert e.value.code == am.AM_ERR_INVALID
    with pytest.raises(am.AmError):
        fold(["ab"], [[(1, 2, 0)]], 0, 0, False)                                               # a span that leaves its haystack


@pytest.mark.parametrize("seed", range(4))
def test_the_host_fold_equals_the_definition_on_the_fragment_pool(seed):
    rng = random.Random(7300 + seed)
    for i in range(10):
        needles, hays = helpers.fragment_case(rng)
        o = oracle.Machine(needles)
        b, a = rng.choice(WIDTHS), rng.choice(WIDTHS)
        for case in (0, 1):
            every = ref.spans(o, case, ref.ALL, needles, hays)
            ll = ref.spans(o, case, ref.LEFTMOST_LONGEST, needles, hays)
            check_fold(hays, every, b, a, xref.EACH)
            check_fold(hays, ll, b, a, xref.EACH)
            check_fold(hays, ll, b, a, xref.MERGED)
            check_fold(hays, ll, 1, 2, xref.MERGED)
            if case == 0:
                assert xref.regex_snippets(needles, hays, b, a) == [xref.fragments([h], [r], b, a, xref.EACH)[2] for h, r in zip(hays, ll)], (needles, hays, b, a)
        words = wref.spans(o, 0, ref.LEFTMOST_LONGEST, needles, hays, wref.DEFAULT_CLASS)
        check_fold(hays, words, b, a, xref.MERGED)
        assert xref.regex_snippets(needles, hays, b, a, whole_words=True) == [xref.fragments([h], [r], b, a, xref.EACH)[2] for h, r in zip(hays, words)], (needles, hays)


@pytest.mark.parametrize("seed", range(3))
def test_the_host_fold_equals_the_definition_on_random_bytes(seed):
    """Not valid UTF-8: the definition is on bytes.  Random spans (ascending and disjoint for MERGED) over bytes drawn from START and continuation bytes alike."""
    rng = random.Random(7400 + seed)
    for _ in range(60):
        hays, every, ll = [], [], []
        for _ in range(rng.randint(1, 4)):
            n = rng.randint(0, 70)
            hays.append(bytes(rng.choice((0x41, 0x80, 0xBF, 0xC3, 0xE2, 0xF0, 0x20)) for _ in range(n)))
            cuts = sorted(rng.randint(0, n) for _ in range(2 * rng.randint(0, 5)))
            ll.append([(cuts[k], cuts[k + 1] - cuts[k], 0) for k in range(0, len(cuts), 2)])
            every.append([(s, rng.randint(0, n - s), 0) for s in (rng.randint(0, n) for _ in range(rng.randint(0, 5)))])
        b, a = rng.choice(WIDTHS + (3, 16, 17)), rng.choice(WIDTHS + (3, 16, 17))
        check_fold(hays, every, b, a, xref.EACH)
        check_fold(hays, ll, b, a, xref.EACH)
        check_fold(hays, ll, b, a, xref.MERGED)


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    assert re.search(r"#define AM_EXTRACT_EACH 0\s", src) and re.search(r"#define AM_EXTRACT_MERGED 1\s", src)
    assert (am.api.EXTRACT_EACH, am.api.EXTRACT_MERGED) == (0, 1)
    assert hasattr(am.api.libhost(), "amh_extract_fold")
    assert len(am.api.DEBUG_ABI) == 14                     # no new am_debug_* symbol
    for n in ("extract_batch", "fragments_from_spans"):
        assert hasattr(am.api.SpanTable, n), n
    assert hasattr(am.Automaton, "extract") and hasattr(am.api, "extract_fold_host")
    build_py = open(os.path.join(ROOT, "alfred-margaret_amd", "build.py")).read()
    assert '"am_extract.cpp"' in build_py and '"am_extract.hip"' in build_py
    part = doc[doc.index("---- extract"):doc.index("am_extract(const")]
    for phrase in ("(b & 0xC0) != 0x80", "NEVER\n * LEAVE THE HAYSTACK", "ZERO-LENGTH", "TOUCHING", "ws_i <= we_{i-1}", "16 bytes per fragment and 8 per haystack",
                   "SOURCE coordinates", "AM_ERR_UNSUPPORTED"):
        assert phrase in part, phrase


def test_every_argument_is_refused_before_any_device_work():
    """Null pointers, a mode of 2, a case_mode of 2 and n_hay >= 0xFFFFFFFF answer AM_ERR_INVALID on a machine without a device: they come before ensure_runtime()."""
    lib = am.api.libam()
    s = am.api._Slices(["abc"])
    out, fr = C.c_void_p(1), C.c_void_p(1)
    EACH, MERGED, ALL, LL = am.api.EXTRACT_EACH, am.api.EXTRACT_MERGED, am.api.SPANS_ALL, am.api.SPANS_LEFTMOST_LONGEST

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and not out.value and word in lib.am_last_error(), (rc, out.value, lib.am_last_error())
        out.value = 1

    # am_fragments_from_spans
    assert lib.am_fragments_from_spans(None, None, 1, 1, EACH, None) == am.AM_ERR_INVALID
    refused(lib.am_fragments_from_spans(None, None, 1, 1, EACH, C.byref(out)), b"null batch or spans")
    refused(lib.am_fragments_from_spans(None, None, 1, 1, MERGED, C.byref(out)), b"null batch or spans")
    refused(lib.am_fragments_from_spans(None, None, 1, 1, 2, C.byref(out)), b"AM_EXTRACT_EACH or AM_EXTRACT_MERGED")
    refused(lib.am_fragments_from_spans(None, None, 1, 1, -1, C.byref(out)), b"AM_EXTRACT_EACH or AM_EXTRACT_MERGED")
    # am_extract_batch
    assert lib.am_extract_batch(None, 0, LL, 1, 1, EACH, None, None, None) == am.AM_ERR_INVALID
    assert lib.am_extract_batch(None, 0, LL, 1, 1, EACH, None, None, C.byref(fr)) == am.AM_ERR_INVALID and not fr.value
    for case, spans_mode, mode, word in ((2, LL, EACH, b"case_mode"), (0, 2, EACH, b"spans_mode"), (0, LL, 2, b"AM_EXTRACT_EACH or AM_EXTRACT_MERGED"),
                                         (1, ALL, MERGED, b"AM_SPANS_LEFTMOST_LONGEST spans only"), (0, LL, MERGED, b"null span table or batch"),
                                         (1, ALL, EACH, b"null span table or batch")):
        fr.value = 1
        refused(lib.am_extract_batch(None, case, spans_mode, 1, 1, mode, None, C.byref(out), C.byref(fr)), word)
        assert not fr.value
        refused(lib.am_extract_batch(None, case, spans_mode, 1, 1, mode, None, C.byref(out), None), word)
    # am_extract
    assert lib.am_extract(None, 0, LL, 1, 1, EACH, s.arr, s.n, None, None) == am.AM_ERR_INVALID
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    for case, spans_mode, mode, hay, n_hay, word in ((0, LL, EACH, None, 1, b"hay is null"), (0, LL, EACH, s.arr, 0xFFFFFFFF, b"too many"),
                                                     (0, LL, EACH, s.arr, 1 << 40, b"too many"), (0, LL, EACH, bad, 1, b"slice with null ptr"),
                                                     (2, LL, EACH, s.arr, s.n, b"case_mode"), (0, 2, EACH, s.arr, s.n, b"spans_mode"),
                                                     (0, LL, 2, s.arr, s.n, b"AM_EXTRACT_EACH or AM_EXTRACT_MERGED"),
                                                     (0, ALL, MERGED, s.arr, s.n, b"AM_SPANS_LEFTMOST_LONGEST spans only"),
                                                     (0, LL, MERGED, s.arr, s.n, b"null span table"), (1, ALL, EACH, s.arr, 0, b"null span table")):
        fr.value = 1
        refused(lib.am_extract(None, case, spans_mode, 1, 1, mode, hay, n_hay, C.byref(out), C.byref(fr)), word)
        assert not fr.value
        refused(lib.am_extract(None, case, spans_mode, 1, 1, mode, hay, n_hay, C.byref(out), None), word)


def test_without_a_gpu_the_front_end_reports_no_device():
    import torch
    a = am.Automaton(["he", "the"])
    if torch.cuda.is_available():
        assert a.extract(0, ["the he she", ""], 1, 1) == [[b"the ", b" he ", b" he"], []]
        return
    with pytest.raises(am.AmError) as e:
        a.extract(0, ["the he she"], 1, 1)
    assert e.value.code == am.AM_ERR_NO_DEVICE
