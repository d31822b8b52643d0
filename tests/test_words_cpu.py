"""Whole-word matching (include/am.h "whole words") without a device: the definition (tests/words_reference.py) gives the examples the header quotes and equals Python's
`re` with look-arounds on random cases, the new entry points exist, are bound and refuse their arguments before any device work, and the host mirror's sequential fold
with a word class (amh_spans_fold_words / amh_substitute_fold_words) equals the definition."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers, spans_reference as ref, words_reference as wref
from tests.conftest import ROOT

NAMES = ("am_word_bytes_default", "am_span_table_create_words", "am_span_table_word_bytes", "am_count_spans_by_needle_batch", "am_count_spans_by_needle")

# (needles, text, {mode: rows}) under AM_CASE_SENSITIVE and the default class: the examples of the header block
EXAMPLES = [
    (["he", "the"], "the he she", {ref.ALL: [(0, 3, 1), (4, 2, 0)], ref.LEFTMOST_LONGEST: [(0, 3, 1), (4, 2, 0)]}),
    (["ab", "ab c"], "ab cd", {ref.ALL: [(0, 2, 0)], ref.LEFTMOST_LONGEST: [(0, 2, 0)]}),
    (["c++"], "c++ is", {ref.ALL: [(0, 3, 0)], ref.LEFTMOST_LONGEST: [(0, 3, 0)]}),
    (["ab"], "ab xab abx ab", {ref.ALL: [(0, 2, 0), (11, 2, 0)], ref.LEFTMOST_LONGEST: [(0, 2, 0), (11, 2, 0)]}),      # a needle at both ends of a haystack
    (["ab"], "ab", {ref.ALL: [(0, 2, 0)]}),
]


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_the_definition_gives_the_examples():
    for needles, text, want in EXAMPLES:
        o = oracle.Machine(needles)
        for mode, rows in want.items():
            assert wref.spans(o, 0, mode, needles, [text], wref.DEFAULT_CLASS) == [rows], (needles, text, mode)
    o = oracle.Machine(["ab", "ab c"])
    assert ref.spans(o, 0, ref.LEFTMOST_LONGEST, ["ab", "ab c"], ["ab cd"]) == [[(0, 4, 1)]]           # the plain table takes `ab c` ...
    assert wref.select_then_filter(o, 0, ["ab", "ab c"], ["ab cd"], wref.DEFAULT_CLASS) == [[]]         # ... which is no whole word: filtering afterwards leaves nothing
    o = oracle.Machine(["he", "the"])
    assert wref.counts(o, 0, ["he", "the"], ["the he she", "he"], wref.DEFAULT_CLASS) == [2, 1]
    assert wref.substitute(o, 0, ["he", "the"], ["the he she"], ["HE", "THE"], wref.DEFAULT_CLASS) == [b"THE HE she"]


def _random_case(rng):
    alphabet = rng.choice(["ab ", "ab+ ", "abc_ -", "aé "])
    needles = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 4))) for _ in range(rng.randint(1, 6))]
    hays = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 24))) for _ in range(rng.randint(1, 3))]
    return needles, hays


def test_the_definition_equals_re_with_look_arounds():
    """AM_CASE_SENSITIVE, the default class: (?<!\\w)(?:n1|n2|...)(?!\\w) with the alternatives ordered by (-length, handle), 800 random cases.  The case set holds cases
    where selecting before filtering gives another answer, so an implementation with the wrong order cannot equal the definition on it."""
    rng = random.Random(20)
    differ = 0
    for i in range(800):
        needles, hays = _random_case(rng)
        o = oracle.Machine(needles)
        got = wref.spans(o, 0, ref.LEFTMOST_LONGEST, needles, hays, wref.DEFAULT_CLASS)
        assert got == wref.regex_spans(needles, hays), (i, needles, hays)
        repl = ["<%d>" % v for v in range(len(needles))]
        assert wref.substitute(o, 0, needles, hays, repl, wref.DEFAULT_CLASS) == wref.regex_substitute(needles, hays, repl), (i, needles, hays)
        differ += got != wref.select_then_filter(o, 0, needles, hays, wref.DEFAULT_CLASS)
    assert differ >= 1, differ


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    for n in ("amh_spans_fold_words", "amh_substitute_fold_words"):
        assert hasattr(am.api.libhost(), n), n
    part = doc[doc.index("---- whole words"):doc.index("am_count_spans_by_needle(")]
    for word in ("WORD CLASS", "WHOLE WORD", "SAME haystack", "FILTER, THEN SELECT", "(?<!\\w)needle(?!\\w)", "U+212A", "0x80", "c++", "ab c"):
        assert word in part, word


def test_the_default_class():
    got = am.default_word_bytes()
    assert got == wref.flags(wref.DEFAULT_CLASS) and len(got) == 256 and sum(got) == 10 + 26 + 26 + 1 + 128
    am.api.libam().am_word_bytes_default(None)               # a null pointer is ignored
    assert am.api._word_flags(None) is None and am.api._word_flags(False) is None
    assert bytes(am.api._word_flags(True)) == got
    assert bytes(am.api._word_flags(b"az")) == wref.flags({ord("a"), ord("z")})
    assert bytes(am.api._word_flags([])) == bytes(256) and bytes(am.api._word_flags(range(256))) == b"\x01" * 256
    with pytest.raises(am.AmError):
        am.api._word_flags([256])


def test_every_argument_is_refused_before_any_device_work():
    lib = am.api.libam()
    s = am.api._Slices(["abc"])
    out = C.c_void_p(1)
    counts = np.zeros(4, np.uint64)
    one = np.ones(1, np.uint32)
    words = np.zeros(256, np.uint8)

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and word in lib.am_last_error(), (rc, lib.am_last_error())

    def refused_out(rc, word):
        refused(rc, word)
        assert not out.value
        out.value = 1

    assert lib.am_span_table_create_words(None, one.ctypes.data, one.ctypes.data, words.ctypes.data, None) == am.AM_ERR_INVALID
    refused_out(lib.am_span_table_create_words(None, one.ctypes.data, one.ctypes.data, words.ctypes.data, C.byref(out)), b"null needle ids")
    refused_out(lib.am_span_table_create_words(None, one.ctypes.data, one.ctypes.data, None, C.byref(out)), b"null needle ids")
    assert lib.am_span_table_word_bytes(None, None) == 0 and lib.am_span_table_word_bytes(None, words.ctypes.data) == 0
    refused(lib.am_count_spans_by_needle_batch(None, 0, None, counts.ctypes.data), b"null span table or batch")
    refused(lib.am_count_spans_by_needle(None, 0, None, 1, counts.ctypes.data), b"hay is null")
    refused(lib.am_count_spans_by_needle(None, 0, s.arr, 0xFFFFFFFF, counts.ctypes.data), b"too many")
    refused(lib.am_count_spans_by_needle(None, 7, s.arr, s.n, counts.ctypes.data), b"case_mode")
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    refused(lib.am_count_spans_by_needle(None, 0, bad, 1, counts.ctypes.data), b"slice with null ptr")
    refused(lib.am_count_spans_by_needle(None, 0, s.arr, s.n, counts.ctypes.data), b"null span table")
    if not _gpu():
        with pytest.raises(am.AmError) as e:
            am.Automaton(["ab"]).count_whole_words(0, ["ab"])
        assert e.value.code == am.AM_ERR_NO_DEVICE
        return
    a = am.Automaton(["ab", "å", ""])
    ids = am.ValuesTable(a)

    def create(lb, lc):
        lb, lc = np.asarray(lb, np.uint32), np.asarray(lc, np.uint32)
        rc = lib.am_span_table_create_words(ids.handle, lb.ctypes.data, lc.ctypes.data, words.ctypes.data, C.byref(out))
        if rc == am.AM_OK:
            lib.am_span_table_destroy(out)
            out.value = None
        return rc

    out.value = 1
    refused_out(lib.am_span_table_create_words(ids.handle, None, one.ctypes.data, words.ctypes.data, C.byref(out)), b"is null")
    refused_out(create([2, 2, 0], [2, 3, 0]), b"exceeds len_bytes")
    refused_out(create([2, 2, 1], [2, 1, 0]), b"exactly one")
    refused_out(create([0xFFFFFFFF, 2, 0], [1 << 30, 1, 0]), b"2^30")
    out.value = None
    assert create([2, 2, 0], [2, 1, 0]) == am.AM_OK
    for cls, t in ((None, am.SpanTable(a)), (True, am.SpanTable(a, word_bytes=True)), (b"abc", am.SpanTable(a, word_bytes=b"abc"))):
        b = C.c_void_p()
        am.api.check(lib.am_batch_upload(s.arr, s.n, C.byref(b)))
        try:
            assert t.word_bytes == (None if cls is None else bytes(am.api._word_flags(cls)))
            refused(lib.am_count_spans_by_needle_batch(t.handle, 0, None, counts.ctypes.data), b"null span table or batch")
            refused(lib.am_count_spans_by_needle_batch(None, 0, b, counts.ctypes.data), b"null span table or batch")
            refused(lib.am_count_spans_by_needle_batch(t.handle, 2, b, counts.ctypes.data), b"case_mode")
            refused(lib.am_count_spans_by_needle_batch(t.handle, 0, b, None), b"counts_out is null")
            refused(lib.am_count_spans_by_needle(t.handle, 0, s.arr, s.n, None), b"counts_out is null")
            refused(lib.am_count_spans_by_needle(t.handle, 3, s.arr, s.n, counts.ctypes.data), b"case_mode")
        finally:
            lib.am_batch_destroy(b)


def _rows(offs, spans):
    assert offs[0] == 0 and offs[-1] == len(spans)
    out = []
    for i in range(len(offs) - 1):
        part = spans[int(offs[i]):int(offs[i + 1])]
        assert (part["haystack"] == i).all()
        out.append([(int(s), int(n), int(v)) for s, n, _, v in part.tolist()])
    return out


def _triples(o, case, hays):
    triples = helpers.oracle_triples(o, case, hays)
    cols = list(zip(*triples)) if triples else ((), (), ())
    return tuple(np.array(c, dtype=t) for c, t in zip(cols, (np.uint32, np.uint64, np.uint32)))


def test_the_host_fold_gives_the_examples_without_a_device():
    for needles, text, want in EXAMPLES:
        o = oracle.Machine(needles)
        lb, lc = (x[:len(needles)] for x in am.api.needle_lengths(needles))
        for mode, rows in want.items():
            assert _rows(*am.api.spans_fold_host(0, mode, _triples(o, 0, [text]), [text], lb, lc, word_bytes=True)) == [rows], (needles, text, mode)
    needles = ["ab", "ab c"]
    o = oracle.Machine(needles)
    lb, lc = (x[:2] for x in am.api.needle_lengths(needles))
    assert _rows(*am.api.spans_fold_host(0, ref.LEFTMOST_LONGEST, _triples(o, 0, ["ab cd"]), ["ab cd"], lb, lc)) == [[(0, 4, 1)]]
    assert am.api.substitute_fold_host(0, _triples(o, 0, ["ab cd"]), ["ab cd"], lb, lc, ["X", "Y"], word_bytes=True) == [b"X cd"]
    assert am.api.substitute_fold_host(0, _triples(o, 0, ["ab cd"]), ["ab cd"], lb, lc, ["X", "Y"]) == [b"Yd"]


@pytest.mark.parametrize("cls", sorted(wref.CLASSES))
@pytest.mark.parametrize("seed", range(4))
def test_the_host_fold_equals_the_definition_on_the_fragment_pool(seed, cls):
    """The cases of test_spans_cpu.py, both case modes and span modes, four classes: the default one, a-z only (digits separate), the empty class (the bytes of the plain
    fold) and the full class (only a span that is its whole haystack)."""
    rng = random.Random(4100 + seed)
    w = wref.CLASSES[cls]
    kept = dropped = 0
    for _ in range(11):
        needles, hays = helpers.fragment_case(rng)
        o = oracle.Machine(needles)
        n = len(needles)
        lb, lc = (x[:n] for x in am.api.needle_lengths(needles))
        repl = ["", "R"] + ["<%d>" % v * 3 for v in range(2, n)]
        for case in (0, 1):
            tr = _triples(o, case, hays)
            for mode in (ref.ALL, ref.LEFTMOST_LONGEST):
                got = am.api.spans_fold_host(case, mode, tr, hays, lb, lc, word_bytes=sorted(w))
                exp = wref.spans(o, case, mode, needles, hays, w)
                assert _rows(*got) == exp, (seed, cls, needles, hays, case, mode)
                plain = am.api.spans_fold_host(case, mode, tr, hays, lb, lc)
                if cls == "empty":
                    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
                if cls == "full":
                    assert all(s == 0 and s + k == len(h.encode()) for row, h in zip(exp, hays) for s, k, _ in row)
                if mode == ref.ALL:
                    kept += len(got[1])
                    dropped += len(plain[1]) - len(got[1])
            got = am.api.substitute_fold_host(case, tr, hays, lb, lc, repl[:n], word_bytes=sorted(w))
            assert got == wref.substitute(o, case, needles, hays, repl[:n], w), (seed, cls, needles, hays, case)
    # (the pool's alphabets hold no separator of the default class: there, as under the full class, only a span that is its whole haystack is kept)
    assert (kept > 0 or cls in ("full", "default")) and (dropped > 0 or cls == "empty"), (kept, dropped)
