"""am_span_table_* / am_spans* (include/am.h "match spans"): the definition (tests/spans_reference.py) gives the issue's examples, the entry points exist, are bound and
check their arguments before any device work, and the host mirror's sequential fold (amh_spans_fold, no device) equals the definition.

am_needle_ids_create needs a device, so on a box without one no span table can be made: there the checks of the run entry points are seen with a null table (it is
checked last), and the front end reports AM_ERR_NO_DEVICE."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers, spans_reference as ref
from tests.conftest import ROOT

NAMES = ("am_span_table_create", "am_span_table_destroy", "am_spans_batch", "am_spans", "am_spans_size", "am_spans_haystacks", "am_spans_offsets", "am_spans_data",
         "am_spans_device_offsets", "am_spans_device_data", "am_spans_rounds", "am_spans_free")

A_RING, KELVIN, ANGSTROM = "\u00c5", "\u212a", "\u212b"

# the issue's table: (needles, values, text, case, {mode: [(start, len, handle)]})
TABLE = [
    (["b", "abc", "abcd"], None, "abcd", 0, {ref.ALL: [(1, 1, 0), (0, 3, 1), (0, 4, 2)], ref.LEFTMOST_LONGEST: [(0, 4, 2)]}),
    (["abcdefgh", "cd", "gh", "hi"], None, "abcdefghi xcd", 0, {ref.LEFTMOST_LONGEST: [(0, 8, 0), (11, 2, 1)]}),
    (["a", "aa", "aaa"], None, "aaaaaaa", 0, {ref.LEFTMOST_LONGEST: [(0, 3, 2), (3, 3, 2), (6, 1, 0)]}),
    (["ab", "ab"], None, "abab", 0, {ref.ALL: [(0, 2, 1), (0, 2, 0), (2, 2, 1), (2, 2, 0)], ref.LEFTMOST_LONGEST: [(0, 2, 0), (2, 2, 0)]}),
    (["", "a"], None, "banana", 0, {ref.ALL: [(1, 1, 1), (2, 0, 0), (3, 1, 1), (4, 0, 0), (5, 1, 1), (6, 0, 0)], ref.LEFTMOST_LONGEST: [(1, 1, 1), (3, 1, 1), (5, 1, 1)]}),
    (["åb"], None, ANGSTROM + "B" + A_RING + "b", 1, {ref.ALL: [(0, 4, 0), (4, 3, 0)], ref.LEFTMOST_LONGEST: [(0, 4, 0), (4, 3, 0)]}),
]


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_the_definition_gives_the_examples():
    for needles, values, text, case, want in TABLE:
        o = oracle.Machine(needles, values)
        for mode, rows in want.items():
            assert ref.spans(o, case, mode, needles, [text]) == [rows], (needles, text, mode)


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    assert "global: am_*;" in open(os.path.join(ROOT, "alfred-margaret_amd", "csrc", "libam.map")).read()
    assert re.search(r"typedef struct am_span \{ uint64_t start; uint64_t len; uint32_t haystack; uint32_t needle; \} am_span;", src)
    assert re.search(r"#define AM_SPANS_ALL 0\b", src) and re.search(r"#define AM_SPANS_LEFTMOST_LONGEST 1\b", src)
    assert (am.api.SPANS_ALL, am.api.SPANS_LEFTMOST_LONGEST) == (0, 1)
    for n in ("amh_spans_fold", "amh_spans"):
        assert hasattr(am.api.libhost(), n), n
    assert "AM_SPANS_CHAIN_LIMIT" in am.api.DEBUG_SWITCHES
    am.debug_set("AM_SPANS_CHAIN_LIMIT", 1)
    am.debug_set("AM_SPANS_CHAIN_LIMIT", -1)
    assert len(am.api.DEBUG_ABI) == 14                     # no new am_debug_* symbol


def test_header_block_states_the_semantics():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    part = doc[doc.index("---- match spans"):doc.index("am_spans_free(")]
    for cite in ("Automaton.hs:442-553", "Replacer.hs:264-274", "Utf8.hs:256-276"):
        assert cite in part, cite
    for word in ("ORDER", "TIE-BREAK", "SKIPPED", "ZERO-LENGTH", "WORKSPACE", "NOT bounded", "bit-identical", "AM_SPANS_CHAIN_LIMIT"):
        assert word in part, word
    for phrase in ("the largest len", "the smallest handle", "start + len is non-decreasing", "12 bytes per record", "24 bytes per span", "29 bytes per distinct start"):
        assert phrase in part, phrase


def test_am_span_layout():
    d = am.api.SPAN_DTYPE
    assert d.itemsize == 24 and [d.fields[n][1] for n in ("start", "len", "haystack", "needle")] == [0, 8, 16, 20]
    assert d.itemsize == am.api.PRIO_MATCH_DTYPE.itemsize and [am.api.PRIO_MATCH_DTYPE.fields[n][1] for n in ("start", "len", "haystack", "payload")] == [0, 8, 16, 20]


def test_every_argument_is_refused_before_any_device_work():
    lib = am.api.libam()
    s = am.api._Slices(["abc"])
    out = C.c_void_p(1)

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and not out.value and word in lib.am_last_error(), (rc, lib.am_last_error())
        out.value = 1

    assert lib.am_spans(None, 0, 0, s.arr, s.n, None) == am.AM_ERR_INVALID
    refused(lib.am_spans(None, 0, 0, None, 1, C.byref(out)), b"hay is null")
    refused(lib.am_spans(None, 0, 0, s.arr, 0xFFFFFFFF, C.byref(out)), b"too many")
    refused(lib.am_spans(None, 7, 0, s.arr, s.n, C.byref(out)), b"case_mode")
    refused(lib.am_spans(None, 0, 2, s.arr, s.n, C.byref(out)), b"mode must be AM_SPANS")
    refused(lib.am_spans(None, 1, -1, s.arr, s.n, C.byref(out)), b"mode must be AM_SPANS")
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    refused(lib.am_spans(None, 0, 0, bad, 1, C.byref(out)), b"slice with null ptr")
    refused(lib.am_spans(None, 0, 0, s.arr, s.n, C.byref(out)), b"null span table")
    refused(lib.am_spans(None, 1, 1, s.arr, 0, C.byref(out)), b"null span table")
    assert lib.am_spans_batch(None, 0, 0, None, None) == am.AM_ERR_INVALID
    refused(lib.am_spans_batch(None, 3, 0, None, C.byref(out)), b"case_mode")
    refused(lib.am_spans_batch(None, 0, 5, None, C.byref(out)), b"mode must be AM_SPANS")
    refused(lib.am_spans_batch(None, 0, 0, None, C.byref(out)), b"null span table or batch")
    one = np.ones(1, np.uint32)
    assert lib.am_span_table_create(None, one.ctypes.data, one.ctypes.data, None) == am.AM_ERR_INVALID
    refused(lib.am_span_table_create(None, one.ctypes.data, one.ctypes.data, C.byref(out)), b"null needle ids")
    # the accessors of a null result
    assert lib.am_spans_size(None) == 0 and lib.am_spans_haystacks(None) == 0 and lib.am_spans_rounds(None) == 0
    assert not lib.am_spans_offsets(None) and not lib.am_spans_data(None)
    assert not lib.am_spans_device_offsets(None) and not lib.am_spans_device_data(None)
    lib.am_spans_free(None)
    lib.am_span_table_destroy(None)
    if not _gpu():
        return
    a = am.Automaton(["ab", "å", ""])
    ids = am.ValuesTable(a)

    def create(lb, lc):
        lb, lc = np.asarray(lb, np.uint32), np.asarray(lc, np.uint32)
        rc = lib.am_span_table_create(ids.handle, lb.ctypes.data, lc.ctypes.data, C.byref(out))
        if rc == am.AM_OK:
            lib.am_span_table_destroy(out)
            out.value = None
        return rc

    refused(lib.am_span_table_create(ids.handle, None, one.ctypes.data, C.byref(out)), b"is null")
    refused(lib.am_span_table_create(ids.handle, one.ctypes.data, None, C.byref(out)), b"is null")
    refused(create([2, 2, 0], [2, 3, 0]), b"exceeds len_bytes")
    refused(create([2, 2, 1], [2, 1, 0]), b"exactly one")
    refused(create([2, 2, 0], [2, 1, 1]), b"exceeds len_bytes")      # (0 bytes, 1 code point)
    refused(create([2, 2, 0], [0, 1, 0]), b"exactly one")
    refused(create([0xFFFFFFFF, 2, 0], [1 << 30, 1, 0]), b"2^30")
    out.value = None
    assert create([0xFFFFFFFF, 2, 0], [(1 << 30) - 1, 1, 0]) == am.AM_OK
    assert create([2, 2, 0], [2, 1, 0]) == am.AM_OK
    t = am.SpanTable(a)
    b = C.c_void_p()
    am.api.check(lib.am_batch_upload(s.arr, s.n, C.byref(b)))
    try:
        out.value = 1
        refused(lib.am_spans_batch(None, 0, 0, b, C.byref(out)), b"null span table or batch")
        refused(lib.am_spans_batch(t.handle, 0, 0, None, C.byref(out)), b"null span table or batch")
        refused(lib.am_spans_batch(t.handle, 2, 0, b, C.byref(out)), b"case_mode")
        refused(lib.am_spans_batch(t.handle, 0, 2, b, C.byref(out)), b"mode must be AM_SPANS")
        assert lib.am_spans_batch(t.handle, 0, 0, b, None) == am.AM_ERR_INVALID
        refused(lib.am_spans(t.handle, 0, 0, None, 1, C.byref(out)), b"hay is null")
    finally:
        lib.am_batch_destroy(b)


def test_without_a_gpu_the_front_end_reports_no_device():
    a = am.Automaton(["b", "abc", "abcd"])
    if _gpu():
        offs, spans = a.spans(0, ["abcd"], leftmost_longest=True)
        assert offs.tolist() == [0, 1] and spans.tolist() == [(0, 4, 0, 2)]
        return
    for call in (lambda: a.spans(0, ["abcd"]), lambda: a.spans(1, ["abcd"], True), lambda: am.SpanTable(a), lambda: a.spans_host_mirror(0, ["abcd"])):
        with pytest.raises(am.AmError) as e:
            call()
        assert e.value.code == am.AM_ERR_NO_DEVICE


def _rows(offs, spans):
    assert offs[0] == 0 and offs[-1] == len(spans)
    out = []
    for i in range(len(offs) - 1):
        part = spans[int(offs[i]):int(offs[i + 1])]
        assert (part["haystack"] == i).all()
        out.append([(int(s), int(n), int(v)) for s, n, _, v in part.tolist()])
    return out


def _fold(case, mode, o, hays, lengths):
    """amh_spans_fold over the oracle's fold steps, as rows of (start, len, handle)."""
    triples = helpers.oracle_triples(o, case, hays)
    cols = list(zip(*triples)) if triples else ((), (), ())
    arrays = tuple(np.array(c, dtype=t) for c, t in zip(cols, (np.uint32, np.uint64, np.uint32)))
    return _rows(*am.api.spans_fold_host(case, mode, arrays, hays, lengths[0], lengths[1]))


def _lengths(handle_needles, n=None):
    return am.api.needle_lengths(handle_needles, n)


def test_the_host_fold_gives_the_examples_without_a_device():
    for needles, values, text, case, want in TABLE:
        o = oracle.Machine(needles, values)
        lb, lc = _lengths(needles)
        for mode, rows in want.items():
            assert _fold(case, mode, o, [text], (lb[:len(needles)], lc[:len(needles)])) == [rows], (needles, text, mode)


@pytest.mark.parametrize("seed", range(4))
def test_the_host_fold_equals_the_definition_on_the_fragment_pool(seed):
    rng = random.Random(4100 + seed)
    for _ in range(11):
        needles, hays = helpers.fragment_case(rng)
        o = oracle.Machine(needles)
        for n in (len(needles), max(0, len(needles) - 2)):                # n below the largest handle: the last two needles are skipped
            lb, lc = _lengths(needles, n)
            for case in (0, 1):
                for mode in (ref.ALL, ref.LEFTMOST_LONGEST):
                    assert _fold(case, mode, o, hays, (lb[:n], lc[:n])) == ref.spans(o, case, mode, needles, hays, n), (seed, needles, hays, n, case, mode)


def test_the_host_fold_with_shared_and_duplicate_handles():
    """A needle under two handles reports under both (list order decides ALL, the smallest handle wins leftmost-longest); two needles of one length under ONE handle
    add into it; handles beyond n are skipped."""
    needles = ["ab", "ab", "cd", "abcd", "b", "xyz"]
    values = [0, 1, 0, 2, 3, 9]
    by_handle = ["ab", "ab", "abcd", "b"]                                 # handle -> a needle of its length ("ab" and "cd" share handle 0)
    hays = ["abcdab", "", "xyzcdcdab", "bbabxyz"]
    o = oracle.Machine(needles, values)
    for n in (4, 3, 1, 0):
        lb, lc = _lengths(by_handle, n)
        for case in (0, 1):
            for mode in (ref.ALL, ref.LEFTMOST_LONGEST):
                got = _fold(case, mode, o, hays, (lb[:n], lc[:n]))
                assert got == ref.spans(o, case, mode, by_handle, hays, n), (n, case, mode)
                if n == 0:
                    assert got == [[], [], [], []]
    lb, lc = _lengths(by_handle)
    assert _fold(0, ref.ALL, o, ["abcd"], (lb[:4], lc[:4]))[0][:2] in ([(0, 2, 0), (0, 2, 1)], [(0, 2, 1), (0, 2, 0)])
    assert _fold(0, ref.LEFTMOST_LONGEST, o, ["ab cd"], (lb[:4], lc[:4])) == [[(0, 2, 0), (3, 2, 0)]]
