"""Per-needle exact case (include/am.h "exact case") without a device: the definition (tests/cased_reference.py) gives the examples the header quotes, the new entry
points exist, are bound and refuse their arguments before any device work, the host mirror's sequential fold with spellings (amh_spans_fold_cased /
amh_substitute_fold_cased) equals the definition on the examples and on 300 seeded random cases, and the comparator of csrc/am_cased.h equals memcmp in a stand-alone
program, plain and under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import cased_reference as cref, helpers, spans_reference as ref, words_reference as wref
from tests.conftest import ROOT

NAMES = ("am_span_table_create_cased", "am_span_table_check_exact", "am_span_table_exact")
MODES = (ref.ALL, ref.LEFTMOST_LONGEST)


def _gpu():
    import torch
    return torch.cuda.is_available()


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


def test_the_definition_gives_the_examples():
    for needles, exact, text, want in cref.EXAMPLES:
        o = oracle.Machine(needles)
        for mode, rows in want.items():
            assert cref.spans(o, 1, mode, needles, [text], exact) == [rows], (needles, exact, text, mode)
    needles, exact = ["ab c", "ab"], ["AB C", None]
    o = oracle.Machine(needles)
    assert ref.spans(o, 1, ref.LEFTMOST_LONGEST, needles, ["ab c"]) == [[(0, 4, 0)]]               # the plain table selects `ab c` ...
    assert cref.select_then_filter(o, 1, needles, ["ab c"], exact) == [[]]                          # ... which is not spelled AB C: filtering afterwards leaves nothing
    needles, exact = ["us", "apple", "nike"], ["US", "Apple", None]
    o = oracle.Machine(needles)
    assert cref.highlight(o, 1, needles, ["us, US and NIKE's apple"], "<b>", "</b>", exact) == [b"us, <b>US</b> and <b>NIKE</b>'s apple"]
    assert cref.counts(o, 1, needles, ["us, US and NIKE's apple", "Apple apple US"], exact) == [2, 1, 1]
    # under AM_CASE_SENSITIVE the rule is a constant per needle: an upper-case spelling of a lower-cased needle keeps nothing, the needle's own spelling everything
    assert cref.spans(o, 0, ref.ALL, needles, ["us US nike"], exact) == [[(6, 4, 2)]]
    assert cref.spans(o, 0, ref.ALL, needles, ["us US nike"], ["us", None, "nike"]) == [[(0, 2, 0), (6, 4, 2)]]


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n                                               # (hasattr: the version script exports it)
    assert re.search(r"#define\s+AM_SPAN_TABLE_WORDS\s+1u", src) and am.api.SPAN_TABLE_WORDS == 1
    assert "am_*" in open(os.path.join(ROOT, "alfred-margaret_amd", "csrc", "libam.map")).read()
    for n in ("amh_spans_fold_cased", "amh_spans_cased", "amh_substitute_fold_cased", "amh_spans"):
        assert hasattr(am.api.libhost(), n), n
    part = doc[doc.index("---- exact case"):doc.index("am_span_table_exact(const")]
    for word in ("exact[v]", "len == |exact[v]|", "FILTER, THEN SELECT", "U+212A", "AB C", "Duplicate", "AM_SPAN_TABLE_WORDS", "START bytes", "single-mode"):
        assert word in part, word
    assert hasattr(am, "Cased") and "exact" in am.SpanTable.__init__.__code__.co_varnames


def test_every_argument_is_refused_before_any_device_work():
    lib = am.api.libam()
    out = C.c_void_p(1)
    one = np.ones(1, np.uint32)
    zero = np.zeros(2, np.uint64)

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and word in lib.am_last_error(), (rc, lib.am_last_error())
        assert not out.value
        out.value = 1

    assert lib.am_span_table_create_cased(None, one.ctypes.data, one.ctypes.data, 0, None, None, None, None) == am.AM_ERR_INVALID
    refused(lib.am_span_table_create_cased(None, one.ctypes.data, one.ctypes.data, 0, None, None, None, C.byref(out)), b"null needle ids")
    refused(lib.am_span_table_create_cased(None, one.ctypes.data, one.ctypes.data, 1, None, zero.ctypes.data, None, C.byref(out)), b"null needle ids")
    refused(lib.am_span_table_create_cased(None, one.ctypes.data, one.ctypes.data, 2, None, None, None, C.byref(out)), b"unknown flag bits")
    refused(lib.am_span_table_create_cased(None, one.ctypes.data, one.ctypes.data, 0x80000001, None, None, None, C.byref(out)), b"unknown flag bits")
    p, n = C.c_void_p(1), C.c_uint64(7)
    assert lib.am_span_table_exact(None, 0, C.byref(p), C.byref(n)) == 0 and not p.value and n.value == 0
    assert lib.am_span_table_exact(None, 0, None, None) == 0
    # the front end's own checks
    a = am.Automaton(["ab", "cd"])
    for bad in (["AB"], ["AB", None, None], ["AB", b""]):
        with pytest.raises(am.AmError) as e:
            am.api._pack_exact(bad, 2)
        assert e.value.code == am.AM_ERR_INVALID
    assert am.api._pack_exact(None, 2) == (None, None) and am.api._pack_exact([None, None], 2) == (None, None)
    offs, pool = am.api._pack_exact(["AB", None], 2)
    assert offs.tolist() == [0, 2, 2] and bytes(pool) == b"AB"
    for needles, exact in ((["US", "nike"], [1]), (["US", "nike"], {"Nike"}), (["", "a"], [1, 0])):
        with pytest.raises(am.AmError) as e:
            am.Cased(needles, exact)
        assert e.value.code == am.AM_ERR_INVALID
    c = am.Cased(["US", "Apple", "nike"], exact={"US", "Apple"})
    assert c.exact == [b"US", b"Apple", None] and c.automaton.needles == [b"us", b"apple", b"nike"]
    assert am.Cased(["US", "Apple", "nike"], exact=[True, True, False]).exact == c.exact
    assert am.Cased(["K"], [1], lower_pairs=[(0x212A, 0x6B)]).automaton.needles == [b"k"]
    # the refusals of the spellings, on any machine: am_span_table_check_exact is the very function am_span_table_create_cased calls between its null-ids check and
    # the runtime (a needle-ids handle cannot be made without a device, so the constructor itself shows them only further below, where there is one)
    lb, lc = np.array([2, 2, 0], np.uint32), np.array([2, 1, 0], np.uint32)

    def check_exact(offs, pool):
        offs = np.asarray(offs, np.uint64)
        buf = (C.c_uint8 * max(len(pool), 1)).from_buffer_copy(pool or b"\0")
        return lib.am_span_table_check_exact(lb.ctypes.data, lc.ctypes.data, 3, offs.ctypes.data, buf)

    for offs, pool, word in (([1, 2, 2, 2], b"xAB", b"exact_off[0]"), ([0, 2, 1, 2], b"ABC", b"descends"), ([0, 1 << 32, 1 << 32, 1 << 32], b"AB", b"2^32"),
                             ([0, 2, 2, 2], b"\x85B", b"continuation byte"), ([0, 3, 3, 3], b"ABC", b"code points"),
                             ([0, 2, 4, 4], b"AB" + "\u00c5".encode()[:1] + b"B", b"code points"), ([0, 0, 0, 1], b"A", b"length 0")):
        rc = check_exact(offs, pool)
        assert rc == am.AM_ERR_INVALID and word in lib.am_last_error(), (offs, rc, lib.am_last_error())
    assert check_exact([0, 2, 4, 4], b"AB" + "\u00c5".encode()) == am.AM_OK and check_exact([0, 0, 0, 0], b"") == am.AM_OK
    assert lib.am_span_table_check_exact(None, None, 3, None, None) == am.AM_OK                     # no spellings: nothing to check
    if not _gpu():
        for call in (lambda: c.spans(["us, US"]), lambda: c.highlight(["US"], "<", ">"), lambda: c.count_by_needle(["US"]), lambda: c.grep(["US"]),
                     lambda: am.SpanTable(a, exact=["AB", None])):
            with pytest.raises(am.AmError) as e:
                call()
            assert e.value.code == am.AM_ERR_NO_DEVICE
        return
    # with a device: every refusal of the spellings, each with *out == NULL, and none of them has made a table
    a = am.Automaton(["ab", "å", ""])
    ids = am.ValuesTable(a)

    def create(offs, pool, flags=0):
        offs = np.asarray(offs, np.uint64)
        buf = (C.c_uint8 * max(len(pool), 1)).from_buffer_copy(pool + b"\0" * (1 - min(len(pool), 1)))
        rc = lib.am_span_table_create_cased(ids.handle, lb.ctypes.data, lc.ctypes.data, flags, None, offs.ctypes.data, buf, C.byref(out))
        if rc == am.AM_OK:
            lib.am_span_table_destroy(out)
            out.value = None
        return rc

    out.value = 1
    refused(create([1, 2, 2, 2], b"xAB"), b"exact_off[0]")
    refused(create([0, 2, 1, 2], b"ABC"), b"descends")
    refused(create([0, 1 << 32, 1 << 32, 1 << 32], b"AB"), b"2^32")
    refused(create([0, 2, 2, 2], b"\x85B"), b"continuation byte")
    refused(create([0, 3, 3, 3], b"ABC"), b"code points")                                          # three START bytes for a needle of two code points
    refused(create([0, 2, 4, 4], b"AB" + "Å".encode()[:1] + b"B"), b"code points")             # two START bytes for a needle of one
    refused(create([0, 0, 0, 1], b"A"), b"length 0")
    refused(create([0, 2, 2, 2], b"AB", flags=4), b"unknown flag bits")
    out.value = None
    assert create([0, 2, 4, 4], b"AB" + "Å".encode()) == am.AM_OK and create([0, 2, 4, 4], b"AB" + "Å".encode(), flags=1) == am.AM_OK
    t = am.SpanTable(a, exact=["AB", None, None], word_bytes=True)
    assert t.exact == [b"AB", None, None] and t.word_bytes == am.default_word_bytes()
    assert am.SpanTable(a, exact=[None] * 3).exact == [None] * 3 and am.SpanTable(a).exact == [None] * 3


def test_the_host_fold_gives_the_examples_without_a_device():
    for needles, exact, text, want in cref.EXAMPLES:
        o = oracle.Machine(needles)
        lb, lc = (x[:len(needles)] for x in am.api.needle_lengths(needles))
        for mode, rows in want.items():
            assert _rows(*am.api.spans_fold_host(1, mode, _triples(o, 1, [text]), [text], lb, lc, exact=exact)) == [rows], (needles, exact, text, mode)
    needles, exact, text = ["us", "apple", "nike"], ["US", "Apple", None], "us, US and NIKE's apple"
    o = oracle.Machine(needles)
    lb, lc = (x[:3] for x in am.api.needle_lengths(needles))
    assert am.api.substitute_fold_host(1, _triples(o, 1, [text]), [text], lb, lc, ["<0>", "<1>", "<2>"], exact=exact) == [b"us, <0> and <2>'s apple"]
    # with the default class too: `us` inside `bonUS` is spelled right and is no whole word
    text = "bonUS US"
    assert _rows(*am.api.spans_fold_host(1, ref.ALL, _triples(o, 1, [text]), [text], lb, lc, exact=exact)) == [[(3, 2, 0), (6, 2, 0)]]
    assert _rows(*am.api.spans_fold_host(1, ref.ALL, _triples(o, 1, [text]), [text], lb, lc, word_bytes=True, exact=exact)) == [[(6, 2, 0)]]


@pytest.mark.parametrize("seed", range(3))
def test_the_host_fold_equals_the_definition_on_random_cases(seed):
    """300 seeded cases in all: the alphabet a A b B k K U+212A U+00C5 U+212B U+0130 and the blank, needles of 1 to 5 code points, texts up to 120 bytes, both case
    modes and span modes, without a class and with the default one.  The set holds cases where filtering after the selection gives another answer."""
    kept = dropped = differ = 0
    for needles, exact, hays in cref.seeded(8800 + seed, oracle.lower_utf8, 100):
        assert all(len(n) <= 5 for n in needles) and all(len(h.encode()) <= 120 for h in hays)
        o = oracle.Machine(needles)
        n = len(needles)
        lb, lc = (x[:n] for x in am.api.needle_lengths(needles))
        repl = ["", "R"] + ["<%d>" % v * 3 for v in range(2, n)]
        for case in (0, 1):
            tr = _triples(o, case, hays)
            for cls in (None, wref.DEFAULT_CLASS):
                wb = None if cls is None else sorted(cls)
                for mode in MODES:
                    got = am.api.spans_fold_host(case, mode, tr, hays, lb, lc, word_bytes=wb, exact=exact)
                    exp = cref.spans(o, case, mode, needles, hays, exact, cls)
                    assert _rows(*got) == exp, (seed, needles, exact, hays, case, mode, cls is not None)
                    if mode == ref.ALL and cls is None and case == 1:
                        plain = am.api.spans_fold_host(case, mode, tr, hays, lb, lc)
                        kept += len(got[1])
                        dropped += len(plain[1]) - len(got[1])
                got = am.api.substitute_fold_host(case, tr, hays, lb, lc, repl[:n], word_bytes=wb, exact=exact)
                assert got == cref.substitute(o, case, needles, hays, repl[:n], exact, cls), (seed, needles, exact, hays, case)
        differ += cref.spans(o, 1, ref.LEFTMOST_LONGEST, needles, hays, exact) != cref.select_then_filter(o, 1, needles, hays, exact)
    assert kept > 100 and dropped > 100 and differ >= 1, (kept, dropped, differ)      # (the case set is not trivial: rows are kept, rows are dropped, the order matters)


def _compile_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", *flags, "-I", os.path.join(ROOT, "alfred-margaret_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "cased_compare_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)      # (a sanitizer's runtime is linked into the program: it starts in the environment as it is)
    assert out.returncode == 0 and "all checks passed" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_the_comparator_on_the_cpu_equals_memcmp(tmp_path):
    """tests/native/cased_compare_main.cpp: cased_equal of csrc/am_cased.h against memcmp -- every spelling length 0 to 48 at every start residue 0 to 15, a single
    differing byte at every position, a span ending on the last byte of its haystack, and one ending on the last byte of the text with non-zero bytes where the
    padding would be; 17, 257 and 66 000 bytes."""
    _compile_and_run(tmp_path, "cased_compare", [])


def test_the_comparator_under_a_sanitizer(tmp_path):
    """The same program with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked in statically: the text is a vector of exactly round_up(total, 16)
    bytes and the pool one of exactly the spelling's groups.  A stand-alone program: no Python code runs under a sanitizer."""
    _compile_and_run(tmp_path, "cased_compare_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"])


def test_the_host_mirror_under_a_sanitizer(tmp_path):
    """tests/native/cased_sanitize_main.cpp: exactCase, spansFold and substituteFold of host/spans.hpp with spellings over hand-written fold steps, compiled with
    AddressSanitizer + UndefinedBehaviorSanitizer (runtimes linked in statically) and run as a stand-alone program: no Python code runs under a sanitizer."""
    exe = str(tmp_path / "cased_sanitize")
    lib_dir = os.path.dirname(am.api.libam()._name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "alfred-margaret_amd", "host"),
                           os.path.join(ROOT, "tests", "native", "cased_sanitize_main.cpp"), "-L", lib_dir, "-lam", "-Wl,-rpath," + lib_dir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
