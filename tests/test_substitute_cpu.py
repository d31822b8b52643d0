"""am_subst_table_* / am_substitute* / am_batch_substitute and the batch accessors (include/am.h "substitute"): the definition (tests/substitute_reference.py) gives the
header's examples and equals an independent regex formulation, the entry points exist, are bound and check their arguments before any device work, and the host mirror's
sequential splice (amh_substitute_fold, no device) equals the definition.

No span table can be made without a device (am_needle_ids_create needs one): there the checks are seen with null handles, which every entry point checks last."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers, spans_reference as ref, substitute_reference as sref
from tests.conftest import ROOT

NAMES = ("am_subst_table_create", "am_subst_table_destroy", "am_batch_substitute", "am_substitute_batch", "am_substitute", "am_substitute_geometry",
         "am_batch_haystacks", "am_batch_device_text", "am_batch_device_offsets", "am_batch_read_offsets", "am_batch_read_text")
KELVIN = "\u212a"

# the header's examples: (needles, replacements, text, case, expected)
TABLE = [
    (["b", "abc", "abcd"], ["X", "Y", "Z"], "abcd b", 0, b"Z X"),
    (["a"], [""], "banana", 0, b"bnn"),
    (["", "a"], ["!", "-"], "banana", 0, b"b-n-n-"),                      # the empty needle inserts nothing
    (["k"], ["K!"], "k" + KELVIN + "K.", 1, b"K!K!K!."),                  # U+212A: three bytes removed
    (["ab", "ab"], ["1", "2"], "abab", 0, b"11"),                         # the smallest handle of equal spans
    (["aa"], ["b"], "aaaaa", 0, b"bba"),
    (["x"], ["y"], "", 0, b""),
    (["x"], ["y"], "abc", 0, b"abc"),
]


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_the_definition_gives_the_examples():
    for needles, repls, text, case, want in TABLE:
        assert sref.substitute(oracle.Machine(needles), case, needles, [text], repls) == [want], (needles, text)
        if case == 0:
            assert sref.regex_substitute(needles, [text], repls) == [want], (needles, text)


@pytest.mark.parametrize("seed", range(4))
def test_the_definition_equals_the_regex_formulation(seed):
    """Duplicate and empty needles over a three-byte alphabet: leftmost start, then the longest, then the smallest handle."""
    rng = random.Random(9200 + seed)
    for _ in range(150):
        needles = ["".join(rng.choice("abc") for _ in range(rng.randint(0, 4))) for _ in range(rng.randint(1, 6))]
        repls = ["".join(rng.choice("abcXY") for _ in range(rng.randint(0, 3))) for _ in needles]
        hays = ["".join(rng.choice("abc") for _ in range(rng.randint(0, 30))) for _ in range(3)]
        assert sref.substitute(oracle.Machine(needles), 0, needles, hays, repls) == sref.regex_substitute(needles, hays, repls), (needles, repls, hays)


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    assert re.search(r"typedef struct am_subst_table am_subst_table;", src)
    for n in ("amh_substitute_fold", "amh_substitute"):
        assert hasattr(am.api.libhost(), n), n
    assert len(am.api.DEBUG_ABI) == 14                     # no new am_debug_* symbol
    for n in ("SubstTable", "batch_to_bytes", "substitute_geometry"):
        assert hasattr(am.api, n), n
    for n in ("substitute", "substitute_host_mirror"):
        assert hasattr(am.Automaton, n), n
    build_py = open(os.path.join(ROOT, "alfred-margaret_amd", "build.py")).read()
    assert '"am_subst.cpp"' in build_py and '"am_subst.hip"' in build_py


def test_header_block_states_the_semantics():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    part = doc[doc.index("---- substitute"):doc.index("am_batch_read_text(const")]
    assert "Replacer.hs:163-180" in part
    for word in ("NEVER SCANNED", "ZERO-LENGTH", "SKIPPED", "SPAN'S OWN len", "BYTE FOR BYTE", "IN ORDER", "WORKSPACE", "NOT bounded", "64-bit", "order of any atomic"):
        assert word in part, word
    for phrase in ("hay[0, s_1) ++ repl[v_1]", "repl_off[0] != 0", "descending offsets", "2^32 bytes", "AM_SPANS_ALL result", "round_up(total, 16)", "36 bytes per piece",
                   "SOURCE coordinates", "must outlive"):
        assert phrase in part, phrase


def test_the_geometry_is_known_without_a_device():
    g, t = am.api.substitute_geometry()
    assert g == 16 and t % g == 0 and t >= 16 * g
    am.api.libam().am_substitute_geometry(None, None)


def test_every_argument_is_refused_before_any_device_work():
    lib = am.api.libam()
    s = am.api._Slices(["abc"])
    out, sp = C.c_void_p(1), C.c_void_p(1)

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and not out.value and word in lib.am_last_error(), (rc, out.value, lib.am_last_error())
        out.value = 1

    off = np.zeros(2, np.uint64)
    assert lib.am_subst_table_create(None, off.ctypes.data, None, None) == am.AM_ERR_INVALID
    refused(lib.am_subst_table_create(None, off.ctypes.data, None, C.byref(out)), b"null span table or repl_off")
    assert lib.am_substitute(None, 0, s.arr, s.n, None) == am.AM_ERR_INVALID
    refused(lib.am_substitute(None, 0, None, 1, C.byref(out)), b"hay is null")
    refused(lib.am_substitute(None, 0, s.arr, 0xFFFFFFFF, C.byref(out)), b"too many")
    refused(lib.am_substitute(None, 7, s.arr, s.n, C.byref(out)), b"case_mode")
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    refused(lib.am_substitute(None, 0, bad, 1, C.byref(out)), b"slice with null ptr")
    refused(lib.am_substitute(None, 0, s.arr, s.n, C.byref(out)), b"null substitution table")
    refused(lib.am_substitute(None, 1, s.arr, 0, C.byref(out)), b"null substitution table")
    assert lib.am_substitute_batch(None, 0, None, None, None) == am.AM_ERR_INVALID
    refused(lib.am_substitute_batch(None, 3, None, C.byref(out), C.byref(sp)), b"case_mode")
    assert not sp.value
    sp.value = 1
    refused(lib.am_substitute_batch(None, 0, None, C.byref(out), C.byref(sp)), b"null substitution table or batch")
    assert not sp.value
    assert lib.am_batch_substitute(None, None, None, None) == am.AM_ERR_INVALID
    refused(lib.am_batch_substitute(None, None, None, C.byref(out)), b"null batch, spans or substitution table")
    # the accessors of a null batch
    assert lib.am_batch_haystacks(None) == 0 and not lib.am_batch_device_text(None) and not lib.am_batch_device_offsets(None)
    buf = np.zeros(4, np.uint64)
    assert lib.am_batch_read_offsets(None, buf.ctypes.data) == am.AM_ERR_INVALID
    assert lib.am_batch_read_text(None, 0, 0, None) == am.AM_ERR_INVALID
    lib.am_subst_table_destroy(None)
    if not _gpu():
        return
    a = am.Automaton(["ab", "c", "d"])
    t = am.SpanTable(a)

    def create(offs, pool=b"xxxxxxxx"):
        offs = np.asarray(offs, np.uint64)
        rc = lib.am_subst_table_create(t.handle, offs.ctypes.data, pool, C.byref(out))
        if rc == am.AM_OK:
            lib.am_subst_table_destroy(out)
            out.value = None
        return rc

    refused(lib.am_subst_table_create(t.handle, None, b"x", C.byref(out)), b"null span table or repl_off")
    refused(create([1, 2, 3, 4]), b"repl_off[0] must be 0")
    refused(create([0, 2, 1, 4]), b"descends")
    refused(create([0, 1, 1 + (1 << 32), 2 + (1 << 32)]), b"2^32 bytes")
    refused(create([0, 1, 2, 3], pool=None), b"repl_bytes is null")
    out.value = None
    assert create([0, 0, 0, 0], pool=None) == am.AM_OK                  # an empty pool needs no bytes
    assert create([0, 1, 1, 8]) == am.AM_OK
    r = am.SubstTable(t, ["1", "2", "3"])
    other = am.SubstTable(am.SpanTable(a, 2), ["1", "2"])
    b, b2 = C.c_void_p(), C.c_void_p()
    am.api.check(lib.am_batch_upload(s.arr, s.n, C.byref(b)))
    s2 = am.api._Slices(["abc", "d"])
    am.api.check(lib.am_batch_upload(s2.arr, s2.n, C.byref(b2)))
    ll = t.spans_batch(0, b, ref.LEFTMOST_LONGEST, raw=True)
    every = t.spans_batch(0, b, ref.ALL, raw=True)
    try:
        out.value = 1
        refused(lib.am_batch_substitute(b, every, r.handle, C.byref(out)), b"AM_SPANS_LEFTMOST_LONGEST")
        refused(lib.am_batch_substitute(b2, ll, r.handle, C.byref(out)), b"haystack count and size")
        refused(lib.am_batch_substitute(b, ll, other.handle, C.byref(out)), b"n_needles differs")
        refused(lib.am_batch_substitute(None, ll, r.handle, C.byref(out)), b"null batch")
        refused(lib.am_batch_substitute(b, None, r.handle, C.byref(out)), b"null batch")
        refused(lib.am_batch_substitute(b, ll, None, C.byref(out)), b"null batch")
        refused(lib.am_substitute_batch(r.handle, 2, b, C.byref(out), None), b"case_mode")
        refused(lib.am_substitute_batch(r.handle, 0, None, C.byref(out), None), b"null substitution table or batch")
        assert lib.am_batch_read_text(b, 1, 3, buf.ctypes.data) == am.AM_ERR_INVALID      # beyond total
        assert lib.am_batch_read_text(b, 4, 0, buf.ctypes.data) == am.AM_ERR_INVALID
        assert lib.am_batch_read_text(b, 3, 0, None) == am.AM_OK
        assert lib.am_batch_read_text(b, 0, 3, None) == am.AM_ERR_INVALID
        assert lib.am_batch_read_text(b, 0, 2 ** 64 - 1, buf.ctypes.data) == am.AM_ERR_INVALID
        out.value = None
        am.api.check(lib.am_batch_substitute(b, ll, r.handle, C.byref(out)))
        assert am.api.batch_to_bytes(out)[1] == [b"12"]
        lib.am_batch_destroy(out)
    finally:
        lib.am_spans_free(ll)
        lib.am_spans_free(every)
        lib.am_batch_destroy(b)
        lib.am_batch_destroy(b2)


def test_without_a_gpu_the_front_end_reports_no_device():
    a = am.Automaton(["b", "abc", "abcd"])
    if _gpu():
        assert a.substitute(0, ["abcd b", ""], ["X", "Y", "Z"]) == [b"Z X", b""]
        return
    for call in (lambda: a.substitute(0, ["abcd"], ["X", "Y", "Z"]), lambda: a.substitute_host_mirror(0, ["abcd"], ["X", "Y", "Z"])):
        with pytest.raises(am.AmError) as e:
            call()
        assert e.value.code == am.AM_ERR_NO_DEVICE


def _fold(case, o, hays, lengths, repls):
    """amh_substitute_fold over the oracle's fold steps."""
    triples = helpers.oracle_triples(o, case, hays)
    cols = list(zip(*triples)) if triples else ((), (), ())
    arrays = tuple(np.array(c, dtype=t) for c, t in zip(cols, (np.uint32, np.uint64, np.uint32)))
    return am.api.substitute_fold_host(case, arrays, hays, lengths[0], lengths[1], repls)


def test_the_host_splice_gives_the_examples_without_a_device():
    for needles, repls, text, case, want in TABLE:
        lb, lc = am.api.needle_lengths(needles)
        n = len(needles)
        assert _fold(case, oracle.Machine(needles), [text], (lb[:n], lc[:n]), repls) == [want], (needles, text)


REPL_POOL = ["", "!", "x" * 15, "y" * 16, "z" * 17, "<" + "r" * 298 + ">"]


@pytest.mark.parametrize("seed", range(4))
def test_the_host_splice_equals_the_definition_on_the_fragment_pool(seed):
    rng = random.Random(4100 + seed)                                      # the cases of tests/test_spans_cpu.py
    for i in range(11):
        needles, hays = helpers.fragment_case(rng)
        if i % 3 == 0:
            needles = needles + [needles[0]]                              # a duplicate needle with a replacement of its own: the smaller handle's is used
        o = oracle.Machine(needles)
        for n in (len(needles), max(0, len(needles) - 2)):                # n below the largest handle: the last two needles are skipped
            lb, lc = am.api.needle_lengths(needles, n)
            repls = [REPL_POOL[(v + seed) % len(REPL_POOL)] + str(v) * (v % 2) for v in range(n)]
            for case in (0, 1):
                exp = sref.substitute(o, case, needles, hays, repls, n)
                assert _fold(case, o, hays, (lb[:n], lc[:n]), repls) == exp, (seed, needles, hays, n, case)
                if case == 0 and n == len(needles):
                    assert sref.regex_substitute(needles, hays, repls) == exp, (seed, needles, hays)


def test_the_host_splice_with_shared_and_duplicate_handles():
    needles = ["ab", "ab", "cd", "abcd", "b", "xyz"]
    values = [0, 1, 0, 2, 3, 9]
    by_handle = ["ab", "ab", "abcd", "b"]                                 # "ab" and "cd" share handle 0; handle 9 is beyond every n: skipped
    repls = ["<0>", "", "TWO" * 6, "b"]
    hays = ["abcdab", "", "xyzcdcdab", "bbabxyz"]
    o = oracle.Machine(needles, values)
    for n in (4, 3, 1, 0):
        lb, lc = am.api.needle_lengths(by_handle, n)
        for case in (0, 1):
            got = _fold(case, o, hays, (lb[:n], lc[:n]), repls[:n])
            assert got == sref.substitute(o, case, by_handle, hays, repls[:n], n), (n, case)
            if n == 0:
                assert got == [h.encode() for h in hays]
    lb, lc = am.api.needle_lengths(by_handle)
    assert _fold(0, o, ["ab cd xyz"], (lb[:4], lc[:4]), repls) == [b"<0> <0> xyz"]
