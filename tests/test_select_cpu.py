"""am_select_* / am_selection_* / am_batch_from_selection (include/am.h "select"): the definition (tests/select_reference.py) agrees with Python itself, the entry points
exist, are bound and check their arguments before any device work.

No automaton, needle-id table or batch can be made without a device: there the checks are seen with null handles, which every entry point checks last, and a well-formed
one-shot call without haystacks reaches the runtime and reports AM_ERR_NO_DEVICE."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from tests import helpers, select_reference as sel, words_reference as wref
from tests.conftest import ROOT

NAMES = ("am_select_any_batch", "am_select_all_batch", "am_select_spans_batch", "am_select_flags", "am_select_any", "am_select_all", "am_selection_size",
         "am_selection_source_haystacks", "am_selection_total_bytes", "am_selection_indices", "am_selection_device_indices", "am_selection_free",
         "am_batch_from_selection", "am_select_geometry")
PYTHON_LOWERS_LIKE_THE_TABLE = (0, 1, 3)                   # helpers.ALPHABETS whose str.lower() is one code point to one code point, as the table's (not: the dotted I, the final sigma)


def _gpu():
    import torch
    return torch.cuda.is_available()


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def cases(seed, n):
    """n fragment-pool cases: (needles, haystacks, python_lower_ok)."""
    rng = random.Random(seed)
    for _ in range(n):
        probe = random.Random()
        probe.setstate(rng.getstate())
        alphabet = helpers.ALPHABETS.index(probe.choice(helpers.ALPHABETS))      # (fragment_case draws the alphabet first)
        needles, hays = helpers.fragment_case(rng)
        yield needles, hays, alphabet in PYTHON_LOWERS_LIKE_THE_TABLE


def test_keep_is_the_complement_under_invert():
    hays = ["ab", "", "b", "abab"]
    assert sel.keep(lambda h: b"a" in h, False, hays) == ([0, 3], [b"ab", b"abab"])
    assert sel.keep(lambda h: b"a" in h, True, hays) == ([1, 2], [b"", b"b"])
    assert sel.offsets([b"ab", b"abab"]).tolist() == [0, 2, 6] and sel.offsets([]).tolist() == [0]


@pytest.mark.parametrize("seed", range(2))
def test_contains_any_is_pythons_in(seed):
    for needles, hays, lower_ok in cases(4100 + seed, 250):
        needles = [n for n in needles if n]
        p = sel.pred_any(needles, 0)
        for h in hays:
            assert p(_b(h)) == any(_b(n) in _b(h) for n in needles), (needles, h)
        if lower_ok:
            low = [n.lower() for n in needles]
            p = sel.pred_any(low, 1)
            for h in hays:
                assert p(_b(h)) == any(n in h.lower() for n in low), (low, h)


@pytest.mark.parametrize("seed", range(2))
def test_contains_all_is_pythons_all(seed):
    for needles, hays, lower_ok in cases(4200 + seed, 250):
        needles = [n for n in needles if n]
        p = sel.pred_all(needles, 0)
        for h in hays:
            assert p(_b(h)) == all(_b(n) in _b(h) for n in needles), (needles, h)
        if lower_ok:
            low = [n.lower() for n in needles]
            p = sel.pred_all(low, 1)
            for h in hays:
                assert p(_b(h)) == all(n in h.lower() for n in low), (low, h)
    assert sel.pred_all([], 0)(b"x") and sel.pred_all([], 1)(b"")
    assert not sel.pred_all([""], 0)(b"abc") and not sel.pred_all([""], 0)(b"")


@pytest.mark.parametrize("seed", range(2))
def test_spans_with_the_default_class_is_a_regex_search(seed):
    """(?<!\\w)(n1|n2|...)(?!\\w) of DESIGN 7.6 with Python's re over bytes; under IgnoreCase over the lowered haystack, where lowering keeps every byte length."""
    for needles, hays, lower_ok in cases(4300 + seed, 250):
        needles = [n for n in needles if n]
        if not needles:
            continue
        rx, _ = wref._regex(needles)
        p = sel.pred_spans(needles, 0, wref.DEFAULT_CLASS)
        plain = sel.pred_spans(needles, 0)
        for h in hays:
            assert p(_b(h)) == (rx.search(_b(h)) is not None), (needles, h)
            assert plain(_b(h)) == any(_b(n) in _b(h) for n in needles), (needles, h)
        if lower_ok and all(len(_b(c)) == len(_b(c.lower())) for h in hays for c in h):
            low = [n.lower() for n in needles]
            rx, _ = wref._regex(low)
            p = sel.pred_spans(low, 1, wref.DEFAULT_CLASS)
            for h in hays:
                assert p(_b(h)) == (rx.search(_b(h.lower())) is not None), (low, h)
    he = sel.pred_spans(["he"], 0, wref.DEFAULT_CLASS)
    assert not he(b"the") and he(b"he said") and he(b"(he)") and not he(b"")


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    assert re.search(r"typedef struct am_selection am_selection;", src)
    assert len(am.api.DEBUG_ABI) == 14                     # no new am_debug_* symbol
    for n in ("Selection", "select_flags", "select_geometry"):
        assert hasattr(am.api, n), n
    assert hasattr(am.Automaton, "grep") and hasattr(am.Searcher, "grep_batch") and hasattr(am.Searcher, "select_batch")
    assert hasattr(am.api.ValuesTable, "select_all_batch") and hasattr(am.api.SpanTable, "select_batch")
    build_py = open(os.path.join(ROOT, "alfred-margaret_amd", "build.py")).read()
    assert '"am_select.cpp"' in build_py and '"am_select.hip"' in build_py


def test_the_geometry_is_known_without_a_device():
    tile, block = am.api.select_geometry()
    assert tile >= 256 and tile % 16 == 0 and block >= 256
    am.api.libam().am_select_geometry(None, None)


def test_every_argument_is_refused_before_any_device_work():
    lib = am.api.libam()
    s = am.api._Slices(["abc"])
    out = C.c_void_p(1)
    fake = C.c_void_p(1)                                   # a handle that is never looked at: the check that refuses the call comes first

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and not out.value and word in lib.am_last_error(), (rc, out.value, lib.am_last_error())
        out.value = 1

    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    for one_shot, noun in ((lib.am_select_any, b"null automaton"), (lib.am_select_all, b"null needle ids")):
        assert one_shot(fake, 0, 0, s.arr, s.n, None) == am.AM_ERR_INVALID
        refused(one_shot(fake, 0, 0, None, 1, C.byref(out)), b"hay is null")
        refused(one_shot(fake, 0, 1, s.arr, 0xFFFFFFFF, C.byref(out)), b"too many")
        refused(one_shot(fake, 0, 0, bad, 1, C.byref(out)), b"slice with null ptr")
        refused(one_shot(fake, 2, 0, s.arr, s.n, C.byref(out)), b"case_mode")
        refused(one_shot(fake, -1, 1, s.arr, 0, C.byref(out)), b"case_mode")
        refused(one_shot(None, 0, 0, s.arr, s.n, C.byref(out)), noun)
        refused(one_shot(None, 1, 1, s.arr, 0, C.byref(out)), noun)
    for batch_form, noun in ((lib.am_select_any_batch, b"null automaton or batch"), (lib.am_select_all_batch, b"null needle ids or batch"),
                             (lib.am_select_spans_batch, b"null span table or batch")):
        assert batch_form(fake, 0, 0, fake, None) == am.AM_ERR_INVALID
        refused(batch_form(fake, 2, 0, fake, C.byref(out)), b"case_mode")
        refused(batch_form(None, 0, 0, fake, C.byref(out)), noun)
        refused(batch_form(fake, 1, 1, None, C.byref(out)), noun)
    flags = np.ones(4, np.uint8)
    assert lib.am_select_flags(None, flags.ctypes.data, 0, None) == am.AM_ERR_INVALID
    refused(lib.am_select_flags(None, flags.ctypes.data, 0, C.byref(out)), b"null batch")
    assert lib.am_batch_from_selection(fake, fake, None) == am.AM_ERR_INVALID
    refused(lib.am_batch_from_selection(None, fake, C.byref(out)), b"null batch or selection")
    refused(lib.am_batch_from_selection(fake, None, C.byref(out)), b"null batch or selection")
    # the accessors of a null selection
    assert lib.am_selection_size(None) == 0 and lib.am_selection_source_haystacks(None) == 0 and lib.am_selection_total_bytes(None) == 0
    assert not lib.am_selection_indices(None) and not lib.am_selection_device_indices(None)
    lib.am_selection_free(None)
    if not _gpu():
        return
    a = am.Automaton(["ab", "c"])
    with_batch = C.c_void_p()
    am.api.check(lib.am_batch_upload(s.arr, s.n, C.byref(with_batch)))
    try:
        refused(lib.am_select_flags(with_batch, None, 0, C.byref(out)), b"flags is null")
        refused(lib.am_select_any_batch(a.device, 5, 0, with_batch, C.byref(out)), b"case_mode")
        out.value = None
        am.api.check(lib.am_select_any_batch(a.device, 0, 0, with_batch, C.byref(out)))
        assert lib.am_selection_size(out) == 1 and lib.am_selection_source_haystacks(out) == 1 and lib.am_selection_total_bytes(out) == 3
        lib.am_selection_free(out)
    finally:
        lib.am_batch_destroy(with_batch)


def test_without_a_gpu_the_front_end_reports_no_device():
    a = am.Automaton(["he", "she"])                        # host-side build + validation works anywhere
    s = am.Searcher(0, ["he", "she"])
    assert s.case == 0
    if _gpu():
        idx, texts = a.grep(0, ["the", "he said", "", "she"], whole_words=True)
        assert idx.dtype == np.uint32 and idx.tolist() == [1, 3] and texts == [b"he said", b"she"]
        assert a.grep(0, ["the", "x", ""], invert=True)[0].tolist() == [1, 2]
        assert s.grep_batch(["the", "she", ""], all=True)[1] == [b"she"]
        return
    for call in (lambda: a.grep(0, ["the"]), lambda: a.grep(0, ["the"], whole_words=True), lambda: s.grep_batch(["the"]), lambda: s.grep_batch(["the"], all=True)):
        with pytest.raises(am.AmError) as e:
            call()
        assert e.value.code == am.AM_ERR_NO_DEVICE
    # valid arguments reach the runtime: the raw one-shot calls without haystacks
    lib = am.api.libam()
    x = C.c_void_p(1)
    assert lib.am_select_any(C.c_void_p(1), 0, 0, None, 0, C.byref(x)) == am.AM_ERR_NO_DEVICE and x.value is None
    x.value = 1
    assert lib.am_select_all(C.c_void_p(1), 1, 1, None, 0, C.byref(x)) == am.AM_ERR_NO_DEVICE and x.value is None
