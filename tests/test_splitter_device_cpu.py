"""am_splitter_* / am_split* / am_fragments_* / am_batch_from_fragments (include/am.h): the entry points exist, are bound, and check their arguments before any
device work.

am_automaton_create works on a box without a GPU (host-side build + validation), so every check of am_splitter_create runs anywhere.  A batch and a result cannot be
made without a device: there the null checks are made on the raw symbols, and the run entry points report AM_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from tests.conftest import ROOT

NAMES = ("am_splitter_create", "am_splitter_destroy", "am_split_batch", "am_split", "am_fragments_size", "am_fragments_haystacks", "am_fragments_offsets",
         "am_fragments_data", "am_fragments_device_offsets", "am_fragments_device_data", "am_fragments_free", "am_batch_from_fragments")


def _gpu():
    import torch
    return torch.cuda.is_available()


def _create(a, nbytes, ncps):
    h = C.c_void_p()
    rc = am.api.libam().am_splitter_create(a.device if a is not None else None, nbytes, ncps, C.byref(h))
    if h.value:
        am.api.libam().am_splitter_destroy(h)
    return rc


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    assert re.search(r"typedef struct am_fragment \{ uint64_t start; uint64_t len; \} am_fragment;", src)
    part = doc[doc.index("---- Splitter"):doc.index("am_batch_from_fragments(const")]
    for cite in ("Splitter.hs:84-85", "Splitter.hs:96-97", "Splitter.hs:141-147", "Splitter.hs:163-164", "Splitter.hs:105-107", "Splitter.hs:117-121", "Utf8.hs:256-276"):
        assert cite in part, cite
    assert "NOT bounded" in part                           # record memory: one scan of the whole batch
    assert "AM_SPLIT_CHAIN_LIMIT" in am.api.DEBUG_SWITCHES
    am.debug_set("AM_SPLIT_CHAIN_LIMIT", 1)
    am.debug_set("AM_SPLIT_CHAIN_LIMIT", -1)
    assert am.api.FRAGMENT_DTYPE.itemsize == 16


def test_splitter_create_checks_its_arguments_without_a_device():
    lib = am.api.libam()
    one = am.Automaton(["ab"])
    assert lib.am_splitter_create(one.device, 2, 2, None) == am.AM_ERR_INVALID
    assert _create(None, 2, 2) == am.AM_ERR_INVALID
    assert b"null" in lib.am_last_error()
    assert _create(one, 0, 0) == am.AM_ERR_INVALID         # the empty separator is refused
    assert _create(one, 0, 1) == am.AM_ERR_INVALID
    assert _create(one, 2, 0) == am.AM_ERR_INVALID
    assert _create(one, 2, 3) == am.AM_ERR_INVALID         # more code points than bytes
    assert _create(one, 2, 2) == am.AM_OK
    assert _create(am.Automaton(["ßß"]), 4, 2) == am.AM_OK
    # not a one-needle automaton: two needles; one needle under two handles (one state, two values); a suffix that reports too; no needle
    for needles in (["ab", "cd"], ["ab", "ab"], ["ab", "b"], []):
        assert _create(am.Automaton(needles), 2, 2) == am.AM_ERR_INVALID, needles
    assert b"one-needle" in lib.am_last_error()
    # a failed create leaves no handle behind
    h = C.c_void_p(1)
    assert lib.am_splitter_create(one.device, 0, 0, C.byref(h)) == am.AM_ERR_INVALID and not h.value


def test_null_arguments_are_invalid_before_any_device_work():
    lib = am.api.libam()
    s = am.api._Slices(["a,b"])
    out = C.c_void_p(1)
    assert lib.am_split_batch(None, 0, None, C.byref(out)) == am.AM_ERR_INVALID and not out.value
    assert lib.am_split(None, 0, s.arr, s.n, C.byref(out)) == am.AM_ERR_INVALID
    assert lib.am_batch_from_fragments(None, None, C.byref(out)) == am.AM_ERR_INVALID
    assert b"null" in lib.am_last_error()
    sp = am.Splitter(",")
    assert lib.am_split(sp.device, 0, s.arr, s.n, None) == am.AM_ERR_INVALID
    assert lib.am_split(sp.device, 0, None, 1, C.byref(out)) == am.AM_ERR_INVALID
    assert lib.am_split(sp.device, 7, s.arr, s.n, C.byref(out)) == am.AM_ERR_INVALID
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    assert lib.am_split(sp.device, 0, bad, 1, C.byref(out)) == am.AM_ERR_INVALID
    assert lib.am_split_batch(sp.device, 0, None, C.byref(out)) == am.AM_ERR_INVALID
    assert lib.am_split_batch(sp.device, 0, None, None) == am.AM_ERR_INVALID
    # the accessors of a null result
    assert lib.am_fragments_size(None) == 0 and lib.am_fragments_haystacks(None) == 0
    assert not lib.am_fragments_offsets(None) and not lib.am_fragments_data(None)
    assert not lib.am_fragments_device_offsets(None) and not lib.am_fragments_device_data(None)
    lib.am_fragments_free(None)
    lib.am_splitter_destroy(None)
    if not _gpu():
        return
    b, f, nb = C.c_void_p(), C.c_void_p(), C.c_void_p()
    am.api.check(lib.am_batch_upload(s.arr, s.n, C.byref(b)))
    am.api.check(lib.am_split_batch(sp.device, 0, b, C.byref(f)))
    try:
        assert lib.am_split_batch(None, 0, b, C.byref(out)) == am.AM_ERR_INVALID
        assert lib.am_split_batch(sp.device, 0, b, None) == am.AM_ERR_INVALID
        assert lib.am_split_batch(sp.device, 2, b, C.byref(out)) == am.AM_ERR_INVALID
        assert lib.am_batch_from_fragments(None, f, C.byref(nb)) == am.AM_ERR_INVALID
        assert lib.am_batch_from_fragments(b, None, C.byref(nb)) == am.AM_ERR_INVALID
        assert lib.am_batch_from_fragments(b, f, None) == am.AM_ERR_INVALID
        # fragments of another batch: the haystack count or the size differs
        for other in (["a,b", ""], ["a,b,"]):
            so = am.api._Slices(other)
            bo = C.c_void_p()
            am.api.check(lib.am_batch_upload(so.arr, so.n, C.byref(bo)))
            try:
                assert lib.am_batch_from_fragments(bo, f, C.byref(nb)) == am.AM_ERR_INVALID and not nb.value
            finally:
                lib.am_batch_destroy(bo)
    finally:
        lib.am_fragments_free(f)
        lib.am_batch_destroy(b)


def test_without_a_gpu_the_run_entry_points_report_no_device():
    sp = am.Splitter(",")
    if _gpu():
        assert sp.split_batch_device(["a,b,,c", "", ","]) == [[b"a", b"b", b"", b"c"], [b""], [b"", b""]]
        return
    lib = am.api.libam()
    s = am.api._Slices(["a,b"])
    out = C.c_void_p()
    assert lib.am_split(sp.device, 0, s.arr, s.n, C.byref(out)) == am.AM_ERR_NO_DEVICE and not out.value
    assert lib.am_split(sp.device, 1, s.arr, 0, C.byref(out)) == am.AM_ERR_NO_DEVICE
    for call in (lambda: sp.split_batch_device(["a,b"]), lambda: sp.split_batch_device(["a,b"], True), lambda: sp.fragments_texts(["a,b"])):
        with pytest.raises(am.AmError) as e:
            call()
        assert e.value.code == am.AM_ERR_NO_DEVICE


def test_the_haskell_package_names_the_new_module():
    """The cabal file lists Data.Text.AhoCorasick.Splitter.Device among its exposed modules, the file exists and declares that module."""
    hs = os.path.join(ROOT, "haskell")
    cabal = open(os.path.join(hs, "alfred-margaret-device.cabal")).read()
    exposed = cabal[cabal.index("exposed-modules:"):cabal.index("extra-libraries:")]
    mods = re.findall(r"\bData\.Text\.AhoCorasick\.[A-Za-z.]+\b", re.sub(r"--[^\n]*", "", exposed))
    assert sorted(mods) == sorted("Data.Text.AhoCorasick.%s.Device" % m for m in ("Automaton", "Searcher", "Replacer", "Splitter")), mods
    for m in mods:
        path = os.path.join(hs, "src", *m.split(".")) + ".hs"
        assert os.path.exists(path), path
        assert re.search(r"^module %s\b" % re.escape(m), open(path).read(), flags=re.M), m
