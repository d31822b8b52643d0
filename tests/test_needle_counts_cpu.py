"""am_count_by_needle* (include/am.h): the three entry points exist, are bound, and check their arguments before any device work.

Every handle the calls take (am_needle_ids, am_batch, am_matches) is made by a call that needs the device, so on a box without a GPU "valid arguments" cannot be
built through the C ABI: there the null checks are made on the raw symbols, and AM_ERR_NO_DEVICE is what the front end's count_by_needle reports (the needle-id
table is the first thing it asks the device for).  On a box with a GPU the same tests go on with real handles: each argument null in turn, n_needles == 0."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from tests.conftest import ROOT

NAMES = ("am_count_by_needle_batch", "am_count_by_needle", "am_matches_count_by_needle")


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_header_declares_and_front_end_binds_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "am.h")).read(), flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+int\s+%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    # the fold is documented with the reference lines it stands for
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    part = doc[doc.index("per-needle match counts"):doc.index("am_matches_count_by_needle(")]
    assert "Automaton.hs:442-553" in part and "Main.hs:67-76" in part and ">= n_needles" in part
    assert "AM_HIST_RECORDS_MIB" in am.api.DEBUG_SWITCHES
    am.debug_set("AM_HIST_RECORDS_MIB", 1)
    am.debug_set("AM_HIST_RECORDS_MIB", -1)


def test_null_arguments_are_invalid_before_any_device_work():
    lib = am.api.libam()
    out = np.zeros(4, np.uint64)
    s = am.api._Slices(["abc"])
    assert lib.am_count_by_needle_batch(None, 0, None, out.ctypes.data) == am.AM_ERR_INVALID
    assert lib.am_count_by_needle(None, 0, s.arr, s.n, out.ctypes.data) == am.AM_ERR_INVALID
    assert lib.am_matches_count_by_needle(None, None, out.ctypes.data) == am.AM_ERR_INVALID
    assert b"null" in lib.am_last_error()
    if not _gpu():
        return
    a = am.Automaton(["abc", "bc"])
    t = am.ValuesTable(a)
    b, m = C.c_void_p(), C.c_void_p()
    am.api.check(lib.am_batch_upload(s.arr, s.n, C.byref(b)))
    am.api.check(lib.am_run_batch(a.device, 0, b, C.byref(m)))
    try:
        assert lib.am_count_by_needle_batch(None, 0, b, out.ctypes.data) == am.AM_ERR_INVALID
        assert lib.am_count_by_needle_batch(t.handle, 0, None, out.ctypes.data) == am.AM_ERR_INVALID
        assert lib.am_count_by_needle_batch(t.handle, 0, b, None) == am.AM_ERR_INVALID
        assert lib.am_count_by_needle(t.handle, 0, None, 1, out.ctypes.data) == am.AM_ERR_INVALID
        assert lib.am_count_by_needle(t.handle, 0, s.arr, s.n, None) == am.AM_ERR_INVALID
        bad = (am.api.Slice * 1)()
        bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
        assert lib.am_count_by_needle(t.handle, 0, bad, 1, out.ctypes.data) == am.AM_ERR_INVALID
        assert lib.am_matches_count_by_needle(None, t.handle, out.ctypes.data) == am.AM_ERR_INVALID
        assert lib.am_matches_count_by_needle(m, None, out.ctypes.data) == am.AM_ERR_INVALID
        assert lib.am_matches_count_by_needle(m, t.handle, None) == am.AM_ERR_INVALID
        assert not out.any()                               # no failed call wrote anything
    finally:
        lib.am_matches_free(m)
        lib.am_batch_destroy(b)


def test_without_a_gpu_the_calls_report_no_device():
    if _gpu():
        a = am.Automaton(["abc", "bc"])
        assert a.count_by_needle(0, ["xabcx"]).tolist() == [1, 1]
        return
    a = am.Automaton(["abc", "bc"])                        # host-side build + validation works anywhere
    for call in (lambda: a.count_by_needle(0, ["xabcx"]), lambda: a.count_by_needle_host_mirror(0, ["xabcx"]), lambda: am.ValuesTable(a)):
        with pytest.raises(am.AmError) as e:
            call()
        assert e.value.code == am.AM_ERR_NO_DEVICE


def test_no_needles_is_ok_and_writes_nothing():
    a = am.Automaton(["abc", "bc"])
    got = a.count_by_needle(0, ["xabcx"], n_values=0)      # (the front end has nothing to ask the device for)
    assert got.dtype == np.uint64 and got.size == 0
    if not _gpu():
        return
    lib = am.api.libam()
    t = am.ValuesTable(a, 0)
    s = am.api._Slices(["xabcx"])
    out = np.full(4, 77, np.uint64)
    b, m = C.c_void_p(), C.c_void_p()
    am.api.check(lib.am_batch_upload(s.arr, s.n, C.byref(b)))
    am.api.check(lib.am_run_batch(a.device, 0, b, C.byref(m)))
    try:
        assert lib.am_count_by_needle_batch(t.handle, 0, b, out.ctypes.data) == am.AM_OK
        assert lib.am_count_by_needle_batch(t.handle, 0, b, None) == am.AM_OK
        assert lib.am_count_by_needle(t.handle, 0, s.arr, s.n, out.ctypes.data) == am.AM_OK
        assert lib.am_matches_count_by_needle(m, t.handle, out.ctypes.data) == am.AM_OK
        assert (out == 77).all()
    finally:
        lib.am_matches_free(m)
        lib.am_batch_destroy(b)
