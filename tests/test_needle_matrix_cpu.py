"""am_count_matrix* (include/am.h): the ten entry points exist, are bound, document their contract and check their arguments before any device work.

Every handle the calls take (am_needle_ids, am_batch, am_matches) is made by a call that needs the device, so on a box without a GPU the null and range checks are made
on the raw symbols, and AM_ERR_NO_DEVICE is what the front end's count_matrix reports.  On a box with a GPU the same tests go on with real handles: each argument null
or out of range in turn."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from tests.conftest import ROOT

NAMES = ("am_count_matrix_batch", "am_count_matrix", "am_matches_count_matrix", "am_needle_matrix_size", "am_needle_matrix_haystacks", "am_needle_matrix_offsets",
         "am_needle_matrix_data", "am_needle_matrix_device_offsets", "am_needle_matrix_device_data", "am_needle_matrix_free")


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_header_declares_and_front_end_binds_the_ten_symbols():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[a-z0-9_ ]+\*?\s*%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    assert "am_debug_needle_matrix_limits" in am.api.DEBUG_ABI and hasattr(lib, "am_debug_needle_matrix_limits")
    assert "amh_count_matrix" in am.api._HOST


def test_header_block_states_the_contract():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    part = doc[doc.index("term-document matrix"):doc.index("am_needle_matrix_free(")]
    assert "Automaton.hs:442-553" in part
    assert "SORTED BY (haystack, needle) ASCENDING" in part and "Map.toAscList" in part                # the order
    assert ">= n_needles are SKIPPED" in part                                                           # the skipped handles
    assert "am_count_by_needle_batch's vector" in part and "am_count_batch's counts_out[i]" in part     # the two identities
    assert "No entry has count 0" in part and "empty row" in part
    assert "per slot" in part and "per haystack" in part and "per entry" in part                        # the workspace of the fold
    assert "typedef struct am_needle_count { uint64_t count; uint32_t needle; uint32_t haystack; } am_needle_count;" in doc


def test_the_entry_layout():
    d = am.api.NEEDLE_COUNT_DTYPE
    assert d.itemsize == 16
    assert [d.fields[k][1] for k in ("count", "needle", "haystack")] == [0, 8, 12]
    assert d.fields["count"][0] == np.uint64 and d.fields["needle"][0] == np.uint32 and d.fields["haystack"][0] == np.uint32


def test_the_limits_accessor_answers_anywhere():
    lim = am.api.needle_matrix_limits()
    assert lim["wave_row"] == 64 and lim["wave_row"] < lim["lds_row"]
    assert lim["lds_slots"] & (lim["lds_slots"] - 1) == 0 and lim["chunk_records"] * 1024 < 2 ** 32      # no LDS counter can wrap between two flushes
    assert am.api.libam().am_debug_needle_matrix_limits(None) == am.AM_ERR_INVALID


def test_null_and_invalid_arguments_are_refused_before_any_device_work():
    lib = am.api.libam()
    s = am.api._Slices(["abc"])
    x = C.c_void_p(77)
    junk = C.c_void_p(1)                                   # stands for a handle: every call below fails before it looks at it
    assert lib.am_count_matrix_batch(None, 0, None, C.byref(x)) == am.AM_ERR_INVALID and x.value is None
    assert lib.am_count_matrix_batch(junk, 0, junk, None) == am.AM_ERR_INVALID
    assert lib.am_count_matrix(None, 0, s.arr, s.n, C.byref(x)) == am.AM_ERR_INVALID
    assert lib.am_count_matrix(junk, 0, s.arr, s.n, None) == am.AM_ERR_INVALID
    assert lib.am_count_matrix(junk, 0, None, 1, C.byref(x)) == am.AM_ERR_INVALID
    assert lib.am_count_matrix(junk, 0, s.arr, 0xFFFFFFFF, C.byref(x)) == am.AM_ERR_INVALID
    assert lib.am_count_matrix(junk, 7, s.arr, s.n, C.byref(x)) == am.AM_ERR_INVALID
    assert b"case_mode" in lib.am_last_error()
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    assert lib.am_count_matrix(junk, 0, bad, 1, C.byref(x)) == am.AM_ERR_INVALID
    assert lib.am_matches_count_matrix(None, None, 1, C.byref(x)) == am.AM_ERR_INVALID
    assert b"null" in lib.am_last_error()
    assert lib.am_matches_count_matrix(junk, junk, 1, None) == am.AM_ERR_INVALID
    assert lib.am_matches_count_matrix(junk, junk, 0xFFFFFFFF, C.byref(x)) == am.AM_ERR_INVALID
    assert x.value is None
    # the accessors of nothing
    assert lib.am_needle_matrix_size(None) == 0 and lib.am_needle_matrix_haystacks(None) == 0
    assert not lib.am_needle_matrix_offsets(None) and not lib.am_needle_matrix_data(None)
    assert not lib.am_needle_matrix_device_offsets(None) and not lib.am_needle_matrix_device_data(None)
    lib.am_needle_matrix_free(None)
    if not _gpu():
        return
    a = am.Automaton(["abc", "bc"])
    t = am.ValuesTable(a)
    b, m = C.c_void_p(), C.c_void_p()
    am.api.check(lib.am_batch_upload(s.arr, s.n, C.byref(b)))
    am.api.check(lib.am_run_batch(a.device, 0, b, C.byref(m)))
    try:
        for rc in (lib.am_count_matrix_batch(None, 0, b, C.byref(x)), lib.am_count_matrix_batch(t.handle, 0, None, C.byref(x)),
                   lib.am_count_matrix_batch(t.handle, 0, b, None), lib.am_count_matrix_batch(t.handle, 2, b, C.byref(x)),
                   lib.am_count_matrix(t.handle, 0, None, 1, C.byref(x)), lib.am_count_matrix(t.handle, 0, s.arr, s.n, None),
                   lib.am_count_matrix(t.handle, -1, s.arr, s.n, C.byref(x)), lib.am_count_matrix(t.handle, 0, bad, 1, C.byref(x)),
                   lib.am_count_matrix(t.handle, 0, s.arr, 0xFFFFFFFF, C.byref(x)),
                   lib.am_matches_count_matrix(None, t.handle, 1, C.byref(x)), lib.am_matches_count_matrix(m, None, 1, C.byref(x)),
                   lib.am_matches_count_matrix(m, t.handle, 1, None), lib.am_matches_count_matrix(m, t.handle, 0xFFFFFFFF, C.byref(x))):
            assert rc == am.AM_ERR_INVALID and x.value is None
    finally:
        lib.am_matches_free(m)
        lib.am_batch_destroy(b)


def test_without_a_gpu_the_front_end_reports_no_device():
    a = am.Automaton(["abc", "bc"])                        # host-side build + validation works anywhere
    if _gpu():
        offs, ents = a.count_matrix(0, ["xabcx", "", "bc"])
        assert offs.tolist() == [0, 2, 2, 3]
        assert [(int(e["haystack"]), int(e["needle"]), int(e["count"])) for e in ents] == [(0, 0, 1), (0, 1, 1), (2, 1, 1)]
        return
    for call in (lambda: a.count_matrix(0, ["xabcx"]), lambda: a.count_matrix_host_mirror(0, ["xabcx"])):
        with pytest.raises(am.AmError) as e:
            call()
        assert e.value.code == am.AM_ERR_NO_DEVICE
    # valid arguments reach the runtime: the raw one-shot call without haystacks
    x = C.c_void_p()
    assert am.api.libam().am_count_matrix(C.c_void_p(1), 0, None, 0, C.byref(x)) == am.AM_ERR_NO_DEVICE and x.value is None


def test_no_values_gives_empty_rows_without_asking_the_device():
    a = am.Automaton(["abc", "bc"])
    for got in (a.count_matrix(0, ["xabcx", "q"], n_values=0), a.count_matrix_host_mirror(0, ["xabcx", "q"], n_values=0)):
        offs, ents = got
        assert offs.dtype == np.uint64 and offs.tolist() == [0, 0, 0]
        assert ents.dtype == am.api.NEEDLE_COUNT_DTYPE and ents.size == 0
