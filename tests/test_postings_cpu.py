"""am_postings_* / am_spans_of_needle (include/am.h "postings") without a device: the definition in numpy (api.postings_host) gives the header's worked example and
agrees with the reference (tests/postings_reference.py, sorted() over the oracle's spans), every entry point is declared and bound, the arguments are checked before
any device work, the geometry is known, and the pass plan of csrc/am_postings.h run on the CPU is std::stable_sort -- plain and under a sanitizer, in a stand-alone
program.

No span table, batch or spans result can be made without a device: there the checks are seen with handles that are never looked at, and a well-formed call reaches
the runtime and reports AM_ERR_NO_DEVICE."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import alfred_margaret_amd as am
from tests import postings_reference as ref
from tests.conftest import ROOT
from tests.test_near_cpu import spans_arrays
from tests.test_select_cpu import cases

NAMES = ("am_postings_from_spans", "am_postings_batch", "am_postings", "am_postings_size", "am_postings_needles", "am_postings_haystacks", "am_postings_offsets",
         "am_postings_data", "am_postings_source", "am_postings_doc_freq", "am_postings_device_offsets", "am_postings_device_data", "am_postings_device_source",
         "am_postings_device_doc_freq", "am_postings_free", "am_spans_of_needle", "am_postings_geometry")
NEEDLE_COUNTS = (1, 2, 255, 256, 257, 65535, 65536, 65537, 2 ** 24 + 2)


def _gpu():
    import torch
    return torch.cuda.is_available()


def check_host(rows, n_needles, what=None):
    """postings_host over the rows against the definition."""
    offsets, data, source, doc_freq = ref.postings(rows, n_needles)
    go, gd, gs, gf = am.api.postings_host(*spans_arrays(rows), n_needles)
    assert go.dtype == gs.dtype == gf.dtype == np.uint64 and gd.dtype == am.api.SPAN_DTYPE
    assert go.tolist() == offsets, (what, "offsets")
    assert [tuple(int(x) for x in r) for r in gd.tolist()] == data, (what, "data")
    assert gs.tolist() == source, (what, "source")
    assert gf.tolist() == doc_freq, (what, "doc_freq")
    return offsets, data, source, doc_freq


def test_the_worked_example_of_the_header():
    rows = ref.rows_of(["nike", "shoe"], 0, ["shoe nike shoe", "nike"])
    assert ref.flat(rows) == [(0, 4, 0, 1), (5, 4, 0, 0), (10, 4, 0, 1), (0, 4, 1, 0)]
    offsets, data, source, doc_freq = check_host(rows, 2)
    assert offsets == [0, 2, 4]
    assert data == [(5, 4, 0, 0), (0, 4, 1, 0), (0, 4, 0, 1), (10, 4, 0, 1)]
    assert source == [1, 3, 0, 2] and doc_freq == [2, 1]
    assert ref.spans_of(rows, 1)[:2] == ([0, 2, 2], [(0, 4, 0, 1), (10, 4, 0, 1)])
    assert ref.spans_of(rows, 0)[:2] == ([0, 1, 2], [(5, 4, 0, 0), (0, 4, 1, 0)])


@pytest.mark.parametrize("seed", range(2))
def test_the_numpy_definition_is_the_reference(seed):
    seen = {"empty_row": 0, "df_below_count": 0, "several_haystacks": 0}
    for needles, hays, _ in cases(9800 + seed, 120):
        for case, mode in ((0, ref.ALL), (1, ref.LEFTMOST_LONGEST)):
            ns = [ref.oracle.lower_utf8(x).decode() for x in needles] if case else needles
            rows = ref.rows_of(ns, case, hays, mode)
            offsets, data, _, doc_freq = check_host(rows, len(ns), (ns, hays, case, mode))
            counts = np.diff(offsets).tolist()
            seen["empty_row"] += 0 in counts
            seen["df_below_count"] += any(f < c for f, c in zip(doc_freq, counts))
            seen["several_haystacks"] += any(f > 1 for f in doc_freq)
            assert all((f == 0) == (c == 0) and f <= c for f, c in zip(doc_freq, counts))
    assert all(v >= 1 for v in seen.values()), seen


def test_the_numpy_definition_s_corners():
    z = np.zeros(0, am.api.SPAN_DTYPE)
    for offs, n in (([0], 0), ([0], 3), ([0, 0, 0], 0), ([0, 0, 0], 5)):
        go, gd, gs, gf = am.api.postings_host(offs, z, n)
        assert go.tolist() == [0] * (n + 1) and gd.shape == (0,) and gs.shape == (0,) and gf.tolist() == [0] * n
    one = np.array([(0, 1, 0, 2)], am.api.SPAN_DTYPE)
    for bad in (lambda: am.api.postings_host([0, 2], one, 3),      # offsets of other spans
                lambda: am.api.postings_host([0, 1], one, 2)):     # a handle that is not below n_needles
        with pytest.raises(am.AmError) as e:
            bad()
        assert e.value.code == am.AM_ERR_INVALID


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    assert re.search(r"struct am_postings;", src)
    assert len(am.api.DEBUG_ABI) == 14                     # no new am_debug_* symbol
    debug = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "am_debug.h")).read(), flags=re.S)
    assert "postings" not in debug
    for n in ("Postings", "postings_host", "postings_geometry"):
        assert hasattr(am, n), n
    for n in ("postings", "doc_freq", "concordance"):
        assert hasattr(am.Automaton, n), n
    for n in ("postings_batch", "postings_texts", "postings_from_spans"):
        assert hasattr(am.api.SpanTable, n), n
    for n in ("offsets", "spans", "source", "doc_freq", "row", "spans_of", "__enter__", "__exit__", "__del__"):
        assert hasattr(am.Postings, n), n
    build_py = open(os.path.join(ROOT, "alfred-margaret_amd", "build.py")).read()
    assert '"am_postings.cpp"' in build_py and '"am_postings.hip"' in build_py
    shared = open(os.path.join(ROOT, "alfred-margaret_amd", "csrc", "am_postings.h")).read()
    for n in ("post_passes", "post_digit", "post_cell"):
        assert n in shared, n


def bitlen(x):
    return int(x).bit_length()


@pytest.mark.parametrize("n_needles", NEEDLE_COUNTS + (0, 3, 128, 129, 2 ** 32 - 1))
def test_the_geometry_is_known_without_a_device(n_needles):
    tile, wave, passes, bits = am.api.postings_geometry(n_needles)
    key_bits = bitlen(n_needles - 1) if n_needles > 1 else 0
    assert tile % wave == 0 and wave % 64 == 0 and tile >= wave >= 64
    assert passes == (0 if n_needles <= 1 else -(-key_bits // 8)) and passes <= 4 and len(bits) == passes
    assert sum(bits) == key_bits and all(1 <= b <= 8 for b in bits)
    raw = (C.c_uint32 * 4)(9, 9, 9, 9)
    am.api.libam().am_postings_geometry(n_needles, None, None, None, raw)
    assert list(raw) == bits + [0] * (4 - passes)          # zero beyond the passes
    am.api.libam().am_postings_geometry(n_needles, None, None, None, None)


def test_the_pass_counts_of_the_issue_s_sizes():
    assert [am.api.postings_geometry(n)[2] for n in (1, 2, 256, 257, 65536, 65537, 2 ** 24 + 2)] == [0, 1, 1, 2, 2, 3, 4]


def test_every_argument_is_refused_before_any_device_work():
    lib = am.api.libam()
    s = am.api._Slices(["abc"])
    out = C.c_void_p(1)
    fake = C.c_void_p(64)                                  # a handle that is never looked at: the check that refuses the call comes first

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and not out.value and word in lib.am_last_error(), (rc, out.value, lib.am_last_error())
        out.value = 1

    # the stage
    assert lib.am_postings_from_spans(fake, None) == am.AM_ERR_INVALID and b"out is null" in lib.am_last_error()
    refused(lib.am_postings_from_spans(None, C.byref(out)), b"null spans")
    # the batch form
    assert lib.am_postings_batch(fake, 0, 0, fake, None) == am.AM_ERR_INVALID
    for case in (-1, 2, 99):
        refused(lib.am_postings_batch(fake, case, 0, fake, C.byref(out)), b"case_mode")
    for mode in (-1, 2, 7):
        refused(lib.am_postings_batch(fake, 0, mode, fake, C.byref(out)), b"spans_mode")
    refused(lib.am_postings_batch(None, 0, 1, fake, C.byref(out)), b"null span table or batch")
    refused(lib.am_postings_batch(fake, 1, 0, None, C.byref(out)), b"null span table or batch")
    # the one-shot form
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    assert lib.am_postings(fake, 0, 0, s.arr, s.n, None) == am.AM_ERR_INVALID
    refused(lib.am_postings(fake, 0, 0, None, 1, C.byref(out)), b"hay is null")
    refused(lib.am_postings(fake, 1, 1, s.arr, 0xFFFFFFFF, C.byref(out)), b"too many")
    refused(lib.am_postings(fake, 0, 0, bad, 1, C.byref(out)), b"slice with null ptr")
    refused(lib.am_postings(fake, 2, 0, s.arr, s.n, C.byref(out)), b"case_mode")
    refused(lib.am_postings(fake, 0, 2, s.arr, s.n, C.byref(out)), b"spans_mode")
    refused(lib.am_postings(None, 0, 0, s.arr, s.n, C.byref(out)), b"null span table")
    # one needle's row
    assert lib.am_spans_of_needle(fake, 0, None) == am.AM_ERR_INVALID
    refused(lib.am_spans_of_needle(None, 0, C.byref(out)), b"null postings")
    # the accessors of a null result
    for f in (lib.am_postings_size, lib.am_postings_needles, lib.am_postings_haystacks):
        assert f(None) == 0
    for f in (lib.am_postings_offsets, lib.am_postings_data, lib.am_postings_source, lib.am_postings_doc_freq, lib.am_postings_device_offsets,
              lib.am_postings_device_data, lib.am_postings_device_source, lib.am_postings_device_doc_freq):
        assert not f(None)
    lib.am_postings_free(None)
    if not _gpu():
        # valid arguments reach the runtime
        for n_hay in (s.n, 0):
            x = C.c_void_p(1)
            assert lib.am_postings(fake, 0, 1, s.arr if n_hay else None, n_hay, C.byref(x)) == am.AM_ERR_NO_DEVICE and x.value is None
    # (the refusals that need real handles -- needle >= N, handles on different devices, a converted row at the byte-span stages -- are in tests/test_gpu_postings.py)


def test_without_a_gpu_the_front_end_reports_no_device():
    a = am.Automaton(["nike", "shoe"])                     # built on the host
    if _gpu():
        return                                             # (what the front end computes is tests/test_gpu_postings.py's)
    for call in (lambda: a.postings(am.CASE_SENSITIVE, ["shoe nike shoe", "nike"]), lambda: a.doc_freq(am.IGNORE_CASE, ["nike"]),
                 lambda: a.concordance(am.IGNORE_CASE, ["a nike shoe"], "nike", before=2, after=2)):
        with pytest.raises(am.AmError) as e:
            call()
        assert e.value.code == am.AM_ERR_NO_DEVICE
    with pytest.raises(am.AmError) as e:
        a.concordance(0, ["x"], "boot")                    # not among the needles: refused before anything is made
    assert e.value.code == am.AM_ERR_INVALID


def _compile_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", *flags, "-I", os.path.join(ROOT, "alfred-margaret_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "postings_sort_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)      # (a sanitizer's runtime is linked into the program: it starts in the environment as it is)
    assert out.returncode == 0 and "all checks passed" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_the_pass_plan_on_the_cpu_is_a_stable_sort(tmp_path):
    """tests/native/postings_sort_main.cpp: per-tile digit counts, the exclusive sum in (digit, tile) order, placement by in-tile rank, pass after pass, with the
    header's own post_plan / post_digit / post_cell, against std::stable_sort -- N in {1, 2, 255, 256, 257, 65 535, 65 536, 65 537, 2^24 + 2}, n around 0, 1, a round,
    one tile +- 1 and three tiles + 1; all-equal keys, two alternating keys, a skewed random draw."""
    _compile_and_run(tmp_path, "postings_sort", [])


def test_the_pass_plan_under_a_sanitizer(tmp_path):
    """The same program with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked in statically: every table is a vector of exactly the size the plan
    gives it.  A stand-alone program: no Python code runs under a sanitizer."""
    _compile_and_run(tmp_path, "postings_sort_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"])
