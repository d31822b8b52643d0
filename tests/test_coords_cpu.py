"""am_coords_* / am_ranges_* (include/am.h "coordinates") without a device: the header declares and the front end binds every entry point, the argument checks answer
before any device work, the lookup arithmetic of csrc/am_coords.h holds on the CPU -- plain and under a sanitizer, in a stand-alone program -- and the reference the
GPU tests use (tests/coords_reference.py) agrees with Python's str semantics.

No batch, spans or index can be made without a device: there the checks are seen with handles that are never looked at."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import alfred_margaret_amd as am
from tests import coords_reference as cref
from tests.conftest import ROOT

NAMES = ("am_coords_create", "am_coords_destroy", "am_coords_index_bytes", "am_coords_spans", "am_coords_fragments", "am_coords_ranges", "am_ranges_size",
         "am_ranges_haystacks", "am_ranges_offsets", "am_ranges_data", "am_ranges_device_offsets", "am_ranges_device_data", "am_ranges_free", "am_coords_positions",
         "am_coords_positions_device")


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    for name, value in (("AM_UNIT_BYTES", "0"), ("AM_UNIT_CODE_POINTS", "1"), ("AM_UNIT_UTF16", "2"), ("AM_COORDS_CODE_POINTS", "1u"), ("AM_COORDS_UTF16", "2u"),
                        ("AM_COORDS_LINES", "4u")):
        assert re.search(r"#define %s %s\b" % (name, value), src), name
    assert (am.BYTES, am.CODE_POINTS, am.UTF16) == (0, 1, 2) == cref.UNITS
    assert (am.api.COORDS_CODE_POINTS, am.api.COORDS_UTF16, am.api.COORDS_LINES) == (1, 2, 4)
    assert re.search(r"typedef struct am_span_range \{ uint64_t start_line, start_col, end_line, end_col; \} am_span_range;", src)
    assert am.api.SPAN_RANGE_DTYPE.itemsize == 32 and am.api.SPAN_RANGE_DTYPE.names == ("start_line", "start_col", "end_line", "end_col")
    build = open(os.path.join(ROOT, "alfred-margaret_amd", "build.py")).read()
    assert '"am_coords.cpp"' in build and '"am_coords.hip"' in build
    debug = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "am_debug.h")).read(), flags=re.S)
    assert not re.search(r"am_debug_\w*(coords|ranges)", debug) and not [n for n in am.api.DEBUG_ABI if "coords" in n or "ranges" in n]      # no new am_debug_* symbol
    import inspect
    for fn in (am.Automaton.spans, am.api.SpanTable.spans_batch, am.Automaton.run_batch_with_case):
        assert inspect.signature(fn).parameters["unit"].default == am.BYTES
    assert inspect.signature(am.Automaton.locate).parameters["unit"].default == am.CODE_POINTS


def test_arguments_are_checked_before_any_device_work():
    lib = am.api.libam()
    fake = C.c_void_p(64)                                   # a handle that is never looked at: every check below comes before the first look
    out = C.c_void_p(1)

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and word in lib.am_last_error(), (rc, lib.am_last_error())

    refused(lib.am_coords_create(fake, 1, None), b"out is null")
    refused(lib.am_coords_create(None, 1, C.byref(out)), b"null batch")
    assert not out.value
    for what in (8, 0x10, 0xFFFFFFFF):
        out.value = 1
        refused(lib.am_coords_create(fake, what, C.byref(out)), b"AM_COORDS_LINES")
        assert not out.value
    for call in (lib.am_coords_spans, lib.am_coords_fragments, lib.am_coords_ranges):
        refused(call(fake, fake, 1, None), b"out is null")
        for c, s in ((None, fake), (fake, None), (None, None)):
            out.value = 1
            refused(call(c, s, 1, C.byref(out)), b"null")
            assert not out.value
        for unit in (-1, 3, 99):
            out.value = 1
            refused(call(fake, fake, unit, C.byref(out)), b"unit must be")
            assert not out.value
    for call in (lib.am_coords_positions, lib.am_coords_positions_device):
        refused(call(None, fake, fake, 1, 1, fake), b"null index")
        refused(call(fake, None, fake, 1, 1, fake), b"null")
        refused(call(fake, fake, None, 1, 1, fake), b"null")
        refused(call(fake, fake, fake, 1, 1, None), b"null")
        refused(call(fake, fake, fake, 1, 3, fake), b"unit must be")
        refused(call(fake, None, None, 0, 7, None), b"unit must be")
    assert lib.am_coords_index_bytes(None) == 0 and lib.am_ranges_size(None) == 0 and lib.am_ranges_haystacks(None) == 0
    assert not lib.am_ranges_offsets(None) and not lib.am_ranges_data(None) and not lib.am_ranges_device_data(None)
    lib.am_coords_destroy(None)
    lib.am_ranges_free(None)


def _compile_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", *flags, "-I", os.path.join(ROOT, "alfred-margaret_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "coords_lookup_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)      # (a sanitizer's runtime is linked into the program: it starts in the environment as it is)
    assert out.returncode == 0 and "all checks passed" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_the_lookup_arithmetic_on_the_cpu(tmp_path):
    """tests/native/coords_lookup_main.cpp: the class masks, the tile counts' host twin, coords_count, coords_linestart and line / column of csrc/am_coords.h against
    byte loops -- every base residue, every position of texts up to 3 tiles + 17 bytes, a line start 0, 1 and 5 tiles back."""
    _compile_and_run(tmp_path, "coords_lookup", [])


def test_the_lookup_arithmetic_under_a_sanitizer(tmp_path):
    """The same program with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked in statically: the text block ends at round_up(total, 16) and the
    prefix arrays at n_tiles + 1 entries, so a read beyond either is a report.  A stand-alone program: no Python code runs under a sanitizer."""
    _compile_and_run(tmp_path, "coords_lookup_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"])


POOL = ["a", "Z", "\n", "é", "ß", "€", "\u212a", "\U0001f600", "\U00010348", " "]      # 1- to 4-byte code points and the newline


def test_the_reference_agrees_with_str_semantics():
    rng = random.Random(28)
    for _ in range(400):
        s = "".join(rng.choice(POOL) for _ in range(rng.randint(0, 40)))
        b = s.encode("utf-8")
        p = 0
        for i in range(len(s) + 1):
            assert cref.cp(b, p) == cref.cp_loop(b, p) == cref.str_cp(s, i)
            assert cref.u16(b, p) == cref.u16_loop(b, p) == cref.str_u16(s, i)
            assert cref.line(b, p) == cref.line_loop(b, p) == cref.str_line(s, i)
            assert cref.linestart(b, p) == cref.linestart_loop(b, p) == len(s[:s.rfind("\n", 0, i) + 1].encode("utf-8"))
            for unit in cref.UNITS:
                assert cref.col(b, p, unit) == cref.str_col(s, i, unit), (s, i, unit)
            if i < len(s):
                p += len(s[i].encode("utf-8"))
    # on bytes that are no UTF-8 the loops are the contract: the numpy form is the loops
    for _ in range(200):
        b = bytes(rng.choice((0x41, 0x0A, 0x80, 0xBF, 0xC3, 0xE2, 0xF0, 0xF4, 0xFF)) for _ in range(rng.randint(0, 60)))
        for p in range(len(b) + 1):
            assert (cref.cp(b, p), cref.u16(b, p), cref.line(b, p), cref.linestart(b, p)) == (cref.cp_loop(b, p), cref.u16_loop(b, p), cref.line_loop(b, p), cref.linestart_loop(b, p))
    # ... and so is the table the long texts are checked with
    for _ in range(50):
        b = bytes(rng.choice((0x41, 0x0A, 0x80, 0xC3, 0xF0, 0x78)) for _ in range(rng.randint(0, 80)))
        t = cref.Table(b)
        starts = [rng.randint(0, len(b)) for _ in range(12)]
        lens = [rng.randint(0, len(b) - s) for s in starts]
        for unit in cref.UNITS:
            cols = [c.tolist() for c in t.spans(starts, lens, unit)]
            for k, (s, n) in enumerate(zip(starts, lens)):
                assert (cols[0][k], cols[1][k]) == cref.span(b, s, n, unit) and tuple(c[k] for c in cols[2:]) == cref.span_range(b, s, n, unit)
    assert cref.span("é NIKE".encode(), 3, 4, cref.CODE_POINTS) == (2, 4)
    assert cref.span_range("a\n\U0001f600x".encode(), 6, 1, cref.UTF16) == (1, 2, 1, 3)
