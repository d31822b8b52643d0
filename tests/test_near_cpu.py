"""am_near_* / am_select_near (include/am.h "proximity"): the definition (tests/near_reference.py, brute force) gives the header's worked examples, the host mirror
(host/near.hpp nearFold, a plain loop to the left and right) agrees with it, the shared pick and bitmap arithmetic of csrc/am_near.h hold under a sanitizer in a
stand-alone program, and the entry points exist, are bound and check their arguments before any device work.

No span table or batch can be made without a device: there the checks are seen with handles that are never looked at, and a well-formed call reaches the runtime and
reports AM_ERR_NO_DEVICE."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import near_reference as ref
from tests.conftest import ROOT
from tests.test_select_cpu import cases

NAMES = ("am_near_create", "am_near_destroy", "am_near_spans", "am_near_batch", "am_near", "am_near_hits_size", "am_near_hits_haystacks", "am_near_hits_queries",
         "am_near_hits_hay_words", "am_near_hits_offsets", "am_near_hits_data", "am_near_hits_fired", "am_near_hits_counts", "am_near_hits_device_offsets",
         "am_near_hits_device_data", "am_near_hits_device_fired", "am_near_hits_device_counts", "am_near_hits_free", "am_select_near", "am_near_geometry")
WANTED = ("tie", "partner_p", "partner_n", "anchor_in_both", "partner_only_next_door", "gap_at_max", "gap_one_beyond")


def _gpu():
    import torch
    return torch.cuda.is_available()


def spans_arrays(rows):
    """(offsets, SPAN_DTYPE rows) of per-haystack (start, len, handle) lists: what near_host takes."""
    offs = np.zeros(len(rows) + 1, np.uint64)
    flat = np.zeros(sum(len(r) for r in rows), am.api.SPAN_DTYPE)
    k = 0
    for h, r in enumerate(rows):
        for s, n, v in r:
            flat[k] = (s, n, h, v)
            k += 1
        offs[h + 1] = k
    return offs, flat


def check_host(rows, masks, queries, what=None, stats=None):
    """near_host over the rows against the definition: pairs, offsets, fired, counts."""
    offsets, pairs, fired, counts = ref.near(rows, masks, queries, stats)
    go, gp, gf, gc = am.api.near_host(*spans_arrays(rows), masks, queries)
    assert go.tolist() == offsets, (what, "offsets")
    assert [tuple(int(x) for x in p) for p in gp.tolist()] == pairs, (what, "pairs")
    assert [[int(w) for w in row] for row in gf] == ref.fired_words(fired, len(rows)), (what, "fired")
    assert gc.tolist() == counts, (what, "counts")
    return pairs


NIKE = ["nike", "shoe", "kids"]
NIKE_MASKS = [1, 2, 0]                                      # A = {nike}, B = {shoe}, kids in no group


def test_the_worked_examples_of_the_header():
    rows = ref.rows_of(NIKE, 0, ["nike kids shoe, shoe nike"])
    assert rows == [[(0, 4, 0), (5, 4, 2), (10, 4, 1), (16, 4, 1), (21, 4, 0)]]
    assert check_host(rows, NIKE_MASKS, [(0, 1, 1, False)]) == [(4, 3, 1, 0, 0)]
    assert check_host(rows, NIKE_MASKS, [(0, 1, 6, False)]) == [(0, 2, 6, 0, 0), (4, 3, 1, 0, 0)]
    assert check_host(rows, NIKE_MASKS, [(0, 1, 6, True)]) == [(0, 2, 6, 0, 0)]
    rows = ref.rows_of(NIKE, 0, ["shoe nike shoe"])
    assert check_host(rows, NIKE_MASKS, [(0, 1, 1, False)]) == [(1, 0, 1, 0, 0)]      # both gaps are 1: the tie goes to p
    assert check_host(rows, NIKE_MASKS, [(0, 1, 0, False)]) == []
    # the anchor is never its own partner; group_a == group_b is a repeated mention; partners never come from another haystack; touching spans have gap 0
    rows = ref.rows_of(["a", "b"], 0, ["aa", "a", "ab", "b"])
    assert check_host(rows, [1, 2], [(0, 0, ref.ANYWHERE, False)]) == [(0, 1, 0, 0, 0), (1, 0, 0, 0, 0)]
    assert check_host(rows, [1, 2], [(0, 1, ref.ANYWHERE, False)]) == [(3, 4, 0, 2, 0)]
    assert check_host(rows, [3, 2], [(0, 1, ref.ANYWHERE, True), (1, 0, 0, False)]) == [(0, 1, 0, 0, 0), (0, 1, 0, 0, 1), (1, 0, 0, 0, 1), (3, 4, 0, 2, 0), (4, 3, 0, 2, 1)]


def random_queries(rng, n_groups, small):
    out = []
    for k in range(rng.randint(1, 6)):
        a = rng.randrange(n_groups)
        b = a if rng.random() < 0.25 else rng.randrange(n_groups)
        out.append((a, b, (0, 1, small, ref.ANYWHERE)[(k + rng.randrange(4)) % 4], rng.random() < 0.4))
    return out


@pytest.mark.parametrize("seed", range(2))
def test_the_host_mirror_is_the_definition(seed):
    rng = random.Random(9100 + seed)
    stats, seen = {}, {"no_group": 0, "several_groups": 0, "same_group": 0, "ordered": 0}
    for needles, hays, _ in cases(9200 + seed, 150):
        for case in (0, 1):
            ns = [oracle.lower_utf8(x).decode() for x in needles] if case else needles
            rows = ref.rows_of(ns, case, hays)
            n_groups = rng.choice([1, 2, 3, 32])
            masks = [0 if rng.random() < 0.2 else rng.getrandbits(32) & rng.getrandbits(32) & ((1 << n_groups) - 1) | (1 << rng.randrange(n_groups)) for _ in ns]
            queries = random_queries(rng, n_groups, rng.randint(2, 6))
            seen["no_group"] += any(m == 0 for m in masks)
            seen["several_groups"] += any(bin(m).count("1") > 1 for m in masks)
            seen["same_group"] += any(q[0] == q[1] for q in queries)
            seen["ordered"] += any(q[3] for q in queries)
            check_host(rows, masks, queries, (ns, hays, masks, queries), stats)
    for k in WANTED:
        assert stats.get(k, 0) >= 1, (k, stats)
    assert all(v >= 1 for v in seen.values()), seen


def test_the_host_mirror_s_corners():
    # no queries, no haystacks, haystacks without spans, groups no needle belongs to
    go, gp, gf, gc = am.api.near_host([0, 0, 0], np.zeros(0, am.api.SPAN_DTYPE), [1, 2], [])
    assert go.tolist() == [0, 0, 0] and gp.shape == (0,) and gf.shape == (0, 1) and gc.shape == (0,)
    go, gp, gf, gc = am.api.near_host([0], np.zeros(0, am.api.SPAN_DTYPE), [], [(0, 1, 5)])
    assert go.tolist() == [0] and gp.shape == (0,) and gf.shape == (1, 0) and gc.tolist() == [0]
    rows = ref.rows_of(["a", "b"], 0, ["ab", "", "ba"])
    assert check_host(rows, [1, 2], [(0, 5, ref.ANYWHERE, False), (7, 0, ref.ANYWHERE, False)]) == []
    # 130 haystacks: three words of fired, the last one partial
    rows = ref.rows_of(["a", "b"], 0, ["ab"] * 130)
    pairs = check_host(rows, [1, 2], [(0, 1, 0, False)])
    assert len(pairs) == 130
    _, _, gf, _ = am.api.near_host(*spans_arrays(rows), [1, 2], [(0, 1, 0, False)])
    assert [int(w) for w in gf[0]] == [2 ** 64 - 1, 2 ** 64 - 1, 3]
    for bad in (lambda: am.api.near_host([0], [], [], [(32, 0, 1)]),                              # a group index beyond 31
                lambda: am.api.near_host([0], [], [], [(0, 0, 1)] * 65),                          # more queries than the maximum
                lambda: am.api.near_host([0], [], [], np.array([(0, 0, 2, 0, 1)], am.api.NEAR_QUERY_DTYPE)),      # an unknown flag
                lambda: am.api.near_host([0], [], [], np.array([(0, 0, 0, 9, 1)], am.api.NEAR_QUERY_DTYPE)),      # reserved
                lambda: am.api.near_host([0, 2], np.zeros(1, am.api.SPAN_DTYPE), [], [])):        # offsets of other spans
        with pytest.raises(am.AmError) as e:
            bad()
        assert e.value.code == am.AM_ERR_INVALID


def test_the_shared_pick_holds_under_a_sanitizer(tmp_path):
    """tests/native/near_pick_main.cpp: near_pick and the bitmap-word arithmetic of csrc/am_near.h on the CPU against a brute-force loop, over 1, 2 and 5 words of 64
    spans, compiled with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked in statically.  A stand-alone program: no Python code runs under a sanitizer."""
    exe = str(tmp_path / "near_pick")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "alfred-margaret_amd", "csrc"), os.path.join(ROOT, "tests", "native", "near_pick_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)      # (the runtimes are linked into the program: it starts in the environment as it is)
    assert out.returncode == 0 and "all checks passed" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_header_declares_and_front_end_binds_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    for n in NAMES:
        assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src), n
        assert n in am.api.ABI and hasattr(lib, n), n
    assert re.search(r"#define AM_NEAR_MAX_GROUPS 32", src) and re.search(r"#define AM_NEAR_MAX_QUERIES 64", src) and re.search(r"#define AM_NEAR_ORDERED 1u", src)
    assert (am.api.NEAR_MAX_GROUPS, am.api.NEAR_MAX_QUERIES, am.api.NEAR_ORDERED) == (32, 64, 1)
    assert re.search(r"typedef struct am_near_query \{ uint32_t group_a, group_b, flags, reserved; uint64_t max_gap; \} am_near_query;", src)
    assert re.search(r"typedef struct am_near_pair \{ uint64_t a, b, gap; uint32_t haystack, query; \} am_near_pair;", src)
    q, p = am.api.NEAR_QUERY_DTYPE, am.api.NEAR_PAIR_DTYPE
    assert q.itemsize == 24 and [q.fields[f][1] for f in ("group_a", "group_b", "flags", "reserved", "max_gap")] == [0, 4, 8, 12, 16]
    assert p.itemsize == 32 and [p.fields[f][1] for f in ("a", "b", "gap", "haystack", "query")] == [0, 8, 16, 24, 28]
    assert len(am.api.DEBUG_ABI) == 14                     # no new am_debug_* symbol
    for n in ("Near", "NearQuery", "NearHits", "near_host", "near_geometry"):
        assert hasattr(am, n), n
    assert hasattr(am.Automaton, "near") and hasattr(am.api.libhost(), "amh_near_fold")
    build_py = open(os.path.join(ROOT, "alfred-margaret_amd", "build.py")).read()
    assert '"am_near.cpp"' in build_py and '"am_near.hip"' in build_py
    assert "nearFold" in open(os.path.join(ROOT, "alfred-margaret_amd", "host", "near.hpp")).read()
    assert "near_pick" in open(os.path.join(ROOT, "alfred-margaret_amd", "csrc", "am_near.h")).read()


def test_the_geometry_is_known_without_a_device():
    tile, word = am.api.near_geometry()
    assert word == 64 and tile >= 64 and tile % 64 == 0     # a wavefront's ballot is a bitmap word; a workgroup step is whole words
    am.api.libam().am_near_geometry(None, None)


def test_every_argument_is_refused_before_any_device_work():
    lib = am.api.libam()
    s = am.api._Slices(["abc"])
    out, sp = C.c_void_p(1), C.c_void_p(1)
    fake = C.c_void_p(1)                                   # a handle that is never looked at: the check that refuses the call comes first
    masks = np.asarray([1], np.uint32)

    def queries(*rows):
        return np.array(list(rows), am.api.NEAR_QUERY_DTYPE)

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and not out.value and word in lib.am_last_error(), (rc, out.value, lib.am_last_error())
        out.value = 1

    # the handle
    ok = queries((0, 1, 0, 0, 5))
    assert lib.am_near_create(fake, masks.ctypes.data, ok.ctypes.data, 1, None) == am.AM_ERR_INVALID
    refused(lib.am_near_create(fake, masks.ctypes.data, queries(*[(0, 1, 0, 0, 5)] * 65).ctypes.data, 65, C.byref(out)), b"n_queries")
    refused(lib.am_near_create(fake, masks.ctypes.data, None, 1, C.byref(out)), b"queries is null")
    refused(lib.am_near_create(fake, masks.ctypes.data, queries((32, 1, 0, 0, 5)).ctypes.data, 1, C.byref(out)), b"group index")
    refused(lib.am_near_create(fake, masks.ctypes.data, queries((0, 1, 0, 0, 5), (0, 32, 0, 0, 5)).ctypes.data, 2, C.byref(out)), b"group index")
    refused(lib.am_near_create(fake, masks.ctypes.data, queries((0, 1, 2, 0, 5)).ctypes.data, 1, C.byref(out)), b"flags")
    refused(lib.am_near_create(fake, masks.ctypes.data, queries((0, 1, 1, 7, 5)).ctypes.data, 1, C.byref(out)), b"reserved")
    refused(lib.am_near_create(None, masks.ctypes.data, ok.ctypes.data, 1, C.byref(out)), b"null span table")
    lib.am_near_destroy(None)
    # the stage and its two wrappers
    assert lib.am_near_spans(fake, fake, None) == am.AM_ERR_INVALID
    refused(lib.am_near_spans(None, fake, C.byref(out)), b"null proximity handle or spans")
    refused(lib.am_near_spans(fake, None, C.byref(out)), b"null proximity handle or spans")

    def refused2(rc, word):
        assert not sp.value
        sp.value = 1
        refused(rc, word)

    assert lib.am_near_batch(fake, 0, fake, None, C.byref(sp)) == am.AM_ERR_INVALID and not sp.value
    sp.value = 1
    refused2(lib.am_near_batch(fake, 2, fake, C.byref(out), C.byref(sp)), b"case_mode")
    refused2(lib.am_near_batch(None, 0, fake, C.byref(out), C.byref(sp)), b"null proximity handle or batch")
    refused2(lib.am_near_batch(fake, 1, None, C.byref(out), C.byref(sp)), b"null proximity handle or batch")
    refused(lib.am_near_batch(fake, -1, fake, C.byref(out), None), b"case_mode")
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    assert lib.am_near(fake, 0, s.arr, s.n, None, C.byref(sp)) == am.AM_ERR_INVALID and not sp.value
    sp.value = 1
    refused2(lib.am_near(fake, 0, None, 1, C.byref(out), C.byref(sp)), b"hay is null")
    refused2(lib.am_near(fake, 1, s.arr, 0xFFFFFFFF, C.byref(out), C.byref(sp)), b"too many")
    refused2(lib.am_near(fake, 0, bad, 1, C.byref(out), C.byref(sp)), b"slice with null ptr")
    refused2(lib.am_near(fake, 2, s.arr, s.n, C.byref(out), C.byref(sp)), b"case_mode")
    refused2(lib.am_near(None, 0, s.arr, s.n, C.byref(out), C.byref(sp)), b"null proximity handle")
    # the select
    assert lib.am_select_near(fake, 0, 0, fake, None) == am.AM_ERR_INVALID
    refused(lib.am_select_near(None, 0, 0, fake, C.byref(out)), b"null proximity hits or batch")
    refused(lib.am_select_near(fake, 0, 1, None, C.byref(out)), b"null proximity hits or batch")
    # the accessors of a null result
    for f in (lib.am_near_hits_size, lib.am_near_hits_haystacks, lib.am_near_hits_queries, lib.am_near_hits_hay_words):
        assert f(None) == 0
    for f in (lib.am_near_hits_offsets, lib.am_near_hits_data, lib.am_near_hits_fired, lib.am_near_hits_counts, lib.am_near_hits_device_offsets,
              lib.am_near_hits_device_data, lib.am_near_hits_device_fired, lib.am_near_hits_device_counts):
        assert not f(None)
    lib.am_near_hits_free(None)
    if not _gpu():
        # valid arguments reach the runtime
        x = C.c_void_p(1)
        assert lib.am_near_create(fake, masks.ctypes.data, ok.ctypes.data, 1, C.byref(x)) == am.AM_ERR_NO_DEVICE and x.value is None
        x, y = C.c_void_p(1), C.c_void_p(1)
        assert lib.am_near(fake, 0, None, 0, C.byref(x), C.byref(y)) == am.AM_ERR_NO_DEVICE and x.value is None and y.value is None
    # (the refusals that need real handles -- query >= n_queries, an AM_SPANS_ALL result, spans of another table, a batch of another size -- are in
    # tests/test_gpu_near.py)


def test_without_a_gpu_the_front_end_reports_no_device():
    a = am.Automaton(["nike", "shoe"])                     # built on the host
    if _gpu():
        return                                             # (what the front end computes is tests/test_gpu_near.py's)
    with pytest.raises(am.AmError) as e:
        a.near(am.IGNORE_CASE, ["nike shoe"], {"brand": ["nike"], "item": ["shoe"]}, [("brand", "item", 20)])
    assert e.value.code == am.AM_ERR_NO_DEVICE
