"""am_weights_* / am_score* / am_scores_* / am_select_top_k / am_select_score (include/am.h "scores"): the definition (tests/score_reference.py) agrees with the
arithmetic over the oracle's per-haystack counts, the host mirror agrees with the definition, and the entry points exist, are bound and check their arguments before
any device work.

No needle-id table or batch can be made without a device: there the checks are seen with handles that are never looked at, and a well-formed call reaches the
runtime and reports AM_ERR_NO_DEVICE."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import score_reference as ref
from tests.conftest import ROOT
from tests.test_select_cpu import cases

NAMES = ("am_weights_create", "am_weights_destroy", "am_score_batch", "am_score", "am_score_spans_batch", "am_matches_score", "am_scores_haystacks", "am_scores_columns",
         "am_scores_data", "am_scores_device_data", "am_scores_free", "am_scores_top_k", "am_select_top_k", "am_select_score", "am_score_geometry")


def _gpu():
    import torch
    return torch.cuda.is_available()


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def variants(rng, needles, hays):
    """The case with what the definition must carry: a needle listed twice, handles of the caller's own with some >= n and two needles under one handle."""
    needles = list(needles) + [needles[0]]
    n = len(needles)
    yield needles, None, n, hays
    n_small = max(1, n - 2)
    values = [rng.randrange(n_small + 2) for _ in needles]            # (n_small, n_small + 1: handles beyond the table)
    values[0] = values[-1] = 0
    yield needles, values, n_small, hays


@pytest.mark.parametrize("seed", range(2))
def test_the_definition_is_the_arithmetic_over_the_counts(seed):
    """score[c][i] = sum over v of count(i, v) * W[c][v] modulo 2^64, with the oracle's per-haystack counts."""
    rng = random.Random(8100 + seed)
    for needles, hays, _ in cases(6100 + seed, 120):
        for ns, values, n, hs in variants(rng, needles, hays):
            weights = ref.random_weights(rng, n, rng.choice([1, 3, 8]))
            for case in (0, 1):
                low = [oracle.lower_utf8(x).decode() for x in ns] if case else ns
                got = ref.expect(low, values, n, case, weights, hs)
                m = oracle.Machine(low, values)
                for i, h in enumerate(hs):
                    val = m.run_list(case, _b(h))[1]
                    counts = np.bincount(val[val < n].astype(np.int64), minlength=n)
                    for c, col in enumerate(weights):
                        assert got[c, i] == ref.wrap(sum(int(counts[v]) * int(col[v]) for v in range(n))), (low, values, h, c)


def test_the_definitions_corners():
    # overlapping occurrences, a suffix chain, the wrap
    got = ref.expect(["a", "aa", "aaa"], None, 3, 0, [[1, 10, 100], [2 ** 62, 0, 0], [ref.INT64_MIN, 0, 0]], ["aaaaa", "", "b", "aa"])
    assert got.tolist() == [[5 + 40 + 300, 0, 0, 2 + 10], [ref.wrap(5 * 2 ** 62), 0, 0, ref.INT64_MIN], [ref.INT64_MIN, 0, 0, 0]]
    assert ref.wrap(5 * 2 ** 62) == 2 ** 62 and ref.wrap(2 * ref.INT64_MIN) == 0 and ref.wrap(2 ** 63) == ref.INT64_MIN
    # two needles under one handle both add its weight; a handle beyond the table is skipped
    assert ref.expect(["a", "b", "c"], [0, 0, 5], 1, 0, [[7]], ["abc", "cc"]).tolist() == [[14, 0]]
    # the empty needle adds once per position, as the oracle reports it
    m = oracle.Machine(["", "a"])
    assert ref.expect(["", "a"], None, 2, 0, [[1, 0]], ["aa"]).tolist() == [[len([v for v in m.run_list(0, b"aa")[1] if v == 0])]]
    # no needles, no haystacks
    assert ref.expect([], None, 0, 0, [[], []], ["x", ""]).tolist() == [[0, 0], [0, 0]] and ref.expect(["a"], None, 1, 0, [[1]], []).shape == (1, 0)
    # top-k: ties go to the lower haystack, in both directions; k beyond n; k == 0
    col = [5, -1, 5, 7, -1, 5]
    assert ref.top_k(col, 3) == [(7, 3), (5, 0), (5, 2)] and ref.top_k(col, 3, largest=False) == [(-1, 1), (-1, 4), (5, 0)]
    assert ref.top_k(col, 0) == [] and len(ref.top_k(col, 13)) == 6 and ref.top_k([], 4) == []
    assert ref.in_range(col, 5, 6) == [0, 2, 5] and ref.in_range(col, 5, 6, invert=True) == [1, 3, 4] and ref.in_range(col, 6, 5) == []


def steps_of(needles, values, case, hays):
    """(haystack, value) arrays of the oracle's fold over the texts, in fold order."""
    m = ref.machine(needles, values)
    hay, val = [], []
    for h, text in enumerate(hays):
        vs = ref.steps(m, case, text)
        hay += [h] * len(vs)
        val += vs
    return np.asarray(hay, np.uint32), np.asarray(val, np.uint32)


@pytest.mark.parametrize("n_cols", [1, 3, 8])
def test_the_host_mirror_is_the_definition(n_cols):
    rng = random.Random(8200 + n_cols)
    seen_empty = 0
    for needles, hays, _ in cases(6200 + n_cols, 100):
        seen_empty += "" in needles
        for ns, values, n, hs in variants(rng, needles, hays):
            weights = ref.random_weights(rng, n, n_cols)
            for case in (0, 1):
                low = [oracle.lower_utf8(x).decode() for x in ns] if case else ns
                exp = ref.expect(low, values, n, case, weights, hs)
                got = am.api.score_host(*steps_of(low, values, case, hs), len(hs), n, weights)
                assert got.dtype == np.int64 and got.shape == exp.shape and np.array_equal(got, exp), (low, values, n, weights, hs)
    assert seen_empty >= 1
    # the wrap: 2^62 five times, -2^63 twice
    got = am.api.score_host(*steps_of(["a"], None, 0, ["aaaaa", "aa"]), 2, 1, [[2 ** 62], [ref.INT64_MIN]])
    assert got.tolist() == [[2 ** 62, ref.INT64_MIN], [ref.INT64_MIN, 0]]
    # no steps, no haystacks, no values
    assert am.api.score_host([], [], 3, 2, [[1, 2]]).tolist() == [[0, 0, 0]]
    assert am.api.score_host([], [], 0, 2, [[1, 2]]).shape == (1, 0)
    assert am.api.score_host([0], [4], 1, 0, [[]]).tolist() == [[0]]
    for bad in (lambda: am.api.score_host([2], [0], 1, 1, [[1]]),                                 # a fold step beyond the haystacks
                lambda: am.api.score_host([0], [0], 1, 1, [[1]] * 9),                             # more columns than the maximum
                lambda: am.api.score_host([0], [0], 1, 1, [[1, 2]])):                             # a column of another length
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
    assert re.search(r"typedef struct am_weights am_weights;", src) and re.search(r"typedef struct am_scores am_scores;", src)
    assert re.search(r"#define AM_SCORE_MAX_COLUMNS 8", src) and am.api.SCORE_MAX_COLUMNS == 8
    assert re.search(r"typedef struct am_scored \{ int64_t score; uint32_t haystack; uint32_t reserved; \} am_scored;", src) and am.api.SCORED_DTYPE.itemsize == 16
    assert len(am.api.DEBUG_ABI) == 14                     # no new am_debug_* symbol
    for n in ("Weights", "Scores", "score_geometry", "score_host"):
        assert hasattr(am.api, n), n
    for n in ("score", "score_host_mirror"):
        assert hasattr(am.Automaton, n), n
    assert hasattr(am.SpanTable, "score_batch")
    assert hasattr(am.api.libhost(), "amh_score")
    build_py = open(os.path.join(ROOT, "alfred-margaret_amd", "build.py")).read()
    assert '"am_score.cpp"' in build_py and '"am_score.hip"' in build_py
    hpp = open(os.path.join(ROOT, "alfred-margaret_amd", "host", "automaton.hpp")).read()
    assert "scoreByHaystack" in hpp


def test_the_geometry_is_known_without_a_device():
    tile, block = am.api.score_geometry()
    assert tile >= 256 and tile % 256 == 0 and block >= 256 and block % 256 == 0      # four wavefronts, each with a whole number of 64-record steps; a thread per bin
    am.api.libam().am_score_geometry(None, None)


def test_every_argument_is_refused_before_any_device_work():
    lib = am.api.libam()
    s = am.api._Slices(["abc"])
    out = C.c_void_p(1)
    fake = C.c_void_p(1)                                   # a handle that is never looked at: the check that refuses the call comes first
    w1 = np.asarray([1], np.int64)

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and not out.value and word in lib.am_last_error(), (rc, out.value, lib.am_last_error())
        out.value = 1

    # the weights
    assert lib.am_weights_create(fake, w1.ctypes.data, 1, None) == am.AM_ERR_INVALID
    refused(lib.am_weights_create(fake, w1.ctypes.data, 0, C.byref(out)), b"n_cols")
    refused(lib.am_weights_create(fake, w1.ctypes.data, 9, C.byref(out)), b"n_cols")
    refused(lib.am_weights_create(None, w1.ctypes.data, 1, C.byref(out)), b"null needle ids")
    lib.am_weights_destroy(None)
    # the folds
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    assert lib.am_score(fake, 0, s.arr, s.n, None) == am.AM_ERR_INVALID
    refused(lib.am_score(fake, 0, None, 1, C.byref(out)), b"hay is null")
    refused(lib.am_score(fake, 1, s.arr, 0xFFFFFFFF, C.byref(out)), b"too many")
    refused(lib.am_score(fake, 0, bad, 1, C.byref(out)), b"slice with null ptr")
    refused(lib.am_score(fake, 2, s.arr, s.n, C.byref(out)), b"case_mode")
    refused(lib.am_score(None, 0, s.arr, s.n, C.byref(out)), b"null weights")
    assert lib.am_score_batch(fake, 0, fake, None) == am.AM_ERR_INVALID
    refused(lib.am_score_batch(fake, -1, fake, C.byref(out)), b"case_mode")
    refused(lib.am_score_batch(None, 0, fake, C.byref(out)), b"null weights or batch")
    refused(lib.am_score_batch(fake, 1, None, C.byref(out)), b"null weights or batch")
    assert lib.am_score_spans_batch(fake, fake, 0, fake, None) == am.AM_ERR_INVALID
    refused(lib.am_score_spans_batch(fake, fake, 7, fake, C.byref(out)), b"case_mode")
    refused(lib.am_score_spans_batch(None, fake, 0, fake, C.byref(out)), b"null span table, weights or batch")
    refused(lib.am_score_spans_batch(fake, None, 0, fake, C.byref(out)), b"null span table, weights or batch")
    refused(lib.am_score_spans_batch(fake, fake, 1, None, C.byref(out)), b"null span table, weights or batch")
    assert lib.am_matches_score(fake, fake, 1, None) == am.AM_ERR_INVALID
    refused(lib.am_matches_score(None, fake, 1, C.byref(out)), b"null matches or weights")
    refused(lib.am_matches_score(fake, None, 1, C.byref(out)), b"null matches or weights")
    refused(lib.am_matches_score(fake, fake, 0xFFFFFFFF, C.byref(out)), b"too many")
    # top-k and the selects
    n_out = C.c_uint64(5)
    row = np.zeros(1, am.api.SCORED_DTYPE)
    assert lib.am_scores_top_k(fake, 0, 1, 1, row.ctypes.data, None) == am.AM_ERR_INVALID
    assert lib.am_scores_top_k(None, 0, 1, 1, row.ctypes.data, C.byref(n_out)) == am.AM_ERR_INVALID and n_out.value == 0 and b"null scores" in lib.am_last_error()
    assert lib.am_select_top_k(fake, 0, 1, 1, fake, None) == am.AM_ERR_INVALID
    refused(lib.am_select_top_k(None, 0, 1, 1, fake, C.byref(out)), b"null scores or batch")
    refused(lib.am_select_top_k(fake, 0, 1, 0, None, C.byref(out)), b"null scores or batch")
    assert lib.am_select_score(fake, 0, 0, 1, 0, fake, None) == am.AM_ERR_INVALID
    refused(lib.am_select_score(None, 0, 0, 1, 0, fake, C.byref(out)), b"null scores or batch")
    refused(lib.am_select_score(fake, 0, 0, 1, 1, None, C.byref(out)), b"null scores or batch")
    # the accessors of a null result
    assert lib.am_scores_haystacks(None) == 0 and lib.am_scores_columns(None) == 0 and not lib.am_scores_data(None) and not lib.am_scores_device_data(None)
    lib.am_scores_free(None)
    if not _gpu():
        # valid arguments reach the runtime
        x = C.c_void_p(1)
        assert lib.am_score(fake, 0, None, 0, C.byref(x)) == am.AM_ERR_NO_DEVICE and x.value is None
        x = C.c_void_p(1)
        assert lib.am_weights_create(fake, w1.ctypes.data, 8, C.byref(x)) == am.AM_ERR_NO_DEVICE and x.value is None
    # (the refusals that need real handles -- column >= n_cols, a span table over other needle ids, a batch of another size, n_hay not above the last record's
    # haystack -- are in tests/test_gpu_score.py)


def test_without_a_gpu_the_front_end_reports_no_device():
    a = am.Automaton(["good", "bad"])                      # built on the host
    if _gpu():
        return                                             # (what the front end computes is tests/test_gpu_score.py's)
    with pytest.raises(am.AmError) as e:
        a.score(am.IGNORE_CASE, ["a good day"], [1, -1])
    assert e.value.code == am.AM_ERR_NO_DEVICE
