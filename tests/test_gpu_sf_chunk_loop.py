"""k_sf's chunk loop at its limits (csrc/am_kernels.hip: the compaction's total and the sub-pass loop it steers, the order of the filter's reads and of the bits they
are shifted into, the probe round's queue and stage reads, the haystack start that decides whether a candidate's window fits), against the oracle.  The texts are
those of tests/sf_chunk_cases.py -- its host model of the filter stage counts the candidates of every chunk, tests/test_sf_chunk_loop_cpu.py holds the builders to it on the CPU, and the cases below assert the count they were built
for --, the needles are a family of tests/helpers.py plus the run's needle: <ILP 1, LW 0> (small), <ILP 1, LW 15> (mid), <ILP 2, LW 15> (large), SHORT (mid+short),
CHILDREN (dict), in both case modes.  Every call goes to k_sf (am_automaton_set_kernel(a, 2); AM_DFA = 0 for the Searchers) and the instantiation it launched is
held to launch_sf_t's rule.  Records are expanded and compared with the oracle's, must ascend strictly, and counts and flags must agree with them.
  queue limits   0, 1, 63 .. 257 and 1 024 candidates in ONE chunk: one queue entry per lane | two, one sub-pass | several with stale entries behind the last one's;
                 in a 3-KiB batch (the light configuration), a 20-KiB one, and as the first and the last chunk of work units of several chunks; also containsAll,
                 and once more under AM_SF_TRACE (the same bytes)
  bit order      the only match of a batch ends at offset 16 L + k of its chunk, L in {0, 1, 31, 62, 63}, k in 0..15 (k < 3 in lane 0: the window reaches into the
                 chunk before, which is another unit's or the same unit's)
  batch end      1 024 m + r bytes, r = 1..17, m in {0, 1, 16}, a match on the last byte
  haystack start the candidate's chunk lies inside one haystack that starts 0..5 bytes before it: the run's four bytes ending on offsets 0..3 of the chunk (a match
                 when they begin at or behind the start: among them the run that ends 3 bytes behind the start, no match, and 4, a match) and a longer needle
                 from before the start into the chunk (no match); the start inside the candidate's chunk, where every candidate looks its haystack up; also
                 under AM_SF_TRACE"""
import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import sf_chunk_cases as cc
from tests.helpers import ImgCheck, sf_expand, sf_oracle_records
from tests.test_sf_variants_cpu import PURPOSE, cell_of, launch_rule

pytestmark = pytest.mark.gpu

PARAMS = [(f, c) for f in cc.FAMILIES for c in (0, 1)]
SIZES = {"light": 1, "full": 18}          # chunks of filler behind the chunk under test: 3 KiB (256-thread workgroups) and 20 KiB


class Setup:
    """the automaton (suffix-filter route), the oracle's machine, the filter model, the filler and the Searchers of a family plus the run's needle"""

    def __init__(self, family):
        self.family, self.needles = family, cc.needles_of(family)
        self.a, self.o = am.Automaton(self.needles), oracle.Machine(self.needles)
        self.a.set_kernel(2)
        self.vo, self.vals = self.a.values_off(), self.a.values()
        self.per_case, self.searchers = {}, {}

    def case(self, case):
        if case not in self.per_case:
            img = ImgCheck().flatten(self.o, case)
            model = cc.FilterModel(img.tobytes(), case)
            fill = cc.filler_of(model, case)
            self.per_case[case] = (model, fill, cc.long_needle_of(self.needles, self.o, case, fill), cell_of(img))
        return self.per_case[case]

    def searcher(self, case):
        if case not in self.searchers:
            self.searchers[case] = am.Searcher(case, self.needles)
        return self.searchers[case]


_SETUPS = {}


def setup_of(family):
    if family not in _SETUPS:
        _SETUPS[family] = Setup(family)
    return _SETUPS[family]


@pytest.fixture(scope="module", autouse=True)
def _release_at_the_end():
    yield
    _SETUPS.clear()
    am.api.libam().am_release_device_memory()
    am.api.libam().am_release_host_memory()


@pytest.fixture(autouse=True)
def _k_sf_only():
    am.debug_set("AM_DFA", 0)
    am.debug_set("AM_SF_TRACE", -1)
    am.api.sf_last_variant()          # (reading clears)
    yield
    am.debug_set("AM_SF_TRACE", -1)


def launched(call, cell, case, mode, total, trace=False):
    """call(), then the k_sf instantiation it launched against the rule's"""
    assert am.api.sf_last_variant() is None
    out = call()
    got, want = am.api.sf_last_variant(), launch_rule(cell, case, mode, (total + cc.CHUNK - 1) // cc.CHUNK, trace)
    assert got == want, (mode, total, got, want)
    return out


def slices(text, offs):
    return [text[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def strictly_ascending(rs):
    k = (rs["haystack"].astype(np.uint64) << np.uint64(32)) | rs["end_pos"].astype(np.uint64)
    return bool((k[1:] > k[:-1]).all())


def check(s, case, text, offs, contains_all=False, traced=False):
    """emit, count and containsAny (containsAll, a traced emit) of one batch against the oracle; returns the oracle's (haystack, end, value) arrays"""
    cell = s.case(case)[3]
    hays, total = slices(text, offs), len(text)
    exp = sf_oracle_records(s.o, case, text, offs)
    rs = launched(lambda: s.a.run_records(case, hays), cell, case, "emit", total)
    got = sf_expand(rs["haystack"], rs["state"], rs["end_pos"], s.vo, s.vals)
    assert all(np.array_equal(g, e) for g, e in zip(got, exp)), (len(got[0]), len(exp[0]))
    assert strictly_ascending(rs)
    assert len(rs) == 0 or int((rs["end_pos"].astype(np.int64) + offs[rs["haystack"]]).max()) <= total          # no record beyond the batch's last byte
    counts = launched(lambda: s.a.count_matches(case, hays), cell, case, "count", total)
    assert np.array_equal(counts, np.bincount(exp[0], minlength=len(hays)))
    flags = launched(lambda: s.searcher(case).contains_any_batch(hays), cell, case, "any", total)
    assert np.array_equal(flags, counts > 0)
    if contains_all:
        want = [s.o.contains_all(case, h) for h in hays]          # (thousands of needles: no haystack holds them all; the launch still queues every candidate)
        got_all = launched(lambda: s.searcher(case).contains_all_batch(hays), cell, case, "ids", total)
        assert got_all.tolist() == want
    if traced:
        am.debug_set("AM_SF_TRACE", 1)
        try:
            again = launched(lambda: s.a.run_records(case, hays), cell, case, "emit", total, trace=True)
            again_counts = launched(lambda: s.a.count_matches(case, hays), cell, case, "count", total, trace=True)
        finally:
            am.debug_set("AM_SF_TRACE", -1)
        assert again.tobytes() == rs.tobytes() and np.array_equal(again_counts, counts)
    return exp


@pytest.mark.parametrize("family,case", PARAMS)
def test_the_full_size_launch_is_the_instantiation_the_family_is_here_for(family, case):
    v = launch_rule(setup_of(family).case(case)[3], case, "emit", 20)
    assert (v["ilp"], v["lw"], v["short"], v["children"]) == PURPOSE[family] and not v["light"]
    assert launch_rule(setup_of(family).case(case)[3], case, "emit", 3)["light"]


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("family,case", PARAMS)
def test_queue_limits_in_one_chunk(family, case, size):
    s = setup_of(family)
    model, fill, _, _ = s.case(case)
    for n in cc.QUEUE_NS + ("every",):
        text, offs, want = cc.queue_batch(fill, case, n, SIZES[size])
        counts = model.per_chunk(text)
        assert counts[1] == want and counts.sum() == want          # what the case exercises: `want` candidates in chunk 1, none anywhere else
        exp = check(s, case, text, offs, contains_all=True, traced=True)
        assert len(exp[0]) == want


@pytest.mark.parametrize("family,case", PARAMS)
def test_queue_limits_in_the_first_and_the_last_chunk_of_a_unit(family, case):
    """the batch size comes from the device, as in tests/test_gpu_scan_filter.test_units_of_several_chunks: work units of two chunks or more"""
    s = setup_of(family)
    model, fill, _, _ = s.case(case)
    w = 16 * am.device_info()["n_cu"]
    total = (2 * w + w // 4) * 1024 + 19
    uc = am.api.sf_unit_chunks(total)
    assert uc >= 2, (total, uc)
    text, offs, placed = cc.unit_batch(fill, case, total, uc)
    counts = model.per_chunk(text)
    assert {c: int(counts[c]) for c, _ in placed} == dict(placed) and counts.sum() == sum(n for _, n in placed)
    assert all(c % uc in (0, uc - 1) for c, _ in placed) and {c % uc for c, _ in placed} == {0, uc - 1}
    exp = check(s, case, text, offs, contains_all=True, traced=True)
    assert len(exp[0]) == sum(n for _, n in placed) - 3          # (the run that fills a unit's first chunk: its first three windows begin in the haystack before)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("family,case", PARAMS)
def test_bit_k_of_a_lane_is_position_k(family, case, size):
    s = setup_of(family)
    model, fill, long_needle, _ = s.case(case)
    total = (2 + SIZES[size]) * cc.CHUNK
    for lane in cc.BIT_LANES:
        for k in range(16):
            at = cc.CHUNK + 16 * lane + k          # chunk 1 is the first chunk of its (one-chunk) unit; lane 0, k < 3: the window begins in chunk 0
            text, offs = cc.single_match_batch(fill, long_needle, at, total)
            assert model.passing(text)[at]
            exp = check(s, case, text, offs)
            assert exp[0].tolist() == [0] and exp[1].tolist() == [at + 1]


@pytest.mark.parametrize("family,case", PARAMS)
def test_bit_k_in_a_chunk_that_is_not_the_first_of_its_unit(family, case):
    s = setup_of(family)
    model, fill, long_needle, _ = s.case(case)
    w = 16 * am.device_info()["n_cu"]
    total = (2 * w + w // 4) * 1024 + 19
    uc = am.api.sf_unit_chunks(total)
    assert uc >= 2, (total, uc)
    for k in (0, 1, 2):
        at = (uc + 1) * cc.CHUNK + k               # the second chunk of the second unit: lane 0's bytes before the chunk come out of the carry
        text, offs = cc.single_match_batch(fill, long_needle, at, total)
        assert model.passing(text)[at]
        exp = check(s, case, text, offs)
        assert exp[0].tolist() == [0] and exp[1].tolist() == [at + 1]


@pytest.mark.parametrize("family,case", PARAMS)
def test_the_batch_ends_inside_a_lane(family, case):
    s = setup_of(family)
    model, fill, long_needle, _ = s.case(case)
    for m in (0, 1, 16):
        for r in range(1, 18):
            total = 1024 * m + r
            needle = long_needle if total >= len(long_needle) else cc.run(4, case) if total >= 4 else None
            text, offs = cc.end_batch(fill, needle, total)
            exp = check(s, case, text, offs)
            assert len(exp[0]) == (needle is not None)
            if needle is not None:
                assert int(exp[1][0]) + int(offs[exp[0][0]]) == total and model.passing(text)[total - 1]          # the match ends on the batch's last byte


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("family,case", PARAMS)
def test_a_chunk_inside_one_haystack_that_starts_0_to_5_bytes_before_it(family, case, size):
    """c0 - hs0 = 0..5 for chunk 1, which lies inside one haystack and holds the batch's only candidate: the run's four bytes ending on offsets 0..3 of the chunk
    (a match exactly when all four lie behind the start -- this includes the run that ends 3 bytes behind the start, for c0 - hs0 <= 2, and the one that ends 4 bytes
    behind it, for c0 - hs0 <= 3), and a longer needle that begins one byte before the start and ends inside the chunk (never a match)"""
    s = setup_of(family)
    model, fill, long_needle, _ = s.case(case)
    total = (2 + SIZES[size]) * cc.CHUNK
    for into in cc.HAY_INTO:
        for what in (0, 1, 2, 3, "across"):
            text, offs, want, last = cc.single_chunk_start_batch(fill, case, long_needle, into, what, total)
            counts = model.per_chunk(text)
            assert model.passing(text)[last] and counts[1] > 0 and counts[2:].sum() == 0          # the candidate is in chunk 1 ...
            if what != "across":
                assert counts.tolist() == [0, 1] + [0] * (len(counts) - 2)          # ... alone (the long needle's inner windows, some of them in chunk 0, may pass too)
            exp = check(s, case, text, offs, traced=True)
            assert len(exp[0]) == want
            if want:
                assert exp[0].tolist() == [1] and exp[1].tolist() == [what + 1 + into]


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("family,case", PARAMS)
def test_a_haystack_that_starts_inside_the_chunk_of_its_first_candidates(family, case, size):
    """the chunk that holds the run's candidate also holds the haystack's start: every candidate of such a chunk looks its haystack up.  The start 4 and 5 bytes
    before the end of chunk 0, 100 bytes into chunk 1 and 4 bytes before its end; the run's four bytes end 3 bytes behind the start (no match) and 4 (a match,
    end 4); the longer needle lies across the start with the start in its middle (no match; its last byte is in the start's chunk or the first of the next)"""
    s = setup_of(family)
    model, fill, long_needle, _ = s.case(case)
    total = (2 + SIZES[size]) * cc.CHUNK
    for hs0 in [cc.CHUNK - 4, cc.CHUNK - 5, cc.CHUNK + 100, 2 * cc.CHUNK - 4]:
        for what in (3, 4, "across"):
            text, offs, want = cc.hay_start_batch(fill, case, long_needle, hs0, what, total)
            counts = model.per_chunk(text)
            last = hs0 + what - 1 if what != "across" else hs0 - len(long_needle) // 2 + len(long_needle) - 1
            assert model.passing(text)[last] and last // cc.CHUNK - hs0 // cc.CHUNK in ((0,) if what != "across" else (0, 1))
            assert what == "across" or counts.sum() == 1          # the run's candidate is the batch's only one, in the chunk the start lies in
            exp = check(s, case, text, offs, traced=True)
            assert len(exp[0]) == want
            if want:
                assert exp[0].tolist() == [1] and exp[1].tolist() == [4]
