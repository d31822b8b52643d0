"""k_sf's straight path against the oracle (csrc/am_kernels.hip: every chunk requests its round's buckets, survivors or not -- a lane without a candidate reads
bucket 0 and ignores it --, the next chunk is prefetched by one load whose address scalar selects choose, and the latch waits for that load alone).  The texts are
tests/sf_latch_cases.py's, whose survivor counts tests/test_sf_latch_cpu.py holds to the host model; every batch goes through tests/test_gpu_sf_chunk_loop.check:
emit, count and containsAny against the oracle, and the launched instantiation against launch_sf_t's rule.
  zeros    chunks with 0 survivors between chunks with survivors (0,N,0 / N,0,0,N / units of filler only) as the first and last chunks of a unit, of a ring epoch
           and of the batch
  limits   1, 63, 64, 65, 127, 128, 129, 257 survivors in one chunk, followed by a chunk with 0 and by one with 64: the straight path into the sub-pass loop and out
  seam     a chunk that spans a haystack seam with survivors on both sides, between two straight chunks
  ends     a last chunk of 1..17 bytes; batches of one chunk per wavefront, of units of 3 chunks and of units of 18 (nothing follows a wavefront's only unit: the
           prefetch at its last chunk reads chunk 0)
  units    more units than wavefronts (the prefetch at a unit's last chunk reads the first chunk of the unit the wavefront has drawn): the smallest batch the
           launcher cuts that way -- just over 64 chunks per wavefront, two units of 33 chunks each -- whose last unit is one chunk of 1 or 17 bytes.  (The
           launcher never makes exactly n_waves + 1 units: up to 64 chunks per wavefront every wavefront gets one unit, beyond that two or more.)
  bucket 0 a needle whose entry lies in bucket 0 of the suffix table, ending on offset 0 of a chunk with no other survivor -- the 63 lanes without a survivor read
           bucket 0 and compute their window from offset 0 --, and across a haystack's start (a survivor that does not probe reads bucket 0 too): one match
Needle sets, both case modes: tests/sf_chunk_cases' small <ILP 1, LW 0>, mid <ILP 1, LW 15> (10k-style) and large <ILP 2, LW 15> (many suffixes, below the two-word
threshold), tests/scan2_filter's `large` <W2, ILP 1>, and tests/sf_latch_cases' pairs set: <ILP 2, LW 0> under IgnoreCase, the only mode that has such an image
(under CaseSensitive the same needles are <ILP 2, LW 15>).  The tests pin behaviour, not the change: they pass on the kernel as it was before."""
import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import scan2_filter as s2
from tests import sf_chunk_cases as cc
from tests import sf_latch_cases as lc
from tests.helpers import ImgCheck
from tests.test_gpu_sf_chunk_loop import Setup, check
from tests.test_sf_variants_cpu import cell_of, launch_rule

pytestmark = pytest.mark.gpu

SETS = ("small", "mid", "large", "w2", "pairs")
PARAMS = [(s, c) for s in SETS for c in (0, 1)]


class W2Setup(Setup):
    """tests/scan2_filter's `large` set plus the run's needle: the image has the derived two-word filter, and every launch beyond the light configuration is
    <W2, ILP 1, LW 15> -- which the rule of tests/test_sf_variants_cpu, written before W2, names for a cell with a small suffix table: the cell says so."""

    def __init__(self):
        self.family, self.needles = "w2", s2.needle_sets()["large"] + [cc.RUN]
        self.a, self.o = am.Automaton(self.needles), oracle.Machine(self.needles)
        self.a.set_kernel(2)
        self.vo, self.vals = self.a.values_off(), self.a.values()
        self.per_case, self.searchers = {}, {}

    def case(self, case):
        if case not in self.per_case:
            img = ImgCheck().flatten(self.o, case)
            assert s2.derived_words(ImgCheck(), img.tobytes()) is not None
            model = cc.FilterModel(img.tobytes(), case)          # (the one-word filter: what passes the two-word one passes it)
            cell = dict(cell_of(img), cap3=15)
            self.per_case[case] = (model, cc.filler_of(model, case), None, cell)
        return self.per_case[case]


class NeedlesSetup(Setup):
    """any needle set plus the run's needle"""

    def __init__(self, name, needles):
        self.family, self.needles = name, list(needles) + [cc.RUN]
        self.a, self.o = am.Automaton(self.needles), oracle.Machine(self.needles)
        self.a.set_kernel(2)
        self.vo, self.vals = self.a.values_off(), self.a.values()
        self.per_case, self.searchers = {}, {}

    def case(self, case):
        if case not in self.per_case:
            img = ImgCheck().flatten(self.o, case)
            model = cc.FilterModel(img.tobytes(), case)
            self.per_case[case] = (model, cc.filler_of(model, case), None, cell_of(img))
        return self.per_case[case]


_SETUPS = {}


def setup_of(name):
    if name not in _SETUPS:
        _SETUPS[name] = (W2Setup() if name == "w2" else NeedlesSetup(name, lc.ilp2_lw0_needles()) if name == "pairs"
                         else NeedlesSetup(name, [lc.bucket0_word()]) if name == "bucket0" else Setup(name))
    return _SETUPS[name]


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


def _batch(s, case, chunks_per_wave, r):
    w = 16 * am.device_info()["n_cu"]
    total = (chunks_per_wave * w - 1) * 1024 + r
    uc = am.api.sf_unit_chunks(total)
    assert uc == chunks_per_wave, (total, uc)
    fill = s.case(case)[1]
    return lc.latch_batch(fill, case, total, uc) + (uc,)


@pytest.mark.parametrize("chunks_per_wave,r", [(3, 17), (18, 1)])
@pytest.mark.parametrize("name,case", PARAMS)
def test_zero_survivor_chunks_queue_limits_and_a_seam_in_units_of_several_chunks(name, case, chunks_per_wave, r):
    s = setup_of(name)
    text, offs, placed, uc = _batch(s, case, chunks_per_wave, r)
    exp = check(s, case, text, offs)
    assert len(exp[0]) == lc.expected_matches(placed, uc)


@pytest.mark.parametrize("name,case", PARAMS)
def test_one_chunk_per_wavefront_and_a_last_chunk_of_1_to_17_bytes(name, case):
    """17 KiB + r: beyond the light configuration, every wavefront has one one-chunk unit, the last one r bytes of it"""
    s = setup_of(name)
    fill = s.case(case)[1]
    for r in range(1, 18):
        total = 17 * 1024 + r
        text, offs, placed = lc.latch_batch(fill, case, 96 * 1024 + r, 1) if r in (1, 17) else (cc.end_batch(fill, cc.run(4, case), total) + (None,))
        exp = check(s, case, text, offs)
        if placed is None:
            assert len(exp[0]) == 1 and int(exp[1][0]) + int(offs[exp[0][0]]) == total
        else:
            assert len(exp[0]) == lc.expected_matches(placed, 1)


@pytest.mark.parametrize("name,case", [p for p in PARAMS if p[0] != "w2"])
def test_the_traced_instantiation_finds_the_same(name, case):
    """(not the two-word set: under AM_SF_TRACE the rule names <ILP 2> for its cell, the launcher's traced W2 instantiation is <ILP 1>, and no cell says both;
    tests/test_gpu_scan2_filter.py holds that instantiation to the oracle)"""
    s = setup_of(name)
    text, offs, placed, uc = _batch(s, case, 3, 5)
    exp = check(s, case, text, offs, traced=True)
    assert len(exp[0]) == lc.expected_matches(placed, uc)


def test_the_pairs_set_is_ilp_2_lw_0_under_ignore_case():
    s = setup_of("pairs")
    v = launch_rule(s.case(1)[3], 1, "emit", 64)
    assert (v["ilp"], v["lw"], v["short"], v["children"], v["light"]) == (2, 0, False, False, False)
    v = launch_rule(s.case(0)[3], 0, "emit", 64)
    assert (v["ilp"], v["lw"], v["short"], v["children"]) == (2, 15, False, False)


@pytest.mark.parametrize("name,case,r", [("w2", 1, 1), ("w2", 1, 17), ("w2", 0, 17), ("mid", 0, 1), ("mid", 1, 17), ("large", 0, 17), ("large", 1, 1), ("pairs", 1, 17),
                                         ("pairs", 0, 1)])
def test_more_units_than_wavefronts_and_a_last_unit_of_one_short_chunk(name, case, r):
    """33 * (2 w - 1) whole chunks and r bytes, w = 16 wavefronts on every CU: 66 chunks per wavefront, so units of 33 chunks, 2 w - 1 whole ones and the last
    of one chunk of r bytes, which some wavefront draws and prefetches at the last chunk of its second unit"""
    s = setup_of(name)
    w = 16 * am.device_info()["n_cu"]
    total = 33 * (2 * w - 1) * 1024 + r
    uc = am.api.sf_unit_chunks(total)
    n_units = ((total + 1023) // 1024 + uc - 1) // uc
    assert uc == 33 and n_units == 2 * w, (total, uc, n_units)
    fill = s.case(case)[1]
    text, offs, placed = lc.latch_batch(fill, case, total, uc)
    last = (total + 1023) // 1024 - 1
    assert last % uc == 0 and placed.get(last - 2) == lc.N          # the last unit is the partial chunk alone; survivors in the unit before it
    exp = check(s, case, text, offs)
    assert len(exp[0]) == lc.expected_matches(placed, uc)


@pytest.mark.parametrize("case", (0, 1))
def test_an_entry_in_bucket_0_is_found_once_and_only_where_it_is(case):
    s = setup_of("bucket0")
    word = lc.bucket0_word()
    model, fill, _, cell = s.case(case)
    assert cell["cap3"] == 2 and lc.t4_bucket_a(word, 2) == 0 and lc.t4_bucket_b(word, 2) == 0          # four buckets, and the word's entry is in bucket 0
    for straddle in (1, 2, 3):
        text, offs, want = lc.bucket0_batch(fill, word, 20 * 1024, straddle)
        counts = model.per_chunk(text)
        assert counts[5] == 1 and counts[9] == 1 and counts.sum() == 2          # one survivor in chunk 5 (offset 0), one at the haystack's start
        exp = check(s, case, text, offs)
        assert exp[0].tolist() == [0] and exp[1].tolist() == [5 * 1024 + 1]
