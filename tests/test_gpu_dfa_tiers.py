"""k_dfa and k_dfa_place (csrc/am_dfa.hip) on every storage tier a transition can come from, in both case modes: the mid-size automaton and text of tests/helpers.py
(dfa_tier_needles, dfa_tier_text; tests/test_dfa_tiers_cpu.py says what they are) under the launch shapes AM_DFA_TUNE can force, against the oracle over the whole
batch.  Needs an MI355X.

The fragment-pool automata of tests/test_gpu_dfa.py live inside LDS (a few hundred states, fewer than 32 classes) and the dictionary that leaves it is IgnoreCase and
held to the oracle on a sample; here rows, hot columns, cold columns, records of both kinds in LDS and in global memory, the look-ahead, both forms of k_dfa_place's table
with aliasing states, and the count path of 15 values and more each take hundreds of steps, counted by a plain walk of the very image the device walks."""
import ctypes as C

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu

CASES = (0, 1)
TUNES = (0x20, 0x21, 0x23, 0x10, 0x11, 0x13, 0x1000020, 0x1000023, 0x120, 0x123, 0x6520, 0x2000020)
ALIAS_CHUNK = 128      # tests/test_dfa_tiers_cpu.py test_alias_floors_of_both_cache_forms: at 256 a group's records do not fit one superblock
SWITCHES = ("AM_DFA", "AM_DFA_CHUNK", "AM_DFA_TUNE", "AM_SF_POOL_BLOCKS")


class Tier:
    """One case mode: the needles, the oracle, the text and what the oracle says about it -- computed once, read by every test."""

    def __init__(self, case):
        needles = H.dfa_tier_needles()
        self.case = case
        self.needles = [oracle.lower_utf8(n).decode() for n in needles] if case else needles
        self.oracle = oracle.Machine(self.needles)
        self.hays = H.dfa_tier_text(self.needles, case)
        self.run_hays = H.dfa_tier_text(self.needles, case, 1, 96 << 10, runs_only=True)
        self.expected = H.oracle_triples(self.oracle, case, self.hays)
        self.automata = {}

    def automaton(self, chunk):
        """One automaton per unit size (AM_DFA and AM_DFA_CHUNK are read when the image is flattened; AM_DFA_TUNE at every launch)."""
        if chunk not in self.automata:
            am.debug_set("AM_DFA", 1)
            am.debug_set("AM_DFA_CHUNK", chunk)
            a = am.Automaton(self.needles)
            a.set_kernel(3)
            img = a.image_bytes(self.case)
            assert H.ImgCheck.dfa_header(np.frombuffer(img, np.uint8))["chunk"] == chunk
            self.automata[chunk] = (a, img)
        return self.automata[chunk]

    def checked_automaton(self, chunk):
        """... and at every use: the image the device holds is still the one the fixture's census walked, and the unit is the image's (am_run.cpp make_plan gives a small
        batch smaller units unless AM_DFA_CHUNK is set)"""
        a, img = self.automata[chunk]
        assert a.image_bytes(self.case) == img
        am.debug_set("AM_DFA", 1)
        am.debug_set("AM_DFA_CHUNK", chunk)
        return a


@pytest.fixture(scope="module")
def tiers():
    """The preconditions and the census floors again, on the image the DEVICE walks (a.image_bytes): this file cannot pass on an image that never leaves LDS."""
    try:
        out = {case: Tier(case) for case in CASES}
        for t in out.values():
            _, img = t.automaton(2048)
            H.dfa_header_preconditions(img)
            for shape in (H.DFA_LDS_TWO_PER_CU, H.DFA_LDS_ONE_PER_CU):
                c = H.dfa_tier_census(img, t.hays, *shape, 2048)
                H.dfa_census_floors(c)
                assert c["ends"] == sorted(set((h, p) for h, p, _ in t.expected))
            runs = H.dfa_tier_census(img, t.run_hays, *H.DFA_LDS_TWO_PER_CU, 2048)
            assert sum(v >= H.DFA_END_LOOK_UP for v in runs["end_values"]) * 4 >= len(runs["ends"]) and len(runs["seam_ends"]) >= 100      # mostly runs, split over seams
            _, img = t.automaton(ALIAS_CHUNK)
            assert len(H.dfa_alias_groups(H.dfa_tier_census(img, t.hays, *H.DFA_LDS_TWO_PER_CU, ALIAS_CHUNK))) >= 4
    finally:
        for s in SWITCHES:
            am.debug_set(s, -1)
    return out


@pytest.fixture()
def switches():
    yield
    for s in SWITCHES:
        am.debug_set(s, -1)


def profile(call):
    lib = am.api.libam()
    am.api.check(lib.am_profile_reset()); am.api.check(lib.am_profile_enable(1))
    try:
        out = call()
    finally:
        am.api.check(lib.am_profile_enable(0))
    n = {}
    for name in ("dfa", "dfa_place"):
        ms, k = C.c_double(0), C.c_uint64(0)
        am.api.check(lib.am_profile_read(name.encode(), C.byref(ms), C.byref(k)))
        n[name] = int(k.value)
    return out, n


def batch_counts(a, case, hays):
    """(per-haystack counts, total_out, flags) of am_count_batch / am_contains_any_batch over an uploaded batch"""
    lib = am.api.libam()
    s = am.api._Slices(hays)
    b = C.c_void_p()
    am.api.check(lib.am_batch_upload(s.arr, s.n, C.byref(b)))
    try:
        counts, tot, flags = np.zeros(s.n, np.uint64), C.c_uint64(0), np.zeros(s.n, np.uint8)
        am.api.check(lib.am_count_batch(a.device, case, b, counts.ctypes.data, C.byref(tot)))
        am.api.check(lib.am_contains_any_batch(a.device, case, b, flags.ctypes.data))
        return counts, int(tot.value), flags
    finally:
        lib.am_batch_destroy(b)


def contains_any(a, case, hays):
    s = am.api._Slices(hays)
    out = np.zeros(max(s.n, 1), np.uint8)
    am.api.check(am.api.libam().am_contains_any(a.device, case, s.arr, s.n, out.ctypes.data))
    return [bool(x) for x in out[:s.n]]


def check_whole_batch(t, a, tag):
    """records -> the oracle's triples over the WHOLE batch, one record per position in order; counts per haystack (am_count and am_count_batch), the total of
    values, the flags of both entry points: the oracle's."""
    o, case, hays = t.oracle, t.case, t.hays
    recs = a.run_records(case, hays)
    keys = list(zip(recs["haystack"].tolist(), recs["end_pos"].tolist()))
    assert keys == sorted(set(keys)), tag
    assert H.expand_records(o.values_off(), o.values(), recs["haystack"], recs["state"], recs["end_pos"]) == t.expected, tag
    per_hay = np.bincount([h for h, _, _ in t.expected], minlength=len(hays)).astype(np.uint64)
    assert np.array_equal(a.count_matches(case, hays), per_hay), tag
    counts, total, flags = batch_counts(a, case, hays)
    assert np.array_equal(counts, per_hay) and total == len(t.expected), tag
    assert [bool(f) for f in flags] == [bool(c) for c in per_hay] == contains_any(a, case, hays), tag


@pytest.mark.parametrize("tune", TUNES, ids=[hex(t) for t in TUNES])
@pytest.mark.parametrize("case", CASES)
def test_every_tier_under_every_launch_shape(tiers, switches, case, tune):
    """Units of 2 048 bytes.  The tunes force two workgroups per CU (0x2.: 512 rows, 640 + 640 records in LDS) or one (0x1.: 1 008, 2 048 + 1 024), so the census of the
    fixture knows what sits where; the three walks (.0 / .1 / .3); no records in LDS (bit 24: every record from global memory or the look-ahead); no rows in LDS
    (0x12.: the hot table and the cold rows take every row state); 100 rows in LDS (0x65..); k_dfa_place's 8-byte entries (bit 25)."""
    t = tiers[case]
    a = t.checked_automaton(2048)
    am.debug_set("AM_DFA_TUNE", tune)
    check_whole_batch(t, a, (case, hex(tune)))


@pytest.mark.parametrize("tune", (0x20, 0x2000020), ids=["4-byte entries", "8-byte entries"])
@pytest.mark.parametrize("case", CASES)
def test_aliasing_states_in_both_forms_of_the_place_table(tiers, switches, case, tune):
    """Units of 128 bytes: every group of 64 units holds at most 3 072 records -- its wavefront's one superblock -- with dozens of pairs of distinct end states in one slot
    of k_dfa_place's table, told apart by the tag (4-byte entries, states beyond 8 192) or by the whole state (8-byte entries under the hash).  Every wavefront takes
    at most one group; one walk, and the records come out of k_dfa_place."""
    t = tiers[case]
    a = t.checked_automaton(ALIAS_CHUNK)
    n_units = (sum(len(h) for h in t.hays) + ALIAS_CHUNK - 1) // ALIAS_CHUNK
    n_groups = (n_units + 63) // 64
    workgroups = min(am.device_info()["n_cu"] * 2, (n_groups + 15) // 16)          # dfa_launch_shape, two workgroups per CU
    assert n_groups <= 16 * workgroups
    am.debug_set("AM_DFA_TUNE", tune)
    _, n = profile(lambda: a.run_records(case, t.hays))
    assert n["dfa"] == 1 and n["dfa_place"] >= 1, n
    check_whole_batch(t, a, (case, hex(tune)))


@pytest.mark.parametrize("walk", (0x20, 0x23), ids=["walk 0", "walk 3"])
@pytest.mark.parametrize("case", CASES)
def test_count_path_of_15_values_and_more(tiers, switches, case, walk):
    """kDfaEndLookUp: a position that reports fewer than 15 values adds its end bits to a 32-bit sum, one of 15 and more reads out[] and adds to the 64-bit sums at once.
    A batch that is mostly runs of QzQz..., every other one split by a haystack seam: a quarter and more of its positions report 15 to 20 values, 14 and 16 next to them.
    Counts per haystack and the total of am_count_batch, am_count per haystack: the oracle's."""
    t = tiers[case]
    a = t.checked_automaton(2048)
    am.debug_set("AM_DFA_TUNE", walk)
    per_hay = np.asarray([t.oracle.count_matches(case, h) for h in t.run_hays], dtype=np.uint64)
    counts, total, _ = batch_counts(a, case, t.run_hays)
    assert total == int(per_hay.sum()) and np.array_equal(counts, per_hay)
    assert np.array_equal(a.count_matches(case, t.run_hays), per_hay)
