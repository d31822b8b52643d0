"""The storage tiers of the table walk (csrc/am_dfa.hip dfa_step), on the CPU: the mid-size automaton of tests/helpers.py (dfa_tier_needles) must leave LDS in every
direction, its text (dfa_tier_text) must send enough steps to every tier under both launch shapes, and the plain walk that says so (dfa_tier_census) must itself find
the oracle's positions.  tests/test_gpu_dfa_tiers.py leans on all three: a GPU test that passes on an image that never leaves LDS says nothing.  CPU only."""
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers as H

CASES = (0, 1)
SHAPES = {"two per CU": H.DFA_LDS_TWO_PER_CU, "one per CU": H.DFA_LDS_ONE_PER_CU}
ALIAS_CHUNK = 128      # see test_alias_floors_of_both_cache_forms


class Tier:
    def __init__(self, chk, case):
        needles = H.dfa_tier_needles()
        self.case = case
        self.needles = [oracle.lower_utf8(n).decode() for n in needles] if case else needles
        self.oracle = oracle.Machine(self.needles)
        chk.set("AM_DFA", 1)
        try:
            self.img = chk.flatten(am.Automaton(self.needles), case)
        finally:
            chk.set("AM_DFA", -1)
        self.figures = H.dfa_header_preconditions(self.img)       # a flattener change that breaks one fails every test of this file here: none goes quiet
        self.hays = H.dfa_tier_text(self.needles, case)
        self.expected = H.oracle_triples(self.oracle, case, self.hays)
        self._census = {}

    def census(self, shape, chunk):
        if (shape, chunk) not in self._census:
            self._census[shape, chunk] = H.dfa_tier_census(self.img, self.hays, *SHAPES[shape], chunk)
        return self._census[shape, chunk]


@pytest.fixture(scope="module")
def chk():
    return H.ImgCheck()


@pytest.fixture(scope="module")
def tiers(chk):
    return {case: Tier(chk, case) for case in CASES}


@pytest.mark.parametrize("case", CASES)
def test_header_preconditions(tiers, case):
    """Rows, single-entry and two-entry records beyond the LDS shares of both launch shapes (1 008 / 2 048 / 1 024), columns beyond the 32 of the LDS rows and the 16 of
    the hot table, more states than 8 192 slots and one tag bit tell apart, a state of 16 values and more; and no byte without a column (the census refuses those)."""
    f = tiers[case].figures
    print(case, f)
    assert f["n_rows"] >= 1100 and f["n_single"] >= 2200 and f["n_two"] >= 1100 and f["log2_classes"] >= 6 and f["n_states"] > 16384 and f["max_values"] >= 16
    assert f["n_rows"] > max(s[0] for s in SHAPES.values()) and f["n_single"] > max(s[1] for s in SHAPES.values()) and f["n_two"] > max(s[2] for s in SHAPES.values())
    assert (1 << f["log2_classes"]) > H.DFA_LDS_COLS > (1 << f["hot_log2"])
    assert f["rare_bytes"] == 0


def test_the_text_is_ragged(tiers):
    for t in tiers.values():
        sizes = [len(h) for h in t.hays]
        assert 256 << 10 >= sum(sizes) > (256 << 10) - 4 and max(sizes) > 8208 and any(a == 0 and b == 0 for a, b in zip(sizes, sizes[1:]))
        for h in t.hays:
            h.decode("utf-8")                                      # cut on code-point boundaries


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("case", CASES)
def test_census_floors(tiers, case, shape):
    """Every tier of DFA_TIERS takes at least 200 steps of the text under either launch shape; ends of 14, 15 and 16 values (kDfaEndLookUp = 15 between them) at least 4
    times each, 2 and more of them past a haystack seam inside their unit of 2 048 bytes."""
    c = tiers[case].census(shape, 2048)
    print(case, shape, c["tiers"], {v: c["end_values"].count(v) for v in range(13, 21)}, len(c["seam_ends"]))
    H.dfa_census_floors(c)
    assert c["tiers"]["class0"] >= 200


@pytest.mark.parametrize("case", CASES)
def test_alias_floors_of_both_cache_forms(tiers, case):
    """k_dfa_place's table of seen states: groups of 64 units whose records fit one superblock (at most 3 072), each with 10 and more pairs of distinct end states that
    share a slot of the 4-byte form (equal modulo 8 192: only the tag tells them apart) and 10 and more that share one of the 8-byte form (equal under its hash).
    The chunk is 128, not 256: this text ends something every 2 to 4 bytes, so a group of 64 x 256 bytes holds 2 950 - 3 050 records CaseSensitive and 5 300 - 5 500 IgnoreCase;
    at 128 it holds half of that, at most 3 072 in both cases, and still hundreds of pairs."""
    c = tiers[case].census("two per CU", ALIAS_CHUNK)
    print(case, [(g["records"], g["alias_low"], g["alias_hash"]) for g in c["groups"]])
    assert len(H.dfa_alias_groups(c)) == len(c["groups"]) >= 4


@pytest.mark.parametrize("case", CASES)
def test_the_census_finds_the_oracles_positions(tiers, case):
    """The census is a walk of its own: what it calls an end must be where the oracle reports, and the list lengths it reads from the end bits and out[] the oracle's."""
    t = tiers[case]
    c = t.census("two per CU", 2048)
    assert c["ends"] == sorted(set((h, p) for h, p, _ in t.expected)) and len(c["ends"]) > 40_000
    per_end = {}
    for h, p, _ in t.expected:
        per_end[h, p] = per_end.get((h, p), 0) + 1
    assert c["end_values"] == [per_end[e] for e in c["ends"]]
    for shape in SHAPES:
        assert t.census(shape, 2048)["ends"] == c["ends"]


def test_the_census_refuses_an_image_with_rare_bytes(chk):
    chk.set("AM_DFA", 1)
    chk.set("AM_DFA_RARE_PERMILLE", 400)
    try:
        img = chk.flatten(am.Automaton(["ab", "abc", "bcd", "cde", "xyz", "a1", "B2", "ya", "aB1"]), 0)
    finally:
        chk.set("AM_DFA", -1)
        chk.set("AM_DFA_RARE_PERMILLE", -1)
    assert 0xFF in H.dfa_tables(img)["cls"].tolist()
    with pytest.raises(ValueError):
        H.dfa_tier_census(img, [b"abcxyzB2"], *H.DFA_LDS_TWO_PER_CU, 2048)


@pytest.mark.parametrize("chunk", [64, 256, 2048, 8192, 8208])
@pytest.mark.parametrize("case", CASES)
def test_host_interpreter_equals_the_oracle(chk, tiers, case, chunk):
    """dfa_scan_unit (am_image.h), the plain form of k_dfa's walk, over the same image and text: the oracle's triples at units of 64 bytes up to the last token unit
    (8 192) and the first two-walk unit (8 208)."""
    t = tiers[case]
    img = t.img.copy()
    chk.set_dfa_chunk(img, chunk)
    n, recs = chk.scan(img, 3, t.hays)
    assert n >= 0
    assert H.expand_records(t.oracle.values_off(), t.oracle.values(), recs[0], recs[1], recs[2]) == t.expected
