"""The texts of tests/sf_latch_cases.py are what they claim, on the CPU: the host model of k_sf's filter stage (tests/sf_chunk_cases.FilterModel) counts in every
chunk exactly the survivors the builder promises -- the zeros between them included, and none anywhere else in the batch --, and the oracle finds a match for every
survivor but the seam's three whose windows begin in the haystack before.  Units of 3 chunks (what a batch of a few MiB gets on the device) and of 18 (a ring epoch's
end inside the unit); the families are the straight path's: <ILP 1, LW 0>, <ILP 1, LW 15>, <ILP 2, LW 15>."""
import pytest

from tests import sf_latch_cases as lc
from tests.helpers import sf_oracle_records
from tests.test_sf_chunk_loop_cpu import setup_of

FAMILIES = ("small", "mid", "large")
PARAMS = [(f, c) for f in FAMILIES for c in (0, 1)]


def total_for(uc, r):
    return (2 * len(lc.patterns(uc)) + 12) * uc * lc.CHUNK + r


@pytest.mark.parametrize("uc", (1, 3, 18))
@pytest.mark.parametrize("family,case", PARAMS)
def test_every_chunk_has_the_survivors_its_pattern_names(family, case, uc):
    m, model, fill, _, _ = setup_of(family, case)
    for r in (1, 4, 17):
        total = total_for(uc, r)
        text, offs, placed = lc.latch_batch(fill, case, total, uc)
        assert len(text) == total and int(offs[0]) == 0 and int(offs[-1]) == total and (offs[1:] >= offs[:-1]).all()
        counts = model.per_chunk(text)
        assert {c: int(counts[c]) for c in placed} == placed, (uc, r)
        assert int(counts.sum()) == sum(placed.values())          # ... and every other chunk has none
        hay, pos, _ = sf_oracle_records(m, case, text, offs)
        assert len(hay) == lc.expected_matches(placed, uc)
        assert (r >= 4) == (len(hay) > 0 and int(pos[-1]) + int(offs[hay[-1]]) == total)          # the match on the batch's last byte


def test_the_patterns_are_the_ones_the_straight_path_is_tested_with():
    names = [n for n, _ in lc.patterns(18)]
    for must in ("0,N,0 first", "0,N,0 last", "N,0,0,N first", "N,0,0,N last", "N,0,0,N epoch"):
        assert must in names
    for m in lc.LIMITS:
        assert "%d then 0" % m in names and "%d then 64" % m in names
    # a zero-survivor chunk follows and precedes a chunk with survivors, at a unit's first and last chunk and at chunks 15 | 16, where the ring is drained
    p = dict(lc.patterns(18))
    assert p["N,0,0,N epoch"] == {14: lc.N, 15: 0, 16: 0, 17: lc.N} and p["0,N,0 last"] == {15: 0, 16: lc.N, 17: 0}


def _setup(needles, case):
    from oracle import oracle
    from tests import sf_chunk_cases as cc
    from tests.helpers import ImgCheck
    from tests.test_sf_variants_cpu import cell_of
    m = oracle.Machine(list(needles) + [cc.RUN])
    img = ImgCheck().flatten(m, case)
    model = cc.FilterModel(img.tobytes(), case)
    return m, model, cc.filler_of(model, case), cell_of(img)


def test_the_pairs_set_has_a_large_suffix_table_behind_a_small_filter_under_ignore_case():
    """65 536 suffixes over eight pairs of bytes that differ in the ASCII case bit and are no letters: 4 096 filter keys under IgnoreCase -- <ILP 2, LW 0>, no
    child entries, no short needles; its texts have the survivors the patterns name"""
    from tests.test_sf_variants_cpu import launch_rule
    m, model, fill, cell = _setup(lc.ilp2_lw0_needles(), 1)
    assert cell["lw"] < 15 and cell["cap3"] > 15 and cell["tiers"] == 0 and cell["children"] == 0
    v = launch_rule(cell, 1, "emit", 64)
    assert (v["ilp"], v["lw"], v["short"], v["children"]) == (2, 0, False, False)
    text, offs, placed = lc.latch_batch(fill, 1, total_for(3, 17), 3)
    counts = model.per_chunk(text)
    assert {c: int(counts[c]) for c in placed} == placed and int(counts.sum()) == sum(placed.values())
    assert len(sf_oracle_records(m, 1, text, offs)[0]) == lc.expected_matches(placed, 3)


@pytest.mark.parametrize("case", (0, 1))
def test_the_bucket_0_word_and_its_text(case):
    word = lc.bucket0_word()
    m, model, fill, cell = _setup([word], case)
    assert cell["cap3"] == 2 and lc.t4_bucket_a(word, 2) == 0 and lc.t4_bucket_b(word, 2) == 0
    for straddle in (1, 2, 3):
        text, offs, want = lc.bucket0_batch(fill, word, 20 * 1024, straddle)
        counts = model.per_chunk(text)
        assert counts[5] == 1 and counts[9] == 1 and counts.sum() == 2
        assert model.passing(text)[5 * 1024]          # chunk 5's survivor is its offset 0
        hay, pos, _ = sf_oracle_records(m, case, text, offs)
        assert hay.tolist() == [0] and pos.tolist() == [5 * 1024 + 1] and want == 1
