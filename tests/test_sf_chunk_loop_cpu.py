"""The texts of tests/sf_chunk_cases.py are what they claim, on the CPU: the host model of k_sf's filter stage counts exactly the candidates every builder promises
(and none anywhere else in the batch), and the oracle finds on them the records the GPU tests then expect -- a match per candidate of a run, the single planted
needle at its exact end, nothing for a needle that lies across a haystack's start."""
import numpy as np
import pytest

from oracle import oracle
from tests import sf_chunk_cases as cc
from tests.helpers import ImgCheck, sf_oracle_records
from tests.test_sf_variants_cpu import PURPOSE, cell_of, launch_rule

_SETUPS = {}


def setup_of(family, case):
    """(machine, model, filler byte, long needle) of a family's needles plus the run's, per case mode"""
    if (family, case) not in _SETUPS:
        m = oracle.Machine(cc.needles_of(family))
        img = ImgCheck().flatten(m, case)
        model = cc.FilterModel(img.tobytes(), case)
        fill = cc.filler_of(model, case)
        _SETUPS[(family, case)] = (m, model, fill, cc.long_needle_of(cc.needles_of(family), m, case, fill), cell_of(img))
    return _SETUPS[(family, case)]


PARAMS = [(f, c) for f in cc.FAMILIES for c in (0, 1)]


@pytest.mark.parametrize("family,case", PARAMS)
def test_the_run_needle_leaves_the_family_in_its_cell(family, case):
    cell = setup_of(family, case)[4]
    v = launch_rule(cell, case, "emit", 256)
    assert (v["ilp"], v["lw"], v["short"], v["children"]) == PURPOSE[family]


@pytest.mark.parametrize("family,case", PARAMS)
def test_queue_limit_chunks_hold_exactly_n_candidates(family, case):
    m, model, fill, _, _ = setup_of(family, case)
    for n in cc.QUEUE_NS + ("every",):
        text, offs, want = cc.queue_batch(fill, case, n, 1)
        assert want == (cc.CHUNK if n == "every" else n)
        assert model.per_chunk(text).tolist() == [0, want, 0]
        hay, pos, _ = sf_oracle_records(m, case, text, offs)
        assert len(hay) == want and (hay == 0).all()              # every candidate of a run is a match of the run's needle
        if want:
            first = cc.CHUNK + (0 if n == "every" else 8 + 3)
            assert pos.tolist() == list(range(first + 1, first + 1 + want))
    # as the first and as the last chunk of units of five chunks, a haystack per unit: the run that fills a unit's first chunk loses its first three matches
    uc, total = 5, 5 * cc.CHUNK * (3 * 12 + 8) + 19
    text, offs, placed = cc.unit_batch(fill, case, total, uc)
    counts = model.per_chunk(text)
    assert {c: int(counts[c]) for c, _ in placed} == dict(placed) and counts.sum() == sum(n for _, n in placed)
    hay, pos, _ = sf_oracle_records(m, case, text, offs)
    assert len(hay) == sum(n for _, n in placed) - 3


@pytest.mark.parametrize("family,case", PARAMS)
def test_single_matches_batch_ends_and_haystack_starts(family, case):
    m, model, fill, long_needle, _ = setup_of(family, case)
    for lane in cc.BIT_LANES:
        for k in range(16):
            at = cc.CHUNK + 16 * lane + k
            text, offs = cc.single_match_batch(fill, long_needle, at, 3 * cc.CHUNK)
            hay, pos, _ = sf_oracle_records(m, case, text, offs)
            assert hay.tolist() == [0] and pos.tolist() == [at + 1]
            assert model.passing(text)[at]
    for total in [1024 * mm + r for mm in (0, 1, 16) for r in range(1, 18)]:
        needle = long_needle if total >= len(long_needle) else cc.run(4, case) if total >= 4 else None
        text, offs = cc.end_batch(fill, needle, total)
        hay, pos, _ = sf_oracle_records(m, case, text, offs)
        assert len(text) == total and len(hay) == (needle is not None)
        if needle is not None:
            assert int(pos[0]) + int(offs[hay[0]]) == total and model.passing(text)[total - 1]
    # chunk 1 inside one haystack that starts 0..5 bytes before it, the batch's only candidate in chunk 1 (the filter sees bytes, not haystacks: the window is a
    # candidate whether or not it fits into the haystack)
    for into in cc.HAY_INTO:
        for what in (0, 1, 2, 3, "across"):
            text, offs, want, last = cc.single_chunk_start_batch(fill, case, long_needle, into, what, 3 * cc.CHUNK)
            counts = model.per_chunk(text)
            assert last // cc.CHUNK == 1 and offs[1] == cc.CHUNK - into and model.passing(text)[last] and counts[1] > 0 and counts[2] == 0
            if what != "across":
                assert counts.tolist() == [0, 1, 0] and want == (what + into >= 3)
            hay, pos, _ = sf_oracle_records(m, case, text, offs)
            assert len(hay) == want
            if want:
                assert hay.tolist() == [1] and pos.tolist() == [what + 1 + into]
    # the start inside the chunk of the run's candidate
    for hs0 in [cc.CHUNK - 4, cc.CHUNK - 5, cc.CHUNK + 100, 2 * cc.CHUNK - 4]:
        for what in (3, 4, "across"):
            text, offs, want = cc.hay_start_batch(fill, case, long_needle, hs0, what, 3 * cc.CHUNK)
            last = hs0 + what - 1 if what != "across" else hs0 - len(long_needle) // 2 + len(long_needle) - 1
            assert model.passing(text)[last] and last // cc.CHUNK - hs0 // cc.CHUNK in ((0,) if what != "across" else (0, 1))
            assert what == "across" or model.per_chunk(text).sum() == 1
            hay, pos, _ = sf_oracle_records(m, case, text, offs)
            assert len(hay) == want
            if want:
                assert hay.tolist() == [1] and pos.tolist() == [4]
