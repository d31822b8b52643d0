"""The reference for a Replacer with the caller's OWN priorities (oracle.Replacer(case, pairs, priorities, min_priority)), pinned on the CPU, and the proof that
the inputs of the limit sweeps (tests/helpers.py, run on the GPU by tests/test_gpu_replacer_priorities.py) are what they claim to be.

runWithLimit (Replacer.hs:203-274) never does arithmetic on a priority: it compares (pMatch < threshold, > pBest, == pBest :255-258; go p :242;
p == minPriority :241).  So a replacer with own priorities IS the plain replacer over the pair list sorted by descending priority: two routes to the same
answer inside the reference.  INT64_MIN is kept out of every priority list: it is the fold's seed (minBound, :222), a match that carried it would never
be "better than nothing"."""
import random

import pytest

from oracle import oracle
from tests import helpers
from tests.helpers import INT32_MIN, priority_families, sorted_by_priority


def _random_case(rng):
    alpha = rng.choice(["abAB", "abc ", "aikİKßẞÅå", "xyzXYZ"])
    pairs = [("".join(rng.choice(alpha) for _ in range(rng.randint(1, 4))), "".join(rng.choice(alpha + "Q") for _ in range(rng.randint(0, 5)))) for _ in range(rng.randint(1, 12))]
    hays = ["".join(rng.choice(alpha) for _ in range(rng.choice((0, 1, 7, 60, 400)))) for _ in range(6)]
    return pairs, hays


def test_order_is_all_that_counts():
    rng = random.Random(71)
    seen = set()
    for it in range(40):
        pairs, hays = _random_case(rng)
        if it % 5 == 0:
            pairs += [pairs[0], (pairs[-1][0], "dup")]              # duplicate needles: one state, several payloads
        for case in (0, 1):
            for fam, prio in priority_families(rng, len(pairs)).items():
                own = oracle.Replacer(case, pairs, priorities=prio)
                plain = oracle.Replacer(case, sorted_by_priority(pairs, prio))
                for h in hays:
                    for max_len in (-1, len(h.encode()), len(h.encode()) + 3, 40):
                        assert own.run(h, max_len) == plain.run(h, max_len), (case, fam, pairs, prio, h, max_len)
                seen |= set(prio)
    assert {INT32_MIN, INT32_MIN - 1, -2**40, -2**62} <= seen and -2**63 not in seen


def test_build_priorities_spelled_out_change_nothing():
    rng = random.Random(72)
    for _ in range(20):
        pairs, hays = _random_case(rng)
        n = len(pairs)
        for case in (0, 1):
            a, b = oracle.Replacer(case, pairs), oracle.Replacer(case, pairs, priorities=[-i for i in range(n)], min_priority=1 - n)
            assert [a.run(h) for h in hays] == [b.run(h) for h in hays]


def test_min_priority_at_or_below_the_smallest_priority_is_only_an_early_exit():
    """Replacer.hs:241: `if p == minPriority then newHaystack else go p newHaystack` -- with minPriority BELOW every priority the loop runs one more scan, finds
    nothing below the threshold (:228-230) and returns the same text.  A min_priority ABOVE the smallest priority cuts the lower priorities off: the caller's
    error (include/am.h), not tested."""
    rng = random.Random(73)
    for _ in range(25):
        pairs, hays = _random_case(rng)
        for case in (0, 1):
            for prio in priority_families(rng, len(pairs)).values():
                exp = [oracle.Replacer(case, pairs, priorities=prio).run(h) for h in hays]
                for mp in (min(prio), min(prio) - 1, min(prio) - 2**20, -2**63 + 1):
                    o = oracle.Replacer(case, pairs, priorities=prio, min_priority=mp)
                    assert [o.run(h) for h in hays] == exp, (case, pairs, prio, mp)


def test_mirror_twin_is_the_same_replacer():
    rng = random.Random(74)
    for _ in range(20):
        pairs, hays = _random_case(rng)
        twin, prio = helpers.mirror_twin(pairs)
        assert sorted_by_priority(twin, prio) == pairs
        for case in (0, 1):
            a, b = oracle.Replacer(case, pairs), oracle.Replacer(case, twin, priorities=prio)
            assert [a.run(h, 300) for h in hays] == [b.run(h, 300) for h in hays]


SWEEPS = helpers.all_sweeps()


@pytest.mark.parametrize("sw", SWEEPS, ids=[s.name + (" IC" if s.case else " CS") for s in SWEEPS])
def test_the_limit_inputs_are_what_they_claim_to_be(sw):
    """Every haystack of a sweep moves ONE quantity across its limit, one step at a time, and keeps the others away from theirs -- computed with the oracle's
    automaton and plain Python, before any kernel sees the input."""
    far = {"first_scan": helpers.LDS_REC - 32, "records_after": helpers.LDS_REC - 4, "pieces": helpers.LDS_PC - 32, "window": helpers.LDS_WIN - 32, "new_records": helpers.LDS_NEW - 32}
    assert sw.pairs[-1] == helpers.NEVER and len(sw.hays) == len(sw.values) == len(sw.fits)
    assert sw.fits[0] and not sw.fits[-1] and sw.fits == sorted(sw.fits, reverse=True), "the sweep straddles its limit"
    assert sum(sw.fits) >= 3 and len(sw.fits) - sum(sw.fits) >= 3
    assert [v for v, f in zip(sw.values, sw.fits) if f][-1] in (sw.limit, sw.limit - 1), "the documented limit is where the sweep turns"      # (- 1: the piece counts of one parity)
    orc = oracle.Replacer(sw.case, sw.pairs)
    for i, h in enumerate(sw.hays):
        q = helpers.sweep_quantities(sw, i)
        assert q[sw.quantity] == sw.values[i], (sw, i, q)
        assert "zz" not in orc.run(h).decode().lower()                   # the lowest priority never matches, in any pass
        for key, bound in far.items():
            if key == sw.quantity or (sw.quantity == "records_after" and key == "first_scan"):
                continue
            if sw.name == "staged records" and key in ("first_scan", "records_after"):
                assert q["first_scan"] == 490                            # (this sweep is ABOUT a nearly full list)
                continue
            if sw.name == "list growth" and key == "new_records":
                assert q[key] == 25
                continue
            assert q[key] <= bound, (sw, i, key, q)
    if sw.name.startswith("new records"):
        # where the new match positions lie in the window's trips of 64 positions (am_rplds.hip:381: from the replacement's first byte)
        for i, m in enumerate(sw.values):
            rep = sw.pairs[i][1].lower()
            first_trip = rep[:64].count("q")
            assert rep.count("q") == m and first_trip == (min(m, 64) if "one" in sw.name else 40)


def test_the_route_limit_inputs():
    """am_replacer.cpp:886-887: round_up_64(2 ov + longest replacement + 16) <= 4096; :952: no document with more than 4096 match positions."""
    for rl, cap in helpers.ROUTE_REPL_LENGTHS:
        pairs = helpers.route_window_pairs(rl)
        ov = helpers.reach(0, pairs)
        assert (2 * ov + rl + 16 + 63) // 64 * 64 == cap and max(len(r) for _, r in pairs) == rl
    assert [c for _, c in helpers.ROUTE_REPL_LENGTHS] == [4096, 4096, 4160]
    m = oracle.Machine([n for n, _ in helpers.ROUTE_MATCH_PAIRS])
    for n in helpers.ROUTE_MATCH_COUNTS:
        pos, _ = m.run_list(0, helpers.route_match_document(n))
        assert len(set(int(p) for p in pos)) == n
    assert helpers.ROUTE_MATCH_COUNTS == (4095, 4096, 4097)
