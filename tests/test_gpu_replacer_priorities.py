"""The Replacer with the CALLER'S OWN priorities, through the C ABI (am_replacer_create / am_replacer_run / am_run_priority), and the one-kernel loop at its
capacity limits, crossed one step at a time.

include/am.h promises any distinct priorities <= 0; the host mirror (host/replacer.hpp) only ever builds priority = -index, which am_replacer_create recognises
(am_replacer.cpp:151-152) and runs on the payload-implicit instantiation of k_rp_lds.  Everything here that passes `priorities` runs the OTHER instantiation
(payload column in LDS, am_rplds.hip:46-54) and, with priorities below INT32_MIN, the value-list side path of single-valued states (am_replacer.cpp:166).
The reference is the oracle with the same priorities (tests/test_oracle_priorities.py pins it on the CPU); the limit inputs come from tests/helpers.py, where
the same CPU test file checks that each moves the one quantity it claims to move.

Left out: the 2-GiB text limit of k_rp_lds (am_rplds.hip:96, :260).  A Replacer run of that size belongs with the large-document tests
(tests/test_gpu_one_large_document.py) and would dominate this file's time."""
import random

import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers
from tests.helpers import INT32_MIN, AbiReplacer, mirror_twin, priority_families

pytestmark = pytest.mark.gpu

LOOP = "k_rp_lds + k_rp_loop"
ROUTES = (("pass by pass", {"AM_RP_LOOP": 0}), (LOOP, {"AM_RP_LOOP": 1}), ("k_rp_loop alone", {"AM_RP_LOOP": 1, "AM_RP_LDS": 0}), ("parallel fold", {"AM_RP_PARALLEL_FOLD": 1}))


def _lds():
    return int(am.libam().am_debug_rp_lds_haystacks())


def _switched(switches, f):
    for k, v in switches.items():
        am.debug_set(k, v)
    try:
        return f()
    finally:
        for k in switches:
            am.debug_set(k, -1)


def _every_route(case, pairs, prio, hays, max_len=-1, min_priority=None, expect=None):
    """One case on every route: the oracle's texts and Nothing entries byte for byte, the same number of passes everywhere, and on the forced one-kernel route
    k_rp_lds finished some haystack (every caller's list holds short ones), so the kernel under test provably ran.  Returns how many it finished."""
    r = AbiReplacer(case, pairs, prio, min_priority)
    assert r.rc == 0, r.error
    if expect is None:
        o = oracle.Replacer(case, pairs, priorities=prio, min_priority=min_priority)
        expect = [o.run(h, max_len) for h in hays]
    passes, lds = {}, 0
    for name, switches in ROUTES:
        got, passes[name] = _switched(switches, lambda: r.run(hays, max_len))
        assert got == expect, (name, case, pairs[:8], prio[:8] if prio else prio, max_len)
        if name == LOOP:
            lds = _lds()
            assert lds > 0, ("no haystack finished in k_rp_lds", case, pairs[:8], prio[:8] if prio else prio, max_len)
    reps = -(-64 // len(hays))
    got, passes["default, >= 64 documents"] = r.run(hays * reps, max_len)
    assert got == expect * reps, ("default", case, pairs[:8], prio[:8] if prio else prio, max_len)
    assert len(set(passes.values())) == 1, passes
    return lds


# Random pair sets can make ANY text that matches outgrow the LDS lists: with ("Xx", "QzxxzQ"), ("Y", "X"), ... under IgnoreCase the replacements feed each other, and
# a two-byte haystack took 11 passes and left k_rp_lds (measured: 0 of 2 short haystacks finished there, the batch went on to the other loops, same texts).  So both
# generators end their list with "#", which no needle matches: it goes through the kernel's first fold and finishes there, and _every_route's count is never
# zero because the kernel did not run.
def _rploop_style(rng):
    """the pair generator of tests/test_gpu_rploop.py (random pair sets, many passes), haystacks kept to what fits the LDS lists"""
    alpha = rng.choice(["abc ", "abİKß", "xyzXYZ", "abcde "])
    pairs = [("".join(rng.choice(alpha) for _ in range(rng.randint(1, 5))), "".join(rng.choice(alpha + "Q") for _ in range(rng.randint(0, 6)))) for _ in range(rng.randint(2, 60))]
    hays = ["".join(rng.choice(alpha) for _ in range(rng.choice((0, 1, 3, 50, 300, 800)))) for _ in range(rng.choice((3, 30)))]
    return pairs, hays + [alpha * 3, alpha[:2], "#"]


def _properties_style(rng):
    """the generator of test_replacer_properties (tests/test_gpu_parity.py)"""
    pairs = [("".join(rng.choice("abAB") for _ in range(rng.randint(1, 3))), "".join(rng.choice("abABxyİ") for _ in range(rng.randint(0, 4)))) for _ in range(rng.randint(1, 5))]
    hays = ["".join(rng.choice("abAB" * 10 + "İz") for _ in range(rng.randint(0, 40))) for _ in range(6)]
    return pairs, hays + ["#"]


def test_own_priorities_on_random_pair_sets():
    rng = random.Random(91)
    for it in range(14):
        pairs, hays = _rploop_style(rng) if it < 6 else _properties_style(rng)
        for case in (0, 1):
            for prio in priority_families(rng, len(pairs)).values():
                _every_route(case, pairs, prio, hays)
                _every_route(case, pairs, prio, hays, 1000 if it < 6 else 30)


def test_length_changing_lower_casings_and_length_limits():
    """makeMatch under IgnoreCase (Replacer.hs:268-274) where lower-casing changes the length (İ 2 -> 1 bytes, ẞ 3 -> 2, K 3 -> 1, Å 3 -> 2), and maxLength
    at, one below and one above the length a pass would produce (:240), with own priorities."""
    rng = random.Random(92)
    pairs = [("i", "<I>"), ("ß", "ss"), ("k", "K!"), ("å", "")]
    hays = ["İxİİ", "ẞßẞ", "KkK", "ÅåÅ" * 30, "İẞKÅ" * 100, "aİ" * 70]
    for prio in list(priority_families(rng, 4).values()) + [[-1, -2, -3, -4]]:
        assert _every_route(1, pairs, prio, hays) > 0
        assert _every_route(0, pairs, prio, hays) > 0
        _every_route(1, pairs, prio, hays, 400)
    pairs2 = [("straße", "STR"), ("i", "İİ"), ("k", ""), ("å", "K")]
    hays2 = ["Straße İstanbul KÅ" * 20, "strasse", "ẞ" * 50 + "straße"]
    for prio in priority_families(rng, 4).values():
        assert _every_route(1, pairs2, prio, hays2) > 0
    r = [("c", ""), ("a", "bbbb")]
    hays3 = ["aa", "a", "", "acac", "cccc", "aaaa" * 10]
    for prio in ([-1, 0], [-7, -3], [INT32_MIN - 1, -2]):
        for lim in (0, 1, 4, 7, 8, 9, 40, 160, 161):
            _every_route(0, r, prio, hays3, lim)
    for lim in (4, 5):
        _every_route(0, [("zz", "y"), ("aa", "bbb")], [-1, 0], ["aaa"], lim)


def test_priorities_that_differ_from_build_in_one_place_and_single_needles():
    """am_replacer.cpp:152 compares every payload with -index: a list that is -i except for its LAST payload turns the check false at the final element; one
    needle with priority 0 is build's replacer, with priority -7 it is not."""
    rng = random.Random(93)
    pairs = [("ab", "X"), ("Xc", "abab"), ("ba", ""), ("aX", "yy"), ("b", "ab")]
    hays = ["abcabcab" * 20, "ab", "bab", "", "cab" * 60] + ["".join(rng.choice("abcX") for _ in range(rng.randint(1, 200))) for _ in range(20)]
    n = len(pairs)
    assert _every_route(0, pairs, [-i for i in range(n - 1)] + [-(n - 1) - 1], hays) > 0
    assert _every_route(0, pairs, [-i for i in range(n - 1)] + [-2**40], hays) > 0
    assert _every_route(0, pairs, [-i for i in range(n)], hays) > 0                 # build's own priorities through the same helper (payload-implicit kernel)
    for p in (0, -7, INT32_MIN + 1, INT32_MIN, INT32_MIN - 1):
        assert _every_route(0, [("ab", "ba")], [p], hays) > 0
        assert _every_route(1, [("AB", "ba")], [p], hays) > 0
    # min_priority far below every priority: one more scan that finds nothing, the same texts (passes differ from the plain replacer's by that scan: all routes agree)
    _every_route(0, pairs, [-3 * i - 1 for i in range(n)], hays, min_priority=-1000)
    _every_route(0, pairs, [-3 * i - 1 for i in range(n)], hays, min_priority=-2**62)


def test_multi_valued_states_under_shuffled_priorities():
    """Duplicate needles and needles that are suffixes of others: one state's value list holds several payloads, in the automaton's order -- with shuffled
    priorities a HIGHER priority sits behind a lower one in the list (am_rp_fold.h:19-33, called at am_rplds.hip:156-167, :181-194 and am_rploop.hip:156, :163, :194, :208)."""
    pairs = [("abc", "1"), ("bc", "2b"), ("c", "3"), ("abc", "c4"), ("c", "5bc"), ("xbc", "ab6"), ("bc", "")]
    rng = random.Random(94)
    hays = ["abcxbcabc", "xbc" * 40, "c" * 100, "", "ab"] + ["".join(rng.choice("abcx") for _ in range(rng.randint(1, 300))) for _ in range(25)]
    n = len(pairs)
    orders = [list(range(n)), list(range(n))[::-1]] + [rng.sample(range(n), n) for _ in range(8)]
    for order in orders:
        for scale in (lambda i: -i, lambda i: -4 * i - 2, lambda i: helpers.WIDE_PRIORITIES[i] if i < 4 else -i):
            prio = [scale(i) for i in order]
            for case in (0, 1):
                assert _every_route(case, pairs, prio, hays) > 0
    _every_route(0, pairs, [-5, -1, -9, 0, -2, -7, -3], hays, 200)


def test_priorities_beyond_32_bits():
    """RpStateOne holds a 32-bit priority (am_replacer.cpp:166): a single-valued state whose priority does not fit takes the value-list side path in k_rp_lds,
    k_rp_loop and the pass-by-pass fold.  Mixed with small priorities, on single-valued and multi-valued states."""
    rng = random.Random(95)
    chain = [("a", "b"), ("b", "c"), ("c", "dd"), ("dd", "")]
    hays = ["abcabc" * 50, "", "dddd", "x", "abba" * 40] + ["".join(rng.choice("abcdx") for _ in range(rng.randint(1, 250))) for _ in range(20)]
    for prio in ([0, INT32_MIN, INT32_MIN - 1, -2**40], [-2**40, INT32_MIN - 1, INT32_MIN, 0], [INT32_MIN, -1, -2**62, INT32_MIN + 1],
                 [-2**62, -2**61, -2**40, INT32_MIN - 1], [-1, INT32_MIN - 1, -2, INT32_MIN - 2]):
        for case in (0, 1):
            assert _every_route(case, chain, prio, hays) > 0
            _every_route(case, chain, prio, hays, 320)
    multi = [("abc", "1"), ("bc", "2b"), ("c", "3"), ("abc", "c4"), ("c", "5bc")]
    hays2 = ["abcxbcabc", "c" * 100, ""] + ["".join(rng.choice("abcx") for _ in range(rng.randint(1, 300))) for _ in range(25)]
    for _ in range(6):
        prio = rng.sample([0, -1, -5, INT32_MIN + 1, INT32_MIN, INT32_MIN - 1, -2**40, -2**62], len(multi))
        for case in (0, 1):
            assert _every_route(case, multi, prio, hays2) > 0


def test_priority_int32_min_on_a_single_valued_state():
    """The smallest priority RpStateOne can hold.  k_rp_lds folds 32-bit priorities with INT32_MIN as its "nothing below the threshold" (am_rplds.hip:151-155), so
    a single-valued state must not carry INT32_MIN in that field: am_replacer_create gives it to the value-list side path like the priorities below it."""
    hays = ["abab", "b" * 30, "xaxbx" * 10]
    for prio, expect in (([0, INT32_MIN], [b"cccc", b"c" * 30, b"xcxcx" * 10]), ([INT32_MIN, 0], [b"bcbc", b"c" * 30, b"xbxcx" * 10])):
        assert _every_route(0, [("a", "b"), ("b", "c")], prio, hays, expect=expect) == len(hays)
        assert [oracle.Replacer(0, [("a", "b"), ("b", "c")], priorities=prio).run(h) for h in hays] == expect


def test_run_priority_with_own_priorities():
    """am_run_priority = prependMatch / makeMatch (Replacer.hs:252-274) for one pass with per-haystack thresholds, against a fold over the oracle's match list."""
    rng = random.Random(96)
    for it in range(12):
        case = it % 2
        alphabet = "abAB" if it < 8 else "aikİKß"
        pairs = [("".join(rng.choice(alphabet) for _ in range(rng.randint(1, 3))), "x" * rng.randint(0, 3)) for _ in range(rng.randint(1, 8))]
        hays = ["".join(rng.choice(alphabet * 3 + "z") for _ in range(rng.choice((0, 5, 60, 700)))) for _ in range(10)]
        for prio in priority_families(rng, len(pairs)).values():
            thresholds = [rng.choice([1, 0, -1, -3, -100, INT32_MIN, INT32_MIN - 1, -2**41] + prio) for _ in hays]
            r = AbiReplacer(case, pairs, prio)
            assert r.rc == 0, r.error
            best, got = r.run_priority(hays, thresholds)
            o = oracle.Machine([oracle.lower_utf8(n).decode() if case else n for n, _ in pairs])
            exp, exp_best = [], []
            for i, h in enumerate(hays):
                hb = h.encode("utf-8")
                pos, val = o.run_list(case, h)
                cands = [(int(p), int(v)) for p, v in zip(pos, val) if prio[int(v)] < thresholds[i]]
                b = max((prio[v] for _, v in cands), default=-2**63)
                exp_best.append(b)
                sel = []
                for p, v in cands:
                    if prio[v] == b:
                        st = oracle.skip_code_points_backwards(hb, p - 1, len(pairs[v][0]) - 1) if case else p - len(pairs[v][0].encode("utf-8"))
                        sel.append((i, st, p - st, v))
                exp += sorted(sel)
            assert best == exp_best, (case, pairs, prio, thresholds)
            assert got == exp, (case, pairs, prio)


def test_create_refuses_positive_and_repeated_priorities():
    pairs = [("a", "b"), ("b", "c"), ("c", "d")]
    for prio in ([0, 1, -1], [1, 0, -1], [0, -1, -1], [-5, -2, -5], [INT32_MIN - 1, 0, INT32_MIN - 1], [2**40, 0, -1]):
        r = AbiReplacer(0, pairs, prio, min_priority=min(prio))
        assert r.rc == am.api.AM_ERR_INVALID, (prio, r.rc)
    assert AbiReplacer(0, pairs, [0, -1, -2]).rc == 0 and AbiReplacer(0, pairs, [-1, -2**62, INT32_MIN]).rc == 0


# ---- C. the limits of the LDS loop, one step at a time ----------------------------------------------------------------------------------------

SWEEPS = helpers.all_sweeps()
NEIGHBOURS = helpers.ordinary_documents()


def _sweep_runners(sw):
    """(label, run(hays) -> (texts, passes)) for the mirror's replacer (payload-implicit kernel) and its twin with own priorities (payload column)."""
    mirror = am.Replacer(sw.case, sw.pairs)

    def run_mirror(hays):
        out = mirror.run_batch(hays)
        return out, mirror.last_stats()[0]
    twin_pairs, twin_prio = mirror_twin(sw.pairs)
    twin = AbiReplacer(sw.case, twin_pairs, twin_prio)
    assert twin.rc == 0, twin.error
    return (("payload implicit", run_mirror), ("payload column", twin.run))


@pytest.mark.parametrize("sw", SWEEPS, ids=[s.name + (" IC" if s.case else " CS") for s in SWEEPS])
def test_sweep_across_a_limit_of_the_lds_loop(sw):
    """One haystack per value from a few below to a few above the limit (tests/helpers.py quotes the limits with file and line).  Every text is the oracle's on the
    forced one-kernel route and on the pass-by-pass route, in both layouts of k_rp_lds; k_rp_lds finishes exactly the haystacks that fit -- eight copies of the
    lowest value all, of the highest none, the whole sweep the ones below the limit; and with 70 ordinary documents around them on the default route the
    neighbours' texts are right too (an overrun of one haystack's lists would land in LDS, not in its own result)."""
    orc = oracle.Replacer(sw.case, sw.pairs)
    exp = [orc.run(h) for h in sw.hays]
    exp_n = [orc.run(h) for h in NEIGHBOURS]
    mixed = NEIGHBOURS[:35] + sw.hays + NEIGHBOURS[35:]
    seen = {}
    for label, run in _sweep_runners(sw):
        ref, ref_passes = _switched({"AM_RP_LOOP": 0}, lambda: run(sw.hays))
        assert ref == exp, (sw, label, "pass by pass")

        def forced(hays):
            out = run(hays)
            return out[0], out[1], _lds()
        got, passes, n_all = _switched({"AM_RP_LOOP": 1}, lambda: forced(sw.hays))
        low, _, n_low = _switched({"AM_RP_LOOP": 1}, lambda: forced([sw.hays[0]] * 8))
        high, _, n_high = _switched({"AM_RP_LOOP": 1}, lambda: forced([sw.hays[-1]] * 8))
        assert got == exp, (sw, label, "one kernel")
        assert passes == ref_passes
        assert low == [exp[0]] * 8 and high == [exp[-1]] * 8
        got, _ = run(mixed)                                               # the default route: >= 64 documents
        n_mixed = _lds()
        assert got == exp_n[:35] + exp + exp_n[35:], (sw, label, "default route, with neighbours")
        seen[label] = (n_low, n_high, n_all, n_mixed)
        print("%s, %s: k_rp_lds finished %d of 8 lowest, %d of 8 highest, %d of %d in the sweep (%d fit), %d of %d with neighbours" %
              (sw, label, n_low, n_high, n_all, len(sw.hays), sum(sw.fits), n_mixed, len(mixed)))
    for label, (n_low, n_high, n_all, n_mixed) in seen.items():
        assert n_low == 8 and n_high == 0, (sw, label, seen)
        assert 0 < n_all < len(sw.hays), (sw, label, seen)
        assert n_all == sum(sw.fits), (sw, label, seen, "the limit is not where csrc/am_rplds.hip puts it")
        assert n_mixed == len(NEIGHBOURS) + sum(sw.fits), (sw, label, seen, "a neighbour was pushed out of LDS, or a haystack beyond the limit stayed")
    assert seen["payload implicit"] == seen["payload column"], seen


def _default_route_took_the_loop(run, hays):
    """Runs an unforced batch and says whether the one-kernel route took it: the counter is first cleared by a forced run without k_rp_lds, and a batch that the
    host refuses (am_replacer.cpp:887, :952) leaves it alone."""
    _switched({"AM_RP_LOOP": 1, "AM_RP_LDS": 0}, lambda: AbiReplacer(0, [("a", "b")], [-1]).run(["xax"]))      # (a replacer of its own: the one under test may be refused even when forced)
    assert _lds() == 0
    out = run(hays)
    return out[0], _lds() > 0


def test_the_hosts_route_limits():
    """am_replacer.cpp:886-887: the one-kernel route takes a replacer while round_up_64(2 ov + longest replacement + 16) <= 4096, forced or not; :952: an unforced
    batch goes pass by pass when some document has more than 4096 match positions.  Same texts on either side of both."""
    for rl, cap in helpers.ROUTE_REPL_LENGTHS:
        pairs = helpers.route_window_pairs(rl)
        hays = NEIGHBOURS + ["x" * 50 + "m" + "x" * 50, "m", "mm"]
        orc = oracle.Replacer(0, pairs)
        exp = [orc.run(h) for h in hays]
        twin_pairs, twin_prio = mirror_twin(pairs)
        twin = AbiReplacer(0, twin_pairs, twin_prio)
        mirror = am.Replacer(0, pairs)
        for run in (twin.run, lambda hs: (mirror.run_batch(hs), 0)):
            got, took = _default_route_took_the_loop(run, hays)
            assert got == exp, (rl, cap)
            assert took == (cap <= 4096), (rl, cap)
            assert _switched({"AM_RP_LOOP": 0}, lambda: run(hays))[0] == exp
            assert _switched({"AM_RP_LOOP": 1}, lambda: run(hays))[0] == exp
    pairs = helpers.ROUTE_MATCH_PAIRS
    orc = oracle.Replacer(0, pairs)
    twin_pairs, twin_prio = mirror_twin(pairs)
    twin = AbiReplacer(0, twin_pairs, twin_prio)
    mirror = am.Replacer(0, pairs)
    for n in helpers.ROUTE_MATCH_COUNTS:
        hays = NEIGHBOURS[:40] + [helpers.route_match_document(n)] + NEIGHBOURS[40:]
        exp = [orc.run(h) for h in hays]
        for run in (twin.run, lambda hs: (mirror.run_batch(hs), 0)):
            got, took = _default_route_took_the_loop(run, hays)
            assert got == exp, n
            assert took == (n <= 4096), n
            assert _switched({"AM_RP_LOOP": 1}, lambda: run(hays))[0] == exp
