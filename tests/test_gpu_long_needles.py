"""Needles of 17 bytes to 66 000 on every scan route and every Replacer route, against the oracle: exact equality of (haystack, end position, value) triples in
fold order, of counts, flags and replaced texts.  No needle of the other files is longer than 240 bytes; what depends on the longest needle -- k_sf's trie walk
and its walker queue, the warm-up of k_dfa and k_ac, the overlap of am_run_range and of am_run's segments, the Replacer's reach and its route limit -- meets here
needles longer than a 1-KiB chunk, than the light configuration's 16 chunks and than a 64-chunk work unit.  The inputs come from tests/helpers.py (long_needle_sets,
long_needle_text, long_needle_unit_text, long_needle_replacer_cases); tests/test_long_needles_cpu.py holds them, and the image's host interpreter on them, to the
oracle on the CPU, so a failure here is a kernel's.  Needs an MI355X."""
import ctypes as C
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers
from tests.helpers import (AbiReplacer, long_near_miss, long_needle_plan, long_needle_replacer_cases, long_needle_sets, long_needle_unit_text, long_text_parts,
                           mirror_twin, sf_expand, sf_oracle_records)
from tests.test_gpu_replacer_priorities import _default_route_took_the_loop, _lds, _switched

pytestmark = pytest.mark.gpu

SETS = long_needle_sets()
SET_CASES = [(name, case) for name in SETS for case in (0, 1)]
IDS = ["%s-%s" % (name, "IC" if case else "CS") for name, case in SET_CASES]
# route -> (am_automaton_set_kernel, switches set BEFORE the automaton is built: the flattener reads AM_DFA and AM_DFA_CHUNK)
ROUTES = {
    "k_sf": (0, {"AM_DFA": 0}),                                    # the default route: no batch here reaches the table walk's 32 MiB
    "k_sf traced": (0, {"AM_DFA": 0, "AM_SF_TRACE": 1}),           # the DBG instantiations: the same walk, no walker queue limit of their own
    "k_ac": (1, {"AM_DFA": 0}),                                    # warm-up 4 * max_needle_cps + 4, ac_chunk grows with it
    "k_dfa": (3, {"AM_DFA": 1}),                                   # the flattener's own dfa_chunk: count -> scan -> emit beyond 8 192-byte units
    # a forced unit: the flattener doubles it until it holds four warm-ups (am_flatten.cpp:907; tests/test_long_needles_cpu.py dfa_chunk_rule pins what comes out),
    # so under these needles 64 and 2 048 end as 4 096 to 524 288 bytes; what a forced unit changes is that am_run.cpp:54-61 no longer shrinks it for a small batch
    "k_dfa 64": (3, {"AM_DFA": 1, "AM_DFA_CHUNK": 64}),
    "k_dfa 2048": (3, {"AM_DFA": 1, "AM_DFA_CHUNK": 2048}),
}

_MACHINES, _RECORDS = {}, {}


def machine(name):
    if name not in _MACHINES:
        _MACHINES[name] = oracle.Machine(SETS[name])
    return _MACHINES[name]


def records(name, case, part):
    """The oracle over one batch, computed once and shared by the routes."""
    key = (name, case, part)
    if key not in _RECORDS:
        t = long_needle_plan(name, case, 0, part)
        _RECORDS[key] = sf_oracle_records(machine(name), case, t.text, t.offs)
    return _RECORDS[key]


@pytest.fixture(scope="module", autouse=True)
def _release_at_the_end():
    yield
    _MACHINES.clear()
    _RECORDS.clear()
    am.api.libam().am_release_device_memory()
    am.api.libam().am_release_host_memory()


def contains_any(a, case, hays):
    s = am.api._Slices(hays)
    out = np.zeros(max(s.n, 1), np.uint8)
    am.api.check(am.api.libam().am_contains_any(a.device, case, s.arr, s.n, out.ctypes.data))
    return out[:s.n].astype(bool)


def ascending(rs):
    """keys == sorted(set(keys)): one record per position, in (haystack, end_pos) order."""
    k = (rs["haystack"].astype(np.uint64) << np.uint64(40)) | rs["end_pos"].astype(np.uint64)
    return bool((k[1:] > k[:-1]).all())


def same_triples(rs, exp, vo, vals):
    got = sf_expand(rs["haystack"], rs["state"], rs["end_pos"], vo, vals)
    return all(np.array_equal(g, e) for g, e in zip(got, exp))


def built(needles, route):
    kernel, switches = ROUTES[route]
    for k, v in switches.items():
        am.debug_set(k, v)
    a = am.Automaton(needles)
    if kernel:
        a.set_kernel(kernel)
    return a


def sf_variants_of(call, modes, total=1 << 20):
    """call(), then the k_sf instantiation it launched last: for a batch beyond 16 KiB one of the full-size ones, in the mode asked for."""
    am.api.sf_last_variant()
    out = call()
    v = am.api.sf_last_variant()
    assert v is not None and v["light"] == (total <= 16 * 1024) and v["mode"] in modes, v
    return out, v


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name,case", SET_CASES, ids=IDS)
def test_records_counts_and_flags_equal_the_oracle(name, case, route):
    """Every batch of the set on one route: am_run's records expanded to the oracle's triples, one record per position in order; am_count; am_contains_any (in
    k_sf the walk to the end inline, no walker queue).  On k_sf, emit and count ran a full-size instantiation, traced or not as asked."""
    a = built(SETS[name], route)
    m = machine(name)
    vo, vals = m.values_off(), m.values()
    for part in range(long_text_parts(name)):
        t = long_needle_plan(name, case, 0, part)
        hays, exp = t.hays(), records(name, case, part)
        assert len(t.text) > 16 * 1024 and len(exp[0]) > 100
        want_counts = np.bincount(exp[0], minlength=len(hays))
        if route.startswith("k_sf"):
            rs, v = sf_variants_of(lambda: a.run_records(case, hays), ("emit",))
            assert v["dbg"] == (route == "k_sf traced") and v["ic"] == bool(case)
            counts, vc = sf_variants_of(lambda: a.count_matches(case, hays), ("count",))
            assert vc["dbg"] == (route == "k_sf traced")
            flags, va = sf_variants_of(lambda: contains_any(a, case, hays), ("any",))
            print("k_sf instantiations:", *("%s <ILP %d, LW %d%s%s%s>" % (x["mode"], x["ilp"], x["lw"], ", SHORT" * x["short"], ", DBG" * x["dbg"], ", CHILDREN" * x["children"])
                                            for x in (v, vc, va)))
        else:
            am.api.sf_last_variant()          # (reading clears)
            rs, counts, flags = a.run_records(case, hays), a.count_matches(case, hays), contains_any(a, case, hays)
            assert am.api.sf_last_variant() is None, "k_sf ran on another kernel's route"
        print("%s %s part %d on %s: %d records, %d matches" % (name, "IC" if case else "CS", part, route, len(rs), len(exp[0])))
        assert same_triples(rs, exp, vo, vals), (name, case, part, route, len(rs))
        assert ascending(rs)
        assert np.array_equal(counts, want_counts), (name, case, part, route)
        assert np.array_equal(flags, want_counts > 0) and flags.any() and not flags.all()


def _upper(rng, text):
    partners = helpers._sf_upper_partners()
    return "".join(rng.choice(partners[c]) if c in partners and rng.random() < 0.35 else c for c in text)


@pytest.mark.parametrize("name,case", SET_CASES, ids=IDS)
def test_contains_all(name, case):
    """Searcher.containsAll sets the needle ids inside k_sf (mode ids: the inline walk, whole value lists).  Every needle; the same with the first code point of
    the longest needle changed; every second needle; nothing.  Under IgnoreCase the text is written with upper-case partners."""
    am.debug_set("AM_DFA", 0)
    needles = SETS[name]
    rng = random.Random("long-all-" + name)
    longest = max(range(len(needles)), key=lambda i: len(needles[i]))
    spoiled = list(needles)
    spoiled[longest] = long_near_miss(needles[longest], "first")
    hays = [" ".join(needles), " ".join(spoiled), " ".join(needles[::2]), ""]
    if case:
        hays = [_upper(rng, h) for h in hays]
    hays = [h.encode("utf-8") for h in hays]
    o, s = machine(name), am.Searcher(case, needles)
    want = [o.contains_all(case, h) for h in hays]
    assert want[0] and not want[1] and not want[3]
    flags, v = sf_variants_of(lambda: s.contains_all_batch(hays), ("ids",), sum(len(h) for h in hays))
    assert flags.tolist() == want


@pytest.mark.parametrize("route", ("k_sf", "k_dfa"))
@pytest.mark.parametrize("case", (0, 1))
def test_needles_across_unit_boundaries(case, route):
    """A batch large enough for work units of two chunks and more (6 MiB, or what am_debug_sf_unit_chunks asks for on this device): the 1 025-, 8 193- and
    16 500-byte needles end 1 byte, 5 bytes, half their length and all but one byte behind a unit boundary, so the walk reads back across one unit, eight and
    sixteen chunks; haystack borders inside and between units."""
    total = 6 << 20
    while am.api.sf_unit_chunks(total) < 2:
        total += 2 << 20
        assert total <= (64 << 20)
    uc = am.api.sf_unit_chunks(total)
    needles, text, offs = long_needle_unit_text(total, uc * 1024)
    hays = [text[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    o = oracle.Machine(needles)
    exp = sf_oracle_records(o, case, text, offs)
    assert {len(needles[v]) for v in set(exp[2].tolist())} >= {1025, 8193, 16500} and len(exp[0]) > 100
    a = built(needles, route)
    if route == "k_sf":
        rs, _ = sf_variants_of(lambda: a.run_records(case, hays), ("emit",))
        counts, _ = sf_variants_of(lambda: a.count_matches(case, hays), ("count",))
    else:
        rs, counts = a.run_records(case, hays), a.count_matches(case, hays)
    print("%d bytes, %d chunks per unit, %s: %d records, %d matches" % (total, uc, route, len(rs), len(exp[0])))
    assert same_triples(rs, exp, o.values_off(), o.values()) and ascending(rs)
    assert np.array_equal(counts, np.bincount(exp[0], minlength=len(hays)))


def _range_document():
    """One haystack that holds the 8 193- and the 16 500-byte needle of beyond/ak𝄞яß (4-byte code points) between filler, near misses and 70-byte heads:
    (needles, text bytes, [end of each whole needle])."""
    ns = SETS["beyond/" + helpers.LONG_ALPHABETS[3]][:4]      # (without the 66 000-byte needle: its overlap would be the whole document for every range)
    rng = random.Random("long-range")
    fill = lambda n: "".join(rng.choice(helpers.LONG_FILLER + "𝄞я") for _ in range(n))
    parts = [fill(3000), ns[2], fill(700), long_near_miss(ns[2], 56), ns[3], fill(1500), ns[0], fill(5), ns[0][1:], fill(2000), ns[1], fill(900)]
    ends, at = [], 0
    for p in parts:
        at += len(p.encode("utf-8"))
        if p in (ns[2], ns[0]):
            ends.append(at)
    return ns, "".join(parts).encode("utf-8"), ends


@pytest.mark.parametrize("case", (0, 1))
def test_ranges_shorter_than_a_needle_add_up_to_the_whole_scan(case):
    """am_run_range / am_count_range (range_window: overlap 4 * max_needle_cps): 2, 3, 7 and 40 ranges that partition the document -- most of the 40 are shorter
    than the needles --, with borders one byte before, at and one byte after the end of the 8 193- and of the 16 500-byte needle and inside a 4-byte code point:
    concatenated they are the whole scan's records, which are the oracle's; the counts add up."""
    lib = am.libam()
    ns, text, ends = _range_document()
    n = len(text)
    inside = next(i for i in range(n // 3, n) if text[i] == 0xF0) + 2          # the third byte of a 𝄞
    o = oracle.Machine(ns)
    a = built(ns, "k_sf")
    whole = a.run_records(case, [text])
    exp = sf_oracle_records(o, case, text, np.asarray([0, n]))
    assert same_triples(whole, exp, o.values_off(), o.values())
    assert {0, 2} <= set(exp[2].tolist())                                     # both long needles are found whole
    total = int(a.count_matches(case, [text])[0])
    vlen = np.diff(a.values_off()).astype(np.int64)
    buf = C.create_string_buffer(text, n + 1)
    sl = am.api.Slice(C.addressof(buf), 0, n)
    rng = random.Random(11)
    borders = [e + d for e in ends for d in (-1, 0, 1)] + [inside]
    for world, pick in ((2, [ends[1]]), (3, [ends[0] - 1, inside]), (7, borders[:3] + borders[4:6] + [inside]), (40, borders)):
        cuts = set([0, n] + pick)
        while len(cuts) < world + 1:
            cuts.add(rng.randint(1, n - 1))
        cuts = sorted(cuts)
        parts, counts = [], 0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            m = C.c_void_p()
            am.check(lib.am_run_range(a.device, case, C.byref(sl), lo, hi, C.byref(m)))
            parts.append(am.api.matches_to_numpy(m))
            lib.am_matches_free(m)
            c = C.c_uint64(0)
            am.check(lib.am_count_range(a.device, case, C.byref(sl), lo, hi, C.byref(c)))
            counts += int(c.value)
            assert int(c.value) == int(vlen[parts[-1]["state"].astype(np.int64)].sum()), (lo, hi)
            assert all(lo < int(e) <= hi for e in parts[-1]["end_pos"])
        assert np.concatenate(parts).tobytes() == whole.tobytes(), (world, cuts)
        assert counts == total
        if world == 40:
            assert min(hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])) == 1 and sorted(hi - lo for lo, hi in zip(cuts[:-1], cuts[1:]))[20] < 8193


@pytest.mark.parametrize("segment_kib", (64, 300))
def test_am_run_in_segments_equals_the_call_in_one_piece(segment_kib):
    """AM_RUN_SEGMENTS: the range document (larger than a 64-KiB segment's share, smaller than 300 KiB) between the haystacks of the beyond set's batch, in segments
    of whole haystacks, against the call in one piece and the oracle."""
    _, doc, _ = _range_document()
    name = "beyond/" + helpers.LONG_ALPHABETS[3]
    ns = SETS[name]
    t = long_needle_plan(name, 1)
    hays = t.hays()[:30] + [doc] + t.hays()[30:60] + [doc, b""]
    a = built(ns, "k_sf")
    o = machine(name)
    one = a.run_records(1, hays)
    am.debug_set("AM_RUN_SEGMENTS", segment_kib)
    cut = a.run_records(1, hays)
    am.debug_set("AM_RUN_SEGMENTS", -1)
    assert len(one) > 40 and one.tobytes() == cut.tobytes()
    text = b"".join(hays)
    offs = np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.int64)
    assert same_triples(cut, sf_oracle_records(o, 1, text, offs), o.values_off(), o.values())


# ---- the Replacer ----------------------------------------------------------------------------------------------------------------------------

RP_CASES = long_needle_replacer_cases()
NEIGHBOURS = helpers.ordinary_documents()
RP_ROUTES = (("pass by pass", {"AM_RP_LOOP": 0}), ("full scans", {"AM_RP_FULL_SCANS": 1}), ("pieces", {"AM_RP_LOOP": 0, "AM_RP_PIECES": 1}),
             ("parallel fold", {"AM_RP_PARALLEL_FOLD": 1}), ("one kernel", {"AM_RP_LOOP": 1}), ("k_rp_loop alone", {"AM_RP_LOOP": 1, "AM_RP_LDS": 0}))


def _runners(c):
    """(label, run(hays) -> (texts, passes)) for the mirror's replacer (payload-implicit kernel) and its twin with own priorities (payload column)."""
    mirror = am.Replacer(c.case, c.pairs)

    def run_mirror(hays):
        out = mirror.run_batch(hays)
        return out, mirror.last_stats()[0]
    twin_pairs, twin_prio = mirror_twin(c.pairs)
    twin = AbiReplacer(c.case, twin_pairs, twin_prio)
    assert twin.rc == 0, twin.error
    return (("payload implicit", run_mirror), ("payload column", twin.run))


@pytest.mark.parametrize("c", RP_CASES, ids=[c.name for c in RP_CASES])
def test_a_replacement_completes_a_long_needle(c):
    """Pass 1 makes N appear, |L| bytes on one side of the replacement and |R| on the other: a re-scan whose reach is too short loses it.  Every route gives the
    listed texts ("!" where N formed) after the pinned number of passes; with 70 ordinary documents around, the default route is the one-kernel loop exactly while
    round_up_64(2 ov + 1 + 16) <= 4096 (am_replacer.cpp:837-838), and k_rp_lds finishes the neighbours and the documents whose window fits its 448 bytes, no other."""
    exp_n = [oracle.Replacer(c.case, c.pairs).run(h) for h in NEIGHBOURS]
    mixed = NEIGHBOURS[:35] + c.docs + NEIGHBOURS[35:]
    for label, run in _runners(c):
        for route, switches in RP_ROUTES:
            if route == "pieces" and c.case:
                continue
            got, passes = _switched(switches, lambda: run(c.docs))
            assert got == c.expect, (c, label, route)
            assert passes == c.passes, (c, label, route, passes)
        got, took = _default_route_took_the_loop(run, mixed)
        n_lds = _lds()
        passes = run(mixed)[1]
        print("%s, %s: ov %d, cap %d, default route %s, k_rp_lds finished %d of %d (%d documents fit)" %
              (c, label, c.ov, c.cap, "one kernel" if took else "pass by pass", n_lds, len(mixed), sum(c.fits)))
        assert got == exp_n[:35] + c.expect + exp_n[35:], (c, label, "default route, with neighbours")
        assert passes == c.passes
        assert took == (c.cap <= 4096), (c, label, c.cap)
        if took:
            assert n_lds == len(NEIGHBOURS) + sum(c.fits), (c, label, n_lds, c.fits)
