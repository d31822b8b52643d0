"""Every k_sf instantiation launch_sf_t (csrc/am_kernels.hip) can pick, against the oracle.  The needle families of tests/helpers.py put an automaton's image into each
cell of the rule (tests/test_sf_variants_cpu.py: CELLS, launch_rule -- checked there on the CPU, with the image's host interpreter held to the oracle on the same texts);
here every call is routed to k_sf (am_automaton_set_kernel(a, 2); AM_DFA = 0 for the Searcher), and after every call am_debug_sf_last_variant must name the instantiation
the rule predicts for it.  The batches:
  light   16 384 bytes         the light configuration (256-thread workgroups), whatever the image
  edge    16 385 bytes         the first batch beyond it
  full    256 KiB              one-chunk units
  units   ~17 MiB on 256 CUs   sf_unit_chunks >= 2 (5 there): the carry between the chunks of a unit; once per (ILP, LW, SHORT, CHILDREN), count and emit
claimed_variants() lists what the cases below launch; the CPU file holds it, plus its list of unreached variants, to everything the rule can return."""
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests.helpers import SF_SHORT_NEEDLES, expand_records, oracle_triples, ragged_cuts, sf_expand, sf_family_needles, sf_oracle_records, sf_text
from tests.test_sf_variants_cpu import CELLS, FAMILIES, launch_rule

pytestmark = pytest.mark.gpu

SIZES = {"light": 16 * 1024, "edge": 16 * 1024 + 1, "full": 256 * 1024}
UNITS = [("small", 0), ("mid", 1), ("large", 0), ("dict", 1), ("small+short", 1), ("mid+short", 0), ("large+short", 1), ("forked+short", 0)]      # one per (ILP, LW, SHORT, CHILDREN)
UNITS_CHUNKS = 17 * 1024                                    # any batch beyond the light one gives the same variant; the test computes its size from the device
ALL_FAMILIES = ("small", "small+short")                     # containsAll: the ids instantiations differ by case mode, SHORT and light only
TRACED = ("small", "mid", "mid+short")                      # <2, 0, SHORT, DBG> (for every filter below 2^15 words), <2, 15, no SHORT, DBG>, <2, 15, SHORT, DBG>


def claimed_variants():
    """The variant of every k_sf launch the tests of this file assert (as launch_rule names it)."""
    out = []
    for family in FAMILIES:
        for case in (0, 1):
            for total in SIZES.values():
                out += [launch_rule(CELLS[family][case], case, mode, (total + 1023) // 1024) for mode in ("emit", "count", "any")]
    for family, case in UNITS:
        out += [launch_rule(CELLS[family][case], case, mode, UNITS_CHUNKS) for mode in ("emit", "count")]
    for family in ALL_FAMILIES:
        for case in (0, 1):
            out += [launch_rule(CELLS[family][case], case, "ids", chunks) for chunks in (16, 17)]
    for family in TRACED:
        for case in (0, 1):
            out += [launch_rule(CELLS[family][case], case, mode, 256, trace=True) for mode in ("emit", "count")]
    return out


class Family:
    """The automaton (suffix-filter route), the oracle's machine and the Searchers of one family, built once per module."""

    def __init__(self, name):
        self.name, self.needles = name, sf_family_needles(name)
        self.a, self.o = am.Automaton(self.needles), oracle.Machine(self.needles)
        self.a.set_kernel(2)
        self.vo, self.vals = self.a.values_off(), self.a.values()
        self.searchers = {}

    def searcher(self, case):
        if case not in self.searchers:
            self.searchers[case] = am.Searcher(case, self.needles)
        return self.searchers[case]


_FAMILIES = {}


def family_of(name):
    if name not in _FAMILIES:
        _FAMILIES[name] = Family(name)
    return _FAMILIES[name]


@pytest.fixture(scope="module", autouse=True)
def _release_at_the_end():
    yield
    _FAMILIES.clear()
    am.api.libam().am_release_device_memory()
    am.api.libam().am_release_host_memory()


@pytest.fixture(autouse=True)
def _no_table_walk():
    """The Searcher's automaton is its own (no am_automaton_set_kernel from here): AM_DFA = 0 gives no image a DFA section and sends no batch to k_dfa."""
    am.debug_set("AM_DFA", 0)
    am.api.sf_last_variant()          # (reading clears)
    yield


def launched(call, family, case, mode, total, trace=False):
    """call(), then the variant it launched against the rule's."""
    assert am.api.sf_last_variant() is None
    out = call()
    got, want = am.api.sf_last_variant(), launch_rule(CELLS[family][case], case, mode, (total + 1023) // 1024, trace)
    assert got == want, (family, case, mode, total, got, want)
    return out


def strictly_ascending(rs):
    k = (rs["haystack"].astype(np.uint64) << np.uint64(32)) | rs["end_pos"].astype(np.uint64)
    return bool((k[1:] > k[:-1]).all())


def slices(text, offs):
    return [text[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", (0, 1))
@pytest.mark.parametrize("family", FAMILIES)
def test_records_counts_and_flags_equal_the_oracle(family, case, size):
    f, total = family_of(family), SIZES[size]
    text, offs = sf_text(family, case, total)
    hays = slices(text, offs)
    exp = oracle_triples(f.o, case, hays)
    assert len(exp) > (200 if size != "full" else 5000)
    rs = launched(lambda: f.a.run_records(case, hays), family, case, "emit", total)
    assert expand_records(f.vo, f.vals, rs["haystack"], rs["state"], rs["end_pos"]) == exp
    assert strictly_ascending(rs)
    counts = launched(lambda: f.a.count_matches(case, hays), family, case, "count", total)
    assert np.array_equal(counts, np.bincount([h for h, _, _ in exp], minlength=len(hays)))
    flags = launched(lambda: f.searcher(case).contains_any_batch(hays), family, case, "any", total)
    want = np.asarray([f.o.contains_any(case, h) for h in hays])
    assert want.any() and not want[np.diff(offs) > 0].all()
    assert np.array_equal(flags, want)
    assert np.array_equal(want, counts > 0)


@pytest.mark.parametrize("family,case", UNITS, ids=["%s-case%d" % fc for fc in UNITS])
def test_units_of_several_chunks(family, case):
    """sf_unit_chunks >= 2: a wavefront walks the chunks of its unit one after the other and carries the 4 bytes before a lane's 16 and the 8 staged bytes before the
    chunk from one to the next.  The family's 256-KiB text tiled to 4.25 KiB per wavefront, cut by ragged_cuts (haystack ends on a unit's last byte among them)."""
    f = family_of(family)
    w = 16 * am.device_info()["n_cu"]
    total = (4 * w + w // 4) * 1024 + 19
    uc = am.api.sf_unit_chunks(total)
    assert uc >= 2, (total, uc)
    base, _ = sf_text(family, case, 256 * 1024)
    t = np.resize(np.frombuffer(base, dtype=np.uint8), total)
    k = total - 1
    while (t[k] & 0xC0) == 0x80:
        k -= 1
    if t[k] >= 0xC0:                       # the code point the end cuts
        t[k:] = ord("x")
    offs = ragged_cuts(t, random.Random(17), uc * 1024, big=3 << 20)
    text = t.tobytes()
    hays = slices(text, offs)
    exp = sf_oracle_records(f.o, case, text, offs)
    assert len(exp[0]) > 300000
    rs = launched(lambda: f.a.run_records(case, hays), family, case, "emit", total)
    got = sf_expand(rs["haystack"], rs["state"], rs["end_pos"], f.vo, f.vals)
    assert all(np.array_equal(g, e) for g, e in zip(got, exp))
    assert strictly_ascending(rs)
    counts = launched(lambda: f.a.count_matches(case, hays), family, case, "count", total)
    assert np.array_equal(counts, np.bincount(exp[0], minlength=len(hays)))


@pytest.mark.parametrize("light", (True, False), ids=("light", "full"))
@pytest.mark.parametrize("case", (0, 1))
@pytest.mark.parametrize("family", ALL_FAMILIES)
def test_contains_all(family, case, light):
    """Searcher.containsAll sets the needle ids inside k_sf (mode ids).  Four haystacks: every needle, the same with the last byte of one needle changed, half of
    them, nothing.  The light batch takes a 300-needle prefix of the family (its short needles included)."""
    needles = sf_family_needles(family)
    if light:
        needles = needles[:300 - len(SF_SHORT_NEEDLES)] + SF_SHORT_NEEDLES if family.endswith("+short") else needles[:300]
    o, s = oracle.Machine(needles), am.Searcher(case, needles)
    up = (lambda x: x.translate(str.maketrans("abcdefghijklmnopqrstuvwxyz", "ABCDEFGHIJKLMNOPQRSTUVWXYZ"))) if case else (lambda x: x)
    victim = max(range(len(needles)), key=lambda i: len(needles[i]))
    spoiled = list(needles)
    spoiled[victim] = spoiled[victim][:-1] + ("#" if spoiled[victim][-1] != "#" else "x")
    hays = [up(" ".join(needles)).encode("utf-8"), " ".join(spoiled).encode("utf-8"), " ".join(needles[::2]).encode("utf-8"), b""]
    total = sum(len(h) for h in hays)
    assert (total <= 16 * 1024) == light
    want = [o.contains_all(case, h) for h in hays]
    assert want == [True, False, False, False]
    flags = launched(lambda: s.contains_all_batch(hays), family, case, "ids", total)
    assert flags.tolist() == want


@pytest.mark.parametrize("case", (0, 1))
@pytest.mark.parametrize("family", TRACED)
def test_traced_launches_write_the_same_records(family, case):
    """AM_SF_TRACE only times: the instrumented instantiations give the untraced launch's records byte for byte, and its counts."""
    f, total = family_of(family), SIZES["full"]
    text, offs = sf_text(family, case, total)
    hays = slices(text, offs)
    plain = launched(lambda: f.a.run_records(case, hays), family, case, "emit", total)
    plain_counts = launched(lambda: f.a.count_matches(case, hays), family, case, "count", total)
    assert len(plain) > 5000
    am.debug_set("AM_SF_TRACE", 1)
    traced = launched(lambda: f.a.run_records(case, hays), family, case, "emit", total, trace=True)
    traced_counts = launched(lambda: f.a.count_matches(case, hays), family, case, "count", total, trace=True)
    assert launch_rule(CELLS[family][case], case, "emit", 256, trace=True)["dbg"]
    assert plain.tobytes() == traced.tobytes()
    assert np.array_equal(plain_counts, traced_counts)
