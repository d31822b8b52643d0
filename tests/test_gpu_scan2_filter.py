"""k_sf's W2 instantiations (csrc/am_kernels.hip): the launches that filter with the derived two-word filter (csrc/am_image.h scan2_mask), against the oracle.  The
needle set is tests/scan2_filter.py's `large` -- just over 3 * 2^15 distinct suffix keys, the three searched-for keys among them --, in both case modes:
  edge    16 385 bytes           the first batch beyond the light configuration
  full    256 KiB                one-chunk units
  units   ~17 MiB on 256 CUs     sf_unit_chunks >= 2: the carry between the chunks of a unit
Records, counts, containsAny and containsAll equal the oracle's; bit 10 of am_debug_sf_last_variant is set for count / emit / containsAny beyond the light
configuration and clear for containsAll and for a 16 384-byte call, and decode_sf_variant's dict is the one the same image got before; the traced launch writes the
untraced launch's bytes; planted needles end in every byte of lanes 0, 1, 31, 62 and 63; a handle attached to a copy of the image (device to device, or from the
host) scans with the W2 instantiation and writes the same records; the 60 000-key set launches what it launched."""
import ctypes as C
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from alfred_margaret_amd import api
from oracle import oracle
from tests import scan2_filter as s2
from tests.helpers import ImgCheck, expand_records, oracle_triples, sf_expand, sf_oracle_records

pytestmark = pytest.mark.gpu

SIZES = {"edge": 16 * 1024 + 1, "full": 256 * 1024}


class Large:
    def __init__(self):
        self.needles = s2.needle_sets()["large"]
        self.a, self.o = am.Automaton(self.needles), oracle.Machine(self.needles)
        self.a.set_kernel(2)
        self.vo, self.vals = self.a.values_off(), self.a.values()
        self.searchers = {}
        self.first = {case: list(s2.searched().values()) + [s2.rejected_window(self.needles, case == 1)] for case in (0, 1)}

    def searcher(self, case):
        if case not in self.searchers:
            self.searchers[case] = am.Searcher(case, self.needles)
        return self.searchers[case]

    def text(self, case, n_bytes):
        t = s2.make_text(self.needles, n_bytes, case, 0, self.first[case])
        return t, s2.cut(t, case)


@pytest.fixture(scope="module")
def large():
    f = Large()
    yield f
    f.searchers.clear()
    del f.a
    am.api.libam().am_release_device_memory()
    am.api.libam().am_release_host_memory()


@pytest.fixture(autouse=True)
def _no_table_walk():
    am.debug_set("AM_DFA", 0)
    api.sf_last_variant()          # (reading clears)
    yield


def variant_of(call):
    assert api.sf_last_variant() is None
    out = call()
    return out, api.sf_last_variant_w2()


def want_variant(case, mode, dbg=False, w2=True):
    """decode_sf_variant's dict of a launch beyond the light configuration: the W2 instantiations probe one candidate per lane (kSfW2Ilp)"""
    return {"ic": bool(case), "mode": mode, "ilp": 1 if w2 else 2, "lw": 15, "short": False, "dbg": dbg, "light": False, "children": False}


def slices(text, offs):
    return [text[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def strictly_ascending(rs):
    k = (rs["haystack"].astype(np.uint64) << np.uint64(32)) | rs["end_pos"].astype(np.uint64)
    return bool((k[1:] > k[:-1]).all())


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", (0, 1))
def test_records_counts_and_flags_equal_the_oracle(large, case, size):
    f = large
    text, offs = f.text(case, SIZES[size])
    assert all(w.encode() in text[:64] for w in f.first[case])          # the searched-for keys and the rejected window are in the text
    hays = slices(text, offs)
    exp = oracle_triples(f.o, case, hays)
    assert len(exp) > (150 if size == "edge" else 3000)
    rs, (v, w2) = variant_of(lambda: f.a.run_records(case, hays))
    assert v == want_variant(case, "emit") and w2
    assert expand_records(f.vo, f.vals, rs["haystack"], rs["state"], rs["end_pos"]) == exp
    assert strictly_ascending(rs)
    counts, (v, w2) = variant_of(lambda: f.a.count_matches(case, hays))
    assert v == want_variant(case, "count") and w2
    assert np.array_equal(counts, np.bincount([h for h, _, _ in exp], minlength=len(hays)))
    flags, (v, w2) = variant_of(lambda: f.searcher(case).contains_any_batch(hays))
    assert v == want_variant(case, "any") and w2
    want = np.asarray([f.o.contains_any(case, h) for h in hays])
    assert want.any() and not want.all()
    assert np.array_equal(flags, want)


@pytest.mark.parametrize("case", (0, 1))
def test_the_light_call_and_contains_all_keep_the_scan_filter(large, case):
    f = large
    text, offs = f.text(case, 16 * 1024)
    hays = slices(text, offs)
    exp = oracle_triples(f.o, case, hays)
    rs, (v, w2) = variant_of(lambda: f.a.run_records(case, hays))
    assert v["light"] and v["lw"] == 0 and not w2
    assert expand_records(f.vo, f.vals, rs["haystack"], rs["state"], rs["end_pos"]) == exp
    # containsAll beyond the light configuration: every needle, the same with the last byte of one needle changed, half of them, nothing
    up = (lambda x: x.upper()) if case else (lambda x: x)
    spoiled = list(f.needles)
    victim = max(range(len(spoiled)), key=lambda i: len(spoiled[i]))
    spoiled[victim] = spoiled[victim][:-1] + "#"
    hays = [up(" ".join(f.needles)).encode(), " ".join(spoiled).encode(), " ".join(f.needles[::2]).encode(), b""]
    want = [f.o.contains_all(case, h) for h in hays]
    assert want == [True, False, False, False]
    flags, (v, w2) = variant_of(lambda: f.searcher(case).contains_all_batch(hays))
    assert v["mode"] == "ids" and not v["light"] and not w2
    assert flags.tolist() == want


@pytest.mark.parametrize("case", (0, 1))
def test_units_of_several_chunks(large, case):
    f = large
    w = 16 * am.device_info()["n_cu"]
    total = (4 * w + w // 4) * 1024 + 19
    uc = api.sf_unit_chunks(total)
    assert uc >= 2, (total, uc)
    base, _ = f.text(case, SIZES["full"])
    text = np.resize(np.frombuffer(base, dtype=np.uint8), total).tobytes()
    offs = s2.cut(text, 7 + case, n_cuts=200)
    hays = slices(text, offs)
    exp = sf_oracle_records(f.o, case, text, offs)
    assert len(exp[0]) > 200000
    rs, (v, w2) = variant_of(lambda: f.a.run_records(case, hays))
    assert v == want_variant(case, "emit") and w2
    got = sf_expand(rs["haystack"], rs["state"], rs["end_pos"], f.vo, f.vals)
    assert all(np.array_equal(g, e) for g, e in zip(got, exp))
    assert strictly_ascending(rs)
    counts, (v, w2) = variant_of(lambda: f.a.count_matches(case, hays))
    assert v == want_variant(case, "count") and w2
    assert np.array_equal(counts, np.bincount(exp[0], minlength=len(hays)))


@pytest.mark.parametrize("case", (0, 1))
def test_traced_launches_write_the_same_records(large, case):
    f = large
    text, offs = f.text(case, SIZES["full"])
    hays = slices(text, offs)
    plain, _ = variant_of(lambda: f.a.run_records(case, hays))
    plain_counts, _ = variant_of(lambda: f.a.count_matches(case, hays))
    assert len(plain) > 3000
    am.debug_set("AM_SF_TRACE", 1)
    traced, (v, w2) = variant_of(lambda: f.a.run_records(case, hays))
    assert v == want_variant(case, "emit", dbg=True) and w2
    traced_counts, (v, w2) = variant_of(lambda: f.a.count_matches(case, hays))
    assert v == want_variant(case, "count", dbg=True) and w2
    assert plain.tobytes() == traced.tobytes()
    assert np.array_equal(plain_counts, traced_counts)


@pytest.mark.parametrize("case", (0, 1))
def test_needles_end_in_every_byte_of_the_edge_lanes(large, case):
    """One needle per KiB chunk, ending at offset 16 * L + k of its chunk for L in {0, 1, 31, 62, 63} and every k: lane L's position k.  Those of lane 0 begin in the
    chunk before (across the chunk edge); the last one ends on the batch's last byte."""
    f = large
    rng = random.Random("scan2-lanes-%d" % case)
    spots = [(L, k) for L in (0, 1, 31, 62, 63) for k in range(16)]
    total = len(spots) * 1024 + 63 * 16 + 15 + 1
    t = bytearray(b"#" * total)
    ends = []
    for i, (L, k) in enumerate(spots + [(63, 15)]):
        nd = rng.choice(f.needles)
        if case:
            nd = "".join(c.upper() if rng.random() < 0.5 else c for c in nd)
        end = (i + 1) * 1024 + 16 * L + k if i < len(spots) else total - 1
        t[end + 1 - len(nd):end + 1] = nd.encode()
        ends.append(end)
    assert ends[-1] == total - 1 and any(e % 1024 < 4 for e in ends)
    hays = [bytes(t)]
    exp = oracle_triples(f.o, case, hays)
    assert {p for _, p, _ in exp} >= {e + 1 for e in ends}          # (matchPos: the offset behind the match)
    rs, (v, w2) = variant_of(lambda: f.a.run_records(case, hays))
    assert w2 and expand_records(f.vo, f.vals, rs["haystack"], rs["state"], rs["end_pos"]) == exp
    counts, (v, w2) = variant_of(lambda: f.a.count_matches(case, hays))
    assert w2 and counts.tolist() == [len(exp)]


@pytest.mark.parametrize("case", (0, 1))
def test_an_image_copy_derives_the_same_words(large, case):
    """am_automaton_image_copy -> am_automaton_from_image (the broadcast path) and am_automaton_from_host_image: the copy is the image byte for byte, so the one
    routine derives the same words from it, and a scan with either attached handle takes the W2 instantiation and writes the fresh handle's records."""
    f = large
    chk = ImgCheck()
    img = f.a.image_bytes(case)
    want = s2.derived_words(chk, img)
    assert want is not None
    text, offs = f.text(case, SIZES["full"])
    hays = slices(text, offs)
    fresh = f.a.run_records(case, hays).tobytes()
    api.sf_last_variant()
    lib = api.libam()
    n = C.c_size_t(0)
    api.check(lib.am_automaton_image_size(f.a.device, case, C.byref(n)))
    hip = C.CDLL("libamdhip64.so")
    buf, h = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(n.value)) == 0
    try:
        api.check(lib.am_automaton_image_copy(f.a.device, case, buf, n.value))
        api.check(lib.am_automaton_from_image(buf, n.value, C.byref(h)))
    finally:
        hip.hipFree(buf)
    copied = am.api.ImageAutomaton.__new__(am.api.ImageAutomaton)          # (the wrapper around a handle that exists: it destroys it)
    copied._h = h
    for ia in (copied, am.api.ImageAutomaton(img)):
        back = (C.c_uint8 * n.value)()
        api.check(lib.am_automaton_image_read(ia.device, case, back, n.value))
        assert bytes(back) == img and np.array_equal(s2.derived_words(chk, bytes(back)), want)
        api.check(lib.am_automaton_set_kernel(ia.device, 2))
        rs, (v, w2) = variant_of(lambda: ia.run_records(case, hays))
        assert v == want_variant(case, "emit") and w2 and rs.tobytes() == fresh


def test_the_60000_key_set_launches_what_it_launched():
    needles = s2.needle_sets()["60000"]
    a, o = am.Automaton(needles), oracle.Machine(needles)
    a.set_kernel(2)
    assert s2.derived_words(ImgCheck(), a.image_bytes(1)) is None
    text = s2.make_text(needles, SIZES["full"], 1, 1)
    hays = slices(text, s2.cut(text, 3))
    rs, (v, w2) = variant_of(lambda: a.run_records(1, hays))
    assert v == want_variant(1, "emit", w2=False) and not w2
    assert expand_records(a.values_off(), a.values(), rs["haystack"], rs["state"], rs["end_pos"]) == oracle_triples(o, 1, hays)
