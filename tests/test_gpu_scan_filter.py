"""k_sf tests windows against the SCAN filter (image version 19): every key's table mask rotated right by product bits 11..15 (scan_mask, csrc/am_image.h), in
the tier-4 loop of the kernel and in sf_filter_short's LDS flavour.  A wrong rotation loses real hits, so everything is held to the oracle: records, counts,
containsAny and containsAll, in both case modes, for the families of tests/helpers.py that reach the LW = 15 instantiations ("mid": ILP 1, "large": ILP 2), a
SHORT one ("mid+short"), the CHILDREN one ("dict") and, at 16 384 bytes, the light configuration of each; at 16 384 bytes, 16 385 bytes and 256 KiB, and in
one batch of several chunks per work unit.  One text is made of every needle and of every needle's 4-byte suffix behind bytes that differ from the needle's in
bit 5: the suffix keys take every rotation 0..31, and each of them must pass.  One AM_SF_TRACE launch writes the untraced launch's bytes."""
import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests.filter_keys import bloom_hash, tier_key
from tests.helpers import expand_records, oracle_triples, sf_expand, sf_family_needles, sf_oracle_records, sf_text
from tests.scan_filter import scan_rot
from tests.test_gpu_sf_variants import family_of, launched, slices, strictly_ascending
from tests.test_sf_variants_cpu import CELLS, PURPOSE, launch_rule

pytestmark = pytest.mark.gpu

FAMILIES = ("mid", "large", "mid+short", "dict")
SIZES = {"light": 16 * 1024, "edge": 16 * 1024 + 1, "full": 256 * 1024}


@pytest.fixture(autouse=True)
def _k_sf_only():
    """AM_DFA = 0: the Searcher's automaton gets no DFA section, every batch goes to k_sf"""
    am.debug_set("AM_DFA", 0)
    am.api.sf_last_variant()          # (reading clears)
    yield


def test_the_families_reach_the_instantiations_they_are_here_for():
    assert PURPOSE["mid"] == (1, 15, False, False) and PURPOSE["large"] == (2, 15, False, False) and PURPOSE["mid+short"] == (1, 15, True, False)
    assert PURPOSE["dict"] == (2, 0, False, True)
    assert all(launch_rule(CELLS[f][c], c, "emit", 16)["light"] for f in FAMILIES for c in (0, 1))


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
    assert np.array_equal(flags, np.asarray([f.o.contains_any(case, h) for h in hays]))


def suffix_text(needles, case):
    """(text, offsets): every needle as it is and, for the a-z words, once more with every byte before its last four flipped in bit 5 -- upper case: a match
    under IgnoreCase, a window that passes the filter and dies in the resolve under CaseSensitive.  A haystack per 2 000 needles."""
    parts, offs, at = [], [0], 0
    for i, n in enumerate(needles):
        b = n.encode("utf-8")
        p = b + b" "
        if n.isascii() and len(b) > 4:
            p += bytes(c ^ 0x20 for c in b[:-4]) + b[-4:] + b" "
        parts.append(p)
        at += len(p)
        if i % 2000 == 1999:
            offs.append(at)
    if offs[-1] != at:
        offs.append(at)
    return b"".join(parts), np.asarray(offs, dtype=np.int64)


@pytest.mark.parametrize("case", (0, 1))
@pytest.mark.parametrize("family", ("mid", "mid+short", "dict"))
def test_no_suffix_is_lost_at_any_rotation(family, case):
    f = family_of(family)
    rots = set()
    for n in f.needles:
        b = n.encode("utf-8")
        t = min(len(b), 4)
        rots.add(scan_rot(bloom_hash(tier_key(int.from_bytes(b[-t:], "little"), t, case == 1), t)))
    assert rots == set(range(32))
    text, offs = suffix_text(f.needles, case)
    hays = slices(text, offs)
    exp = sf_oracle_records(f.o, case, text, offs)
    flipped = sum(1 for n in f.needles if n.isascii() and len(n) > 4)
    assert len(exp[0]) >= len(f.needles) + (flipped if case else 0) and flipped > len(f.needles) // 2
    rs = f.a.run_records(case, hays)
    got = sf_expand(rs["haystack"], rs["state"], rs["end_pos"], f.vo, f.vals)
    assert all(np.array_equal(g, e) for g, e in zip(got, exp))
    counts = f.a.count_matches(case, hays)
    assert np.array_equal(counts, np.bincount(exp[0], minlength=len(hays)))


@pytest.mark.parametrize("family,case", [("large", 1), ("mid+short", 0)])
def test_units_of_several_chunks(family, case):
    """the family's 256-KiB text tiled until a work unit is two chunks or more: the filter keys of a chunk's first windows come out of the carry"""
    f = family_of(family)
    w = 16 * am.device_info()["n_cu"]
    total = (2 * w + w // 4) * 1024 + 19
    assert am.api.sf_unit_chunks(total) >= 2
    base, base_offs = sf_text(family, case, 256 * 1024)
    reps = total // len(base) + 1
    text = base * reps
    offs = np.concatenate([base_offs[:-1] + k * len(base) for k in range(reps)] + [[reps * len(base)]]).astype(np.int64)
    assert am.api.sf_unit_chunks(len(text)) >= 2
    hays = slices(text, offs)
    one = sf_oracle_records(f.o, case, base, base_offs)
    n_base = len(base_offs) - 1
    exp = (np.concatenate([one[0] + np.uint32(k * n_base) for k in range(reps)]), np.tile(one[1], reps), np.tile(one[2], reps))
    rs = launched(lambda: f.a.run_records(case, hays), family, case, "emit", len(text))
    got = sf_expand(rs["haystack"], rs["state"], rs["end_pos"], f.vo, f.vals)
    assert len(exp[0]) > 100000 and all(np.array_equal(g, e) for g, e in zip(got, exp))
    counts = launched(lambda: f.a.count_matches(case, hays), family, case, "count", len(text))
    assert np.array_equal(counts, np.bincount(exp[0], minlength=len(hays)))


@pytest.mark.parametrize("light", (True, False), ids=("light", "full"))
@pytest.mark.parametrize("case", (0, 1))
@pytest.mark.parametrize("family", ("mid", "mid+short"))
def test_contains_all(family, case, light):
    """four haystacks: every needle, the same with the last byte of one needle changed, half of them, nothing; the light batch takes a 300-needle prefix"""
    needles = sf_family_needles(family)
    if light:
        needles = needles[:290] + needles[-10:]
    o, s = oracle.Machine(needles), am.Searcher(case, needles)
    up = (lambda x: x.translate(str.maketrans("abcdefghijklmnopqrstuvwxyz", "ABCDEFGHIJKLMNOPQRSTUVWXYZ"))) if case else (lambda x: x)
    victim = max(range(len(needles)), key=lambda i: len(needles[i]))
    spoiled = list(needles)
    spoiled[victim] = spoiled[victim][:-1] + "#"
    hays = [up(" ".join(needles)).encode("utf-8"), " ".join(spoiled).encode("utf-8"), " ".join(needles[::2]).encode("utf-8"), b""]
    assert (sum(len(h) for h in hays) <= 16 * 1024) == light
    want = [o.contains_all(case, h) for h in hays]
    assert want == [True, False, False, False]
    assert s.contains_all_batch(hays).tolist() == want


def test_a_traced_launch_writes_the_same_bytes():
    f, case, total = family_of("mid"), 1, SIZES["full"]
    text, offs = sf_text("mid", case, total)
    hays = slices(text, offs)
    plain = launched(lambda: f.a.run_records(case, hays), "mid", case, "emit", total)
    am.debug_set("AM_SF_TRACE", 1)
    try:
        traced = launched(lambda: f.a.run_records(case, hays), "mid", case, "emit", total, trace=True)
    finally:
        am.debug_set("AM_SF_TRACE", -1)
    assert len(plain) > 5000 and plain.tobytes() == traced.tobytes()
