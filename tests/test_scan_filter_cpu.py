"""The scan filter (image version 19, ImageHeader::off_scan_bloom; scan_mask in csrc/am_image.h): the keys of the filter at off_bloom once more, each under its
table mask ROTATED RIGHT by product bits 11..15.  k_sf copies this section into LDS; the section at off_bloom keeps the unrotated rule for everything that tests
a window in global memory.  The exact suffix keys are read back out of the image (tests/filter_keys.image_keys), both sections are rebuilt here and compared
bit for bit, in both case modes, for needle sets with all four tiers: a handful of needles, a set that fills a filter of 2^8 words to its two keys per word, and
one that reaches 2^15 words.  Needles are searched for until the keys take every rotation 0..31: 0 and 31 are the ends where a wrong shift shows.  CPU only."""
import itertools
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from tests.filter_keys import bloom_hash, filter_of, header, image_keys, log2_words, stored_filter, tier_key
from tests.helpers import ImgCheck
from tests.scan_filter import off_scan_bloom, rotr32, scan_filter_of, scan_mask, scan_rot, stored_scan_filter
from tests.test_filter_keys_cpu import NEEDLES

SHORT = ["k", "é", "ω", "kk", "ké", "q7", "z9k", "語"]      # needles of 1, 2 and 3 bytes: tiers 1-3


def until_every_rotation(needles, fold):
    """`needles` plus five-letter words a-z, taken in a fixed order, whose 4-byte suffix key rotates its mask by an amount no key rotated by yet."""
    seen = set()
    for n in needles:
        b = n.encode()
        t = min(len(b), 4)
        seen.add(scan_rot(bloom_hash(tier_key(int.from_bytes(b[-t:], "little"), t, fold), t)))
    out = list(needles)
    for letters in itertools.product("bcdfghjlmnpqrstvwxz", repeat=5):
        if len(seen) == 32:
            break
        w = "".join(letters)
        r = scan_rot(bloom_hash(tier_key(int.from_bytes(w.encode()[-4:], "little"), 4, fold), 4))
        if r not in seen:
            seen.add(r)
            out.append(w)
    assert len(seen) == 32
    return out


PLAIN = ["~", "q7", "z9q"]                                  # 1, 2, 3 bytes without a case variant outside ASCII: one filter key each in either mode


def words(seed, n):
    """n words of 5-9 letters with n different 4-byte suffixes; no i, k or s, whose variants U+0130, U+212A and U+017F would be suffix keys of their own"""
    rng, out, ends = random.Random(seed), [], set()
    while len(out) < n:
        w = "".join(rng.choice("abcdefghjlmnopqrtuvwxyz") for _ in range(rng.randint(5, 9)))
        if w[-4:] not in ends:
            ends.add(w[-4:])
            out.append(w)
    return out


def needle_sets(fold):
    """name -> (needles, log2 of the filter's words)"""
    few = until_every_rotation(NEEDLES, fold)
    # two keys per word: 512 distinct filter keys are what 2^8 words hold, 513 would take 2^9
    full = PLAIN + words("scan-2^8", 512 - len(PLAIN))
    big = SHORT + words("scan-2^15", 34000)
    return {"few": (few, 8), "2^8 words full": (full, 8), "2^15 words": (big, 15)}


@pytest.fixture(scope="module")
def chk():
    return ImgCheck()


def test_rotr32_at_both_ends():
    assert rotr32(0x80000001, 0) == 0x80000001 and rotr32(0x80000001, 31) == 0x00000003 and rotr32(0x80000001, 1) == 0xC0000000
    assert all(bin(rotr32(0x00010203, r)).count("1") == 4 for r in range(32))


@pytest.mark.parametrize("name", ["few", "2^8 words full", "2^15 words"])
@pytest.mark.parametrize("case", [0, 1], ids=["CaseSensitive", "IgnoreCase"])
def test_both_sections_hold_the_keys_under_their_rule(chk, case, name):
    fold = case == 1
    needles, want_lw = needle_sets(fold)[name]
    img = chk.flatten(am.Automaton(needles), case).tobytes()
    h = header(img)
    assert h["version"] == 19 and h["case_mode"] == case and h["sf_tiers"] == 0xF
    lw = h["sf_bloom_log2_words"]
    keys = image_keys(img, h)
    fkeys = {(t, tier_key(k, t, fold)) for t, k in keys}
    assert lw == want_lw == log2_words(len(fkeys))
    if name == "2^8 words full":
        assert len(fkeys) == 512
    # the section at off_bloom is what it was: the unrotated rule
    plain, n = filter_of(keys, lw, fold)
    assert n == len(fkeys) and np.array_equal(plain, stored_filter(img, h))
    # the scan section: the same keys, rotated masks, a section of its own inside the image
    off = off_scan_bloom(img)
    assert off % 4 == 0 and off + (4 << lw) <= h["total_bytes"] == len(img) and abs(off - h["off_bloom"]) >= 4 << lw
    stored = stored_scan_filter(img, h)
    assert np.array_equal(scan_filter_of(keys, lw, fold), stored)
    assert not np.array_equal(stored, stored_filter(img, h))
    # every key passes it, and the keys take every rotation
    rots = set()
    for t, k in fkeys:
        hh = bloom_hash(k, t)
        m = scan_mask(hh)
        assert int(stored[hh >> (32 - lw)]) & m == m, (t, hex(k))
        rots.add(scan_rot(hh))
    assert rots == set(range(32))


def test_the_scan_section_adds_one_filter_to_the_image(chk):
    """same size as the filter at off_bloom: 128 KiB at most"""
    needles, _ = needle_sets(False)["2^15 words"]
    img = chk.flatten(am.Automaton(needles), 0).tobytes()
    h = header(img)
    assert 4 << h["sf_bloom_log2_words"] == 128 * 1024
    a = sorted([h["off_bloom"], off_scan_bloom(img)])
    assert a[1] - a[0] >= 128 * 1024
