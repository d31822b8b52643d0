"""The two-word scan filter (scan2_mask in csrc/am_image.h, scan2_derive in csrc/am_flatten.cpp): derived from an image's own tier-4 keys where the 2^15-word filter
holds more than three keys per word and no needle is shorter than 4 bytes; never part of the image.  The rule is restated in tests/scan2_filter.py; here the words
scan2_derive gives on the host (amflat_scan2_filter, exported by the test library libam_imgcheck.so) are held to it bit for bit, in both case modes, the image is shown to be what it was (version 19, both stored sections
under their rules), and the sets that must get no derived filter get none: exactly at the threshold, 60 000 keys, a large set with one 2-byte needle.  CPU only; the
copy of an image from device to device has no CPU form and is tested in tests/test_gpu_scan2_filter.py."""
import numpy as np
import pytest

import alfred_margaret_amd as am
from tests import scan2_filter as s2
from tests.filter_keys import bloom_hash, filter_of, header, image_keys, stored_filter, tier_key
from tests.helpers import ImgCheck
from tests.scan_filter import scan_filter_of, scan_mask, scan_rot, stored_scan_filter

CASES = pytest.mark.parametrize("case", [0, 1], ids=["CaseSensitive", "IgnoreCase"])


@pytest.fixture(scope="module")
def chk():
    return ImgCheck()


@pytest.fixture(scope="module")
def automata():
    """name -> Automaton, built once"""
    return {name: am.Automaton(needles) for name, needles in s2.needle_sets().items()}


def test_three_bit_entries_are_the_table_entries_without_their_last_bit():
    from tests.filter_keys import MASKS
    assert [s2.mask_entry_n(i, 4) for i in range(512)] == MASKS
    for i in range(512):
        assert bin(s2.MASKS3[i]).count("1") == 3 and s2.MASKS3[i] & MASKS[i] == s2.MASKS3[i]
        assert s2.mask_entry_n(i, 2) & s2.MASKS3[i] == s2.mask_entry_n(i, 2)


@CASES
def test_derived_words_equal_the_rule_and_the_image_is_what_it_was(chk, automata, case):
    fold = case == 1
    a = automata["large"]
    img = chk.flatten(a, case).tobytes()
    h = header(img)
    keys = image_keys(img, h)
    assert h["version"] == 19 and h["case_mode"] == case and h["sf_tiers"] == 8 and h["sf_bloom_log2_words"] == 15
    assert {k for _, k in keys} == {s2.key_of(w) for w in s2.needle_sets()["large"]}
    fkeys = {tier_key(k, 4, fold) for _, k in keys}
    assert len(fkeys) == s2.MIN_KEYS + 3 and s2.applies(h, keys, fold)
    # the image: both stored sections under today's rules
    assert np.array_equal(filter_of(keys, 15, fold)[0], stored_filter(img, h))
    assert np.array_equal(scan_filter_of(keys, 15, fold), stored_scan_filter(img, h))
    # the derived words, bit for bit
    want = s2.scan2_filter_of(keys, fold)
    got = s2.derived_words(chk, img)
    assert got is not None and got.dtype == np.uint32 and np.array_equal(got, want)
    assert not np.array_equal(got, stored_scan_filter(img, h))
    # every key passes both of its words
    for k in fkeys:
        hh = bloom_hash(k, 4)
        m = s2.scan2_mask(hh)
        assert int(got[s2.word1(hh)]) & m == m and int(got[s2.word2(hh)]) & m == m and bin(m).count("1") == 3, hex(k)


@CASES
@pytest.mark.parametrize("name", ["threshold", "60000", "large + a 2-byte needle"])
def test_sets_without_a_derived_filter(chk, automata, case, name):
    a = automata[name]
    img = chk.flatten(a, case).tobytes()
    assert s2.derived_words(chk, img) is None
    if case == 1:                          # why the rule says no
        h = header(img)
        keys = image_keys(img, h)
        assert h["sf_bloom_log2_words"] == 15 and not s2.applies(h, keys, True)
        n4 = len({tier_key(k, 4, True) for t, k in keys if t == 4})
        if name == "threshold":
            assert n4 == s2.MIN_KEYS and h["sf_tiers"] == 8
        elif name == "60000":
            assert n4 == 60000 and h["sf_tiers"] == 8
        else:
            assert n4 > s2.MIN_KEYS and h["sf_tiers"] & 7


@CASES
def test_searched_keys_and_the_rejected_window(case):
    fold = case == 1
    large = s2.needle_sets()["large"]
    ex = s2.searched()
    assert set(ex) == {"same word", "rotation 0", "rotation 31"} and all(w in large for w in ex.values())
    hh = bloom_hash(tier_key(s2.key_of(ex["same word"]), 4, fold), 4)
    # (a key whose two words are one word exists under CaseSensitive only: tests/scan2_filter.py SAME_WORD)
    assert (s2.word2(hh) == s2.word1(hh)) == (not fold) and ((hh >> 2) & 0x7FFF == 0) == (not fold)
    assert scan_rot(bloom_hash(s2.key_of(ex["rotation 0"]), 4)) == 0 and scan_rot(bloom_hash(s2.key_of(ex["rotation 31"]), 4)) == 31
    keys = {(4, s2.key_of(w)) for w in large}
    one, two = scan_filter_of(keys, 15, fold), s2.scan2_filter_of(keys, fold)
    assert all(s2.passes(two, tier_key(s2.key_of(w), 4, fold)) for w in ex.values())
    w = s2.rejected_window(large, fold)
    k = s2.key_of(w)
    hh = bloom_hash(k, 4)
    assert tier_key(k, 4, fold) == k and k not in {tier_key(x, 4, fold) for _, x in keys}
    assert int(one[hh >> 17]) & scan_mask(hh) == scan_mask(hh) and not s2.passes(two, k)
