"""The suffix filter's keys (bloom_key, csrc/am_image.h): an IgnoreCase image keys its filter by the window modulo the ASCII case bit (w | 0x20202020), a
CaseSensitive image by the window itself.  The exact suffix keys are read back out of the image (tier tables, cold cuckoo slots), the filter is rebuilt here
with the same hash and masks, and the host interpreter (libam_imgcheck.so) scans every case variant against the oracle.  CPU only."""
import itertools

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests.filter_keys import MASKS, bloom_hash, filter_of, header, image_keys, log2_words, stored_filter, tier_key
from tests.helpers import ImgCheck, expand_records, oracle_triples

# every case variant of a lower-case letter of the needles below (Unicode simple lower-case mapping): what an IgnoreCase image must find
VARIANTS = {"é": "éÉ", "р": "рР", "ω": "ωΩ\u2126", "k": "kK\u212a", "а": "аА", "с": "сС", "т": "тТ", "ф": "фФ", "a": "aA", "f": "fF", "c": "cC", "t": "tT", "s": "sS"}
NEEDLES = ["café", "ké", "kk", "éé", "старр", "рррр", "aω", "ωωω", "stack", "aké", "k", "é", "ω", "фаа"]


@pytest.fixture(scope="module")
def chk():
    return ImgCheck()


def variants(needle):
    return ["".join(p) for p in itertools.product(*[VARIANTS.get(c, c) for c in needle])]


def suffix_key(b):
    """(tier, key) of a needle variant's bytes: its last four bytes, newest on top, or all of them when there are fewer"""
    t = min(len(b), 4)
    return t, int.from_bytes(b[-t:], "little")


def fold_ascii(b):
    """fold_dword of am_image.h on bytes: A-Z -> a-z, nothing else"""
    return bytes(c + 0x20 if 0x41 <= c <= 0x5A else c for c in b)


def folded(text):
    """the filter key (tier, key) of a text's suffix under IgnoreCase"""
    t, k = suffix_key(fold_ascii(text.encode()))
    return t, tier_key(k, t, True)


def test_ignore_case_filter_holds_the_distinct_folded_keys(chk):
    img = chk.flatten(am.Automaton(NEEDLES), 1).tobytes()
    h = header(img)
    assert h["case_mode"] == 1 and h["sf_tiers"] == 0xF
    keys = image_keys(img, h)
    # the exact tables hold the suffix of every variant as the ASCII-folded text shows it: É next to é, U+212A next to k
    assert keys == {suffix_key(fold_ascii(v.encode())) for n in NEEDLES for v in variants(n)}
    f, n_folded = filter_of(keys, h["sf_bloom_log2_words"], True)
    assert folded("é") == folded("É") and folded("café") == folded("CAFÉ") and folded("фаа") == folded("фАА")      # one key: the pair differs in bit 5 of a byte
    assert folded("aω") != folded("aΩ") and folded("aω") != folded("a\u2126") and folded("р") != folded("Р") and folded("k") != folded("\u212a")      # two keys as before
    assert n_folded == len({folded(v) for n in NEEDLES for v in variants(n)}) < len(keys)
    assert np.array_equal(f, stored_filter(img, h))                  # the filter holds the folded keys, all of them and nothing else
    assert not np.array_equal(filter_of(keys, h["sf_bloom_log2_words"], False)[0], f)


def test_filter_is_sized_by_the_distinct_folded_keys(chk):
    """300 needles "??é": 600 exact suffix keys (é, É), 300 filter keys.  Two keys per word: 600 keys would take 2^9 words, 300 take 2^8."""
    needles = [a + b + "é" for a, b in itertools.islice(itertools.product("bcdfghjlmnpqrstvwxyz", repeat=2), 300)]
    img = chk.flatten(am.Automaton(needles), 1).tobytes()
    h = header(img)
    keys = image_keys(img, h)
    f, n_folded = filter_of(keys, h["sf_bloom_log2_words"], True)
    assert (len(keys), n_folded) == (600, 300)
    assert log2_words(len(keys)) == 9 and h["sf_bloom_log2_words"] == log2_words(n_folded) == 8
    assert np.array_equal(f, stored_filter(img, h))
    img = chk.flatten(am.Automaton(needles), 0).tobytes()            # CaseSensitive: 300 keys as they are
    h = header(img)
    assert h["sf_bloom_log2_words"] == 8 and len(image_keys(img, h)) == 300


def test_every_variant_suffix_passes_the_host_filter(chk):
    o = oracle.Machine(NEEDLES)
    img = chk.flatten(am.Automaton(NEEDLES), 1)
    hays = []
    for n in NEEDLES:
        vs = variants(n)
        hays += vs + ["@`" + v + "[{" for v in vs] + [" ".join(vs)]
    # what differs from a needle in bit 5 of a byte without being its case variant must not match: × / ÷ and ß / ÿ are no case pairs, nor are ` / @
    hays += ["cafÉ café cafÈ cafè", "×÷ßÿ", "kK@`\u212aKKk", "".join(chr(ord(c) ^ 0x20) for c in "stack"), "ÐÑÐñ"]
    exp = oracle_triples(o, 1, hays)
    assert len(exp) >= 3 * sum(len(variants(n)) for n in NEEDLES)      # every variant stands in three haystacks and is a match in each
    for which in (1, 2):                                              # 1: only what passes the filter is verified; 2: every position is
        n, recs = chk.scan(img, which, hays)
        assert n >= 0
        assert expand_records(o.values_off(), o.values(), recs[0], recs[1], recs[2]) == exp, which
    # and each variant's suffix key, folded, is in the stored filter
    h = header(img.tobytes())
    f, lw = stored_filter(img.tobytes(), h), h["sf_bloom_log2_words"]
    for n in NEEDLES:
        for v in variants(n):
            t, k = folded(v)
            hh = bloom_hash(k, t)
            m = MASKS[(hh >> 2) & 511]
            assert int(f[hh >> (32 - lw)]) & m == m, (n, v)


def test_case_sensitive_filter_is_keyed_by_the_window_itself(chk):
    needles = NEEDLES + ["CAFÉ", "Kk", "\u212a\u212a", "ΩΩ", "\u2126", "@[\\]^", "`{|}~"]
    o = oracle.Machine(needles)
    img = chk.flatten(am.Automaton(needles), 0)
    h = header(img.tobytes())
    keys = image_keys(img.tobytes(), h)
    assert keys == {suffix_key(n.encode()) for n in needles}
    f, n = filter_of(keys, h["sf_bloom_log2_words"], False)          # g = identity
    assert n == len(keys) and np.array_equal(f, stored_filter(img.tobytes(), h))
    hays = needles + ["@[\\]^`{|}~@[\\]^", "cafÉ café CAFÉ", " ".join(needles)]
    exp = oracle_triples(o, 0, hays)
    n, recs = chk.scan(img, 1, hays)
    assert expand_records(o.values_off(), o.values(), recs[0], recs[1], recs[2]) == exp
