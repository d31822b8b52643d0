"""The TWO-WORD scan filter (scan2_mask / scan2_derive in csrc/am_image.h and csrc/am_flatten.cpp), restated in Python for the tests: derived data that is no part of
the image.  An image gets one iff its filter has 2^15 words, it has no needle (variant) shorter than 4 bytes and more than 3 * 2^15 distinct tier-4 filter keys.
A key sets a 3-bit mask -- its table entry without the bit placed last, rotated like the scan filter's -- in two words: a1 = h >> 17 and a2 = a1 ^ h[16:2]; a
window passes iff both words hold its mask.  One place to edit when the rule changes."""
import numpy as np

from tests.filter_keys import bloom_hash, tier_key
from tests.scan_filter import rotr32, scan_rot

BITS = 3
LOG2_WORDS = 15
MIN_KEYS = 3 << LOG2_WORDS          # the rule holds for MORE distinct filter keys than this


def mask_entry_n(i, nbits):
    """bloom_mask_entry(i, nbits) of am_image.h: the first nbits bits of table entry i"""
    x = ((i + 1) * 0x9E3779B1) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x85EBCA6B) & 0xFFFFFFFF; x ^= x >> 13; x = (x * 0xC2B2AE35) & 0xFFFFFFFF; x ^= x >> 16
    m = 0
    for k in range(nbits):
        b = (x >> (5 * k)) & 31
        while m & (1 << b):
            b = (b + 1) & 31
        m |= 1 << b
    return m


MASKS3 = [mask_entry_n(i, BITS) for i in range(512)]


def word1(hh):
    return hh >> (32 - LOG2_WORDS)


def word2(hh):
    return word1(hh) ^ ((hh >> 2) & ((1 << LOG2_WORDS) - 1))


def scan2_mask(hh):
    return rotr32(MASKS3[(hh >> 2) & 511], scan_rot(hh))


def applies(h, keys, fold):
    """does an image with header h and exact keys `keys` ({(tier, key)}) get the derived filter?"""
    return h["sf_bloom_log2_words"] == LOG2_WORDS and (h["sf_tiers"] & 7) == 0 and len({tier_key(k, t, fold) for t, k in keys if t == 4}) > MIN_KEYS


def scan2_filter_of(keys, fold):
    """the derived words of a set of (tier, exact key), tier 4 only"""
    f = np.zeros(1 << LOG2_WORDS, np.uint32)
    for k in {tier_key(k, t, fold) for t, k in keys if t == 4}:
        hh = bloom_hash(k, 4)
        m = scan2_mask(hh)
        f[word1(hh)] |= m
        f[word2(hh)] |= m
    return f


def derived_words(chk, img):
    """amflat_scan2_filter (csrc/am_flatten.cpp) through libam_imgcheck.so (chk: tests/helpers.ImgCheck): the words scan2_derive -- the routine of every upload path --
    gives for a flattened image, or None where the rule does not apply to it"""
    import ctypes as C
    img = bytes(img)
    out = np.zeros(1 << LOG2_WORDS, np.uint32)
    chk.lib.amflat_scan2_filter.restype = C.c_longlong
    n = chk.lib.amflat_scan2_filter(C.c_char_p(img), C.c_size_t(len(img)), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size))
    assert n in (0, out.size), n
    return out if n else None


def passes(f, key):
    """does the filter key (a folded window) pass the two-word filter f?"""
    hh = bloom_hash(key, 4)
    m = scan2_mask(hh)
    return int(f[word1(hh)]) & int(f[word2(hh)]) & m == m


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The needle sets and texts of tests/test_scan2_filter_cpu.py and tests/test_gpu_scan2_filter.py.  Lower-case ASCII words (and SAME_WORD, which has no case
# variant either): a set has as many distinct filter keys as it has words, in either case mode.

_CACHE = {}


def key_of(word):
    return int.from_bytes(word.encode()[-4:], "little")


# A key whose two filter words are the SAME word has h[16:2] == 0, i.e. h mod 2^17 in 0..3: its two oldest bytes are 00 00, 51 2F, A2 5E or F3 8D (times the
# multiplier's inverse), and bit 0 of the third is fixed.  A2 5E 62 62 is the tail of this word.  No IgnoreCase key can be one -- bit 5 is set in all of its bytes and
# in none of the four pairs -- so under IgnoreCase the word is a key like any other (A2 7E 62 62).
SAME_WORD = "\u00a2^bb"


def searched_words(taken):
    """SAME_WORD, and five-letter words, taken in a fixed order, whose suffix is not in `taken`: the first whose mask is rotated by 0 and the first rotated by 31 --
    the ends where a wrong address or shift shows."""
    import itertools
    out = {"same word": SAME_WORD}
    for letters in itertools.product("bcdfghjlmnpqrtvwxz", repeat=5):
        w = "".join(letters)
        if w[-4:] in taken:
            continue
        r = scan_rot(bloom_hash(key_of(w), 4))
        for name, hit in (("rotation 0", r == 0), ("rotation 31", r == 31)):
            if hit and name not in out:
                out[name] = w
        if len(out) == 3:
            return out
    raise AssertionError("no such words")


def needle_sets():
    """name -> needles.  `threshold` has exactly MIN_KEYS distinct suffix keys and gets no derived filter; `large` is it plus the three searched_words."""
    if "sets" not in _CACHE:
        from tests.test_scan_filter_cpu import words
        base = words("scan2-threshold", MIN_KEYS)
        extra = searched_words({w[-4:] for w in base})
        _CACHE["extra"] = extra
        _CACHE["sets"] = {"threshold": base, "large": base + list(extra.values()), "60000": base[:60000], "large + a 2-byte needle": base + list(extra.values()) + ["q7"]}
    return _CACHE["sets"]


def searched():
    needle_sets()
    return _CACHE["extra"]


def rejected_window(needles, fold):
    """Four letters that are no needle's suffix, pass the one-word scan filter of `needles` and fail the two-word one: what the derived filter is for."""
    if ("reject", fold) not in _CACHE:
        import itertools
        from tests.scan_filter import scan_filter_of, scan_mask
        keys = {(4, key_of(w)) for w in needles}
        fkeys = {tier_key(k, 4, fold) for _, k in keys}
        one, two = scan_filter_of(keys, LOG2_WORDS, fold), scan2_filter_of(keys, fold)
        for letters in itertools.product("abcdefghjlmnopqrtuvwxyz", repeat=4):
            w = "".join(letters)
            k = key_of(w)                      # (lower-case letters: its own filter key under either mode)
            hh = bloom_hash(k, 4)
            if k not in fkeys and int(one[word1(hh)]) & scan_mask(hh) == scan_mask(hh) and not passes(two, k):
                _CACHE[("reject", fold)] = w
                break
    return _CACHE[("reject", fold)]


def make_text(needles, n_bytes, case, seed, first=()):
    """n_bytes of ASCII: the strings of `first`, then about 35 % verbatim needles (IgnoreCase: letters upper-cased at random), 25 % near misses (one letter changed, in
    the last four bytes or before them), the rest filler."""
    import random
    rng = random.Random("scan2-text-%d-%d-%d" % (n_bytes, case, seed))
    az = "abcdefghjlmnopqrtuvwxyz"
    parts, at = [], 0
    for p in first:
        parts.append(p + " "); at += len(p) + 1
    while at < n_bytes:
        r = rng.random()
        if r < 0.35:
            p = rng.choice(needles)
            if case and rng.random() < 0.5:
                p = "".join(c.upper() if rng.random() < 0.4 else c for c in p)
        elif r < 0.60:
            p = list(rng.choice(needles))
            i = rng.randrange(len(p) - 4, len(p)) if len(p) == 4 or rng.random() < 0.5 else rng.randrange(0, len(p) - 4)
            p[i] = "b" if p[i] != "b" else "c"
            p = "".join(p)
        else:
            p = "".join(rng.choice(az + " ,.#") for _ in range(rng.randint(1, 24)))
        parts.append(p); at += len(p)
    return "".join(parts).encode()[:n_bytes]


def cut(text, seed, n_cuts=24):
    """offsets (np.int64) of haystacks over `text`: random cuts, cuts at multiples of 1 024 +- 1, one empty haystack"""
    import random
    rng = random.Random("scan2-cuts-%d-%d" % (len(text), seed))
    cuts = {0, len(text)} | {rng.randrange(1, len(text)) for _ in range(n_cuts)}
    cuts |= {k * 1024 + d for k in rng.sample(range(1, max(2, len(text) // 1024)), min(6, max(1, len(text) // 1024 - 1))) for d in (-1, 1) if 0 < k * 1024 + d < len(text)}
    offs = sorted(cuts)
    return np.asarray(offs[:3] + [offs[2]] + offs[3:], dtype=np.int64)
