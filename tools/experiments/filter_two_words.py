"""CPU only: what k_sf's suffix filter would pass if every key set its mask in TWO words of the 2^15-word filter instead of one, where that filter is overloaded
(cfg3 and cfg4: 112 890 keys in 32 768 words, 3.4 keys per word).  A key sets one rotated mask m of 2, 3 or 4 bits in f[a1] and f[a2]; a window passes iff
(f[a1] & f[a2] & m) == m.  The k-bit table entry is bloom_mask_entry(i) of csrc/am_image.h WITHOUT ITS LAST-PLACED BITS: the first k of the four bits the
entry's loop places (k = 0 .. 3 of its 5-bit fields), so the 3-bit entry drops the bit placed from x[19:15] and the 2-bit entry that and the one from x[14:10].

With h = bloom_key(w) * kBloomMul, a1 = h >> 17, m = rotr32(mask_k[(h >> 2) & 511], (h >> 11) & 31), the second word's index is counted two ways:
    (a) a2 = a1 ^ ((h >> 2) & 0x7FFF)              no second multiply; its bits overlap the mask index and the rotation
    (b) a2 = (bloom_key(w) * 0x85EBCA6B) >> 17     an independent second multiply, the yardstick

The script flattens the workload's needles with the host flattener, reads the exact suffix keys back out of the image, rebuilds today's scan filter -- it must
reproduce the stored section bit for bit -- and counts positions passing per KiB on a MiB of text for every rule.

    python tools/experiments/filter_two_words.py [workload] [first_cell]

The gate of the two-word filter: fewer than 53 positions per KiB on cfg3 cells 0..1023 AND on cfg4 cells 500000..501023 (the same needles and case mode).
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import alfred_margaret_amd as am
from alfred_margaret_amd import synth
from filter_fold_keys import MASKS, fold_key, hashes, keys_by_tier
from filter_rotated_masks import rot
from tests.filter_keys import header
from tests.helpers import ImgCheck
from tests.scan_filter import ROT_SHIFT, stored_scan_filter

U = np.uint32
MUL2 = 0x85EBCA6B
GATE = 53.0


def mask_entry_k(i, nbits):
    """bloom_mask_entry of am_image.h, stopped after its first `nbits` bits"""
    x = ((i + 1) * 0x9E3779B1) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x85EBCA6B) & 0xFFFFFFFF; x ^= x >> 13; x = (x * 0xC2B2AE35) & 0xFFFFFFFF; x ^= x >> 16
    m = 0
    for k in range(nbits):
        b = (x >> (5 * k)) & 31
        while m & (1 << b):
            b = (b + 1) & 31
        m |= 1 << b
    return m


TABLES = {k: np.array([mask_entry_k(i, k) for i in range(512)], np.uint32) for k in (2, 3, 4)}
assert np.array_equal(TABLES[4], MASKS)


def mask_of(hh, nbits):
    return rot(TABLES[nbits][(hh >> U(2)) & U(511)], hh >> U(ROT_SHIFT))


def second_a(k, hh):
    return (hh >> U(17)) ^ ((hh >> U(2)) & U(0x7FFF))


def second_b(k, hh):
    return ((k.astype(np.uint64) * np.uint64(MUL2) & np.uint64(0xFFFFFFFF)) >> np.uint64(17)).astype(np.uint32)


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "cfg3_runLower_100k_10GiB"
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    w = synth.WORKLOADS[wl]
    needles = synth.needles_for(wl)
    img = ImgCheck().flatten(am.Automaton(needles), w["case"]).tobytes()
    h = header(img)
    lw, ic = h["sf_bloom_log2_words"], h["case_mode"] == 1
    keys = keys_by_tier(img, h)
    assert lw == 15 and set(keys) == {4}, "the two-word rule is for 2^15-word filters of 4-byte keys only"
    exact = keys[4]
    fk = np.unique(fold_key(exact, 4, ic))
    hk = hashes(fk, 4)
    a = synth.haystacks_host(needles, w["mixed"], first, 1024, natural=bool(w.get("natural"))).copy()
    if ic:
        up = (a >= 0x41) & (a <= 0x5A)
        a[up] += 0x20
    a = np.concatenate([np.zeros(3, np.uint8), a]).astype(np.uint32)
    win = (a[3:] << 24) | (a[2:-1] << 16) | (a[1:-2] << 8) | a[:-3]          # window ending at every position, newest byte on top (bytes before the text: 0)
    fw = fold_key(win, 4, ic)
    hw = hashes(fw, 4)
    real = np.isin(win, exact)
    kib = len(win) / 1024.0
    print("%s, image version %d, %s, cells %d..%d: %d needles, %d distinct filter keys in 2^%d words" % (
        wl, h["version"], "IgnoreCase" if ic else "CaseSensitive", first, first + 1024, len(needles), len(fk), lw))

    def report(name, p):
        assert not (real & ~p).any(), "a real suffix hit does not pass the filter"
        print("  %-46s: per KiB %6.2f positions pass: %.2f real suffix hits, %.2f false%s" % (
            name, p.sum() / kib, (p & real).sum() / kib, (p & ~real).sum() / kib, "" if p.sum() / kib >= GATE else "   < %.0f" % GATE))
        return p.sum() / kib

    f = np.zeros(1 << lw, np.uint32)
    np.bitwise_or.at(f, hk >> U(17), mask_of(hk, 4))
    assert np.array_equal(f, stored_scan_filter(img, h)), "the keys read from the image do not reproduce its scan filter"
    m = mask_of(hw, 4)
    report("one word, 4 bits (scan filter, reproduced)", (f[hw >> U(17)] & m) == m)
    for nbits in (2, 3, 4):
        f = np.zeros(1 << lw, np.uint32)
        np.bitwise_or.at(f, hk >> U(17), mask_of(hk, nbits))
        m = mask_of(hw, nbits)
        report("one word, %d bits" % nbits, (f[hw >> U(17)] & m) == m)
    for nbits in (2, 3, 4):
        for tag, second in (("(a) a2 = a1 ^ h[16:2]", second_a), ("(b) second multiply", second_b)):
            f = np.zeros(1 << lw, np.uint32)
            mk = mask_of(hk, nbits)
            np.bitwise_or.at(f, hk >> U(17), mk)
            np.bitwise_or.at(f, second(fk, hk), mk)
            m = mask_of(hw, nbits)
            report("two words, %d bits, %s" % (nbits, tag), (f[hw >> U(17)] & f[second(fw, hw)] & m) == m)


if __name__ == "__main__":
    main()
