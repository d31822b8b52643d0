"""CPU only: what k_sf's suffix filter passes when every key's table mask is ROTATED by five more bits of its hash (scan_mask in csrc/am_image.h, the scan
filter of image version 19) instead of being one of the 512 table masks as it is (the filter at off_bloom).  With 512 masks a text window that lands in the
word of a key with the same mask passes outright; the rotation makes 16 384 masks out of the same table.

The script flattens a workload's needles with the host flattener, reads the exact suffix keys back out of the image, rebuilds BOTH stored sections with the
kernel's own hash -- each must reproduce its section bit for bit -- and counts what each rule passes on a MiB of the workload's text: positions per KiB, split
into real suffix hits and false positives.  The other (mask index, rotation) assignments that were weighed are counted next to them.

    python tools/experiments/filter_rotated_masks.py [workload] [first_cell]
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import alfred_margaret_amd as am
from alfred_margaret_amd import synth
from filter_fold_keys import MASKS, fold_key, hashes, keys_by_tier
from tests.filter_keys import header
from tests.helpers import ImgCheck
from tests.scan_filter import ROT_SHIFT, stored_scan_filter

U = np.uint32


def rot(m, r):
    """rotr32 of am_image.h on arrays; like v_alignbit_b32 it reads the low five bits of r"""
    r = r & U(31)
    return ((m >> r) | (m << ((U(32) - r) & U(31)))).astype(np.uint32)


def table(shift):
    return lambda h: MASKS[(h >> U(shift)) & U(511)]


# name -> mask of an array of hashes; the first two are the image's sections
RULES = [
    ("shipped: idx = h[10:2]", table(2)),
    ("idx = h[10:2], r = h[%d:%d] (scan filter)" % (ROT_SHIFT + 4, ROT_SHIFT), lambda h: rot(table(2)(h), h >> U(ROT_SHIFT))),
    ("idx = h[16:8], no rotation", table(8)),
    ("idx = h[16:8], r = h[4:0]", lambda h: rot(table(8)(h), h)),
    ("idx = h[16:8], r = h[7:3]", lambda h: rot(table(8)(h), h >> U(3))),
]


def make_filter(keys, lw, fold, mask_of):
    f = np.zeros(1 << lw, np.uint32)
    for t, k in keys.items():
        hh = hashes(np.unique(fold_key(k, t, fold)), t)
        np.bitwise_or.at(f, hh >> U(32 - lw), mask_of(hh))
    return f


def passes(f, lw, keys, win, fold, mask_of):
    """per position: passes the filter, and is a real suffix hit (the exact window is a key)"""
    p, real = np.zeros(len(win), bool), np.zeros(len(win), bool)
    for t, k in keys.items():
        wt = win >> U(8 * (4 - t))
        hh = hashes(fold_key(wt, t, fold), t)
        m = mask_of(hh)
        p |= (f[hh >> U(32 - lw)] & m) == m
        real |= np.isin(wt, k)
    return p, real


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "cfg3_runLower_100k_10GiB"
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    w = synth.WORKLOADS[wl]
    needles = synth.needles_for(wl)
    img = ImgCheck().flatten(am.Automaton(needles), w["case"]).tobytes()
    h = header(img)
    lw, ic = h["sf_bloom_log2_words"], h["case_mode"] == 1
    keys = keys_by_tier(img, h)
    assert np.array_equal(make_filter(keys, lw, ic, RULES[0][1]), np.frombuffer(img, np.uint32, 1 << lw, h["off_bloom"])), "the keys read from the image do not reproduce its filter"
    assert np.array_equal(make_filter(keys, lw, ic, RULES[1][1]), stored_scan_filter(img, h)), "the keys read from the image do not reproduce its scan filter"
    a = synth.haystacks_host(needles, w["mixed"], first, 1024, natural=bool(w.get("natural"))).copy()
    if ic:
        up = (a >= 0x41) & (a <= 0x5A)
        a[up] += 0x20
    a = np.concatenate([np.zeros(3, np.uint8), a]).astype(np.uint32)
    win = (a[3:] << 24) | (a[2:-1] << 16) | (a[1:-2] << 8) | a[:-3]          # window ending at every position, newest byte on top (bytes before the text: 0)
    kib = len(win) / 1024.0
    print("%s, image version %d, %s, cells %d..%d: %d needles, filter of 2^%d words, both sections reproduced" % (
        wl, h["version"], "IgnoreCase" if ic else "CaseSensitive", first, first + 1024, len(needles), lw))
    for name, mask_of in RULES:
        f = make_filter(keys, lw, ic, mask_of)
        p, real = passes(f, lw, keys, win, ic, mask_of)
        assert not (real & ~p).any(), "a real suffix hit does not pass the filter"
        print("  %-44s: per KiB %6.2f positions pass: %.2f real suffix hits, %.2f false" % (name, p.sum() / kib, (p & real).sum() / kib, (p & ~real).sum() / kib))


if __name__ == "__main__":
    main()
