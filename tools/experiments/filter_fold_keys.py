"""CPU only: what k_sf's suffix filter passes when an IgnoreCase image keys it by the 4-byte window MODULO THE ASCII CASE BIT (w | 0x20202020, bloom_key in
csrc/am_image.h) instead of by the exact folded window.  The flattener bakes the case variants of non-ASCII code points into the suffix tables (É next to é,
А next to а); many of those pairs differ in bit 5 of one byte only and become one filter key.

The script flattens a workload's needles with the host flattener, reads the exact suffix keys back out of the image (tier tables and the cold cuckoo slots),
rebuilds the filter both ways with the kernel's own hash and masks -- the way the image's version uses must reproduce the image's filter bit for bit -- and
counts what each passes on a MiB of the workload's text: distinct keys, fill, positions per KiB split into real suffix hits and false positives.

    python tools/experiments/filter_fold_keys.py [workload] [first_cell]
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import alfred_margaret_amd as am
from alfred_margaret_amd import synth
from tests.filter_keys import MASKS as _MASKS, MUL, SALT, header, image_keys
from tests.helpers import ImgCheck

FOLDED_SINCE = 18                        # image version from which IgnoreCase filters hold folded keys
MASKS = np.array(_MASKS, dtype=np.uint32)


def keys_by_tier(img, h):
    """{tier: exact keys as an array} of an image"""
    out = {}
    for t, k in image_keys(img, h):
        out.setdefault(t, []).append(k)
    return {t: np.unique(np.array(k, np.uint32)) for t, k in out.items()}


def fold_key(k, tier, on):
    """bloom_tier_key of am_image.h on an array of keys of `tier` bytes"""
    return k | np.uint32(0x20202020 >> (8 * (4 - tier))) if on else k


def hashes(k, tier):
    return ((k.astype(np.uint64) + np.uint64(((4 - tier) * SALT) & 0xFFFFFFFF)) * np.uint64(MUL) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def make_filter(keys, lw, on):
    f = np.zeros(1 << lw, np.uint32)
    n = 0
    for t, k in keys.items():
        k = np.unique(fold_key(k, t, on))
        n += len(k)
        hh = hashes(k, t)
        np.bitwise_or.at(f, hh >> np.uint32(32 - lw), MASKS[(hh >> np.uint32(2)) & np.uint32(511)])
    return f, n


def passes(f, lw, keys, win, on):
    """per position: passes the filter, and is a real suffix hit (the exact window is a key)"""
    p, real = np.zeros(len(win), bool), np.zeros(len(win), bool)
    for t, k in keys.items():
        wt = win >> np.uint32(8 * (4 - t))
        hh = hashes(fold_key(wt, t, on), t)
        m = MASKS[(hh >> np.uint32(2)) & np.uint32(511)]
        p |= (f[hh >> np.uint32(32 - lw)] & m) == m
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
    stored = np.frombuffer(img, np.uint32, 1 << lw, h["off_bloom"])
    own, _ = make_filter(keys, lw, ic and h["version"] >= FOLDED_SINCE)
    assert np.array_equal(own, stored), "the keys read from the image do not reproduce its filter"
    a = synth.haystacks_host(needles, w["mixed"], first, 1024, natural=bool(w.get("natural"))).copy()
    if ic:
        up = (a >= 0x41) & (a <= 0x5A)
        a[up] += 0x20
    a = np.concatenate([np.zeros(3, np.uint8), a]).astype(np.uint32)
    win = (a[3:] << 24) | (a[2:-1] << 16) | (a[1:-2] << 8) | a[:-3]          # window ending at every position, newest byte on top (bytes before the text: 0)
    kib = len(win) / 1024.0
    print("%s, image version %d, %s, cells %d..%d: %d needles, filter of 2^%d words" % (wl, h["version"], "IgnoreCase" if ic else "CaseSensitive", first, first + 1024, len(needles), lw))
    for name, on in (("exact keys", False), ("keys | 0x20", True)):
        if on and not ic: break
        f, n = make_filter(keys, lw, on)
        p, real = passes(f, lw, keys, win, on)
        fill = float(np.unpackbits(f.view(np.uint8)).mean())
        print("  %-11s: %6d distinct keys (%.2f bits per key), fill %.4f (fill^4 %.4f); per KiB %.1f positions pass: %.1f real suffix hits, %.1f false" % (
            name, n, 32.0 * (1 << lw) / max(n, 1), fill, fill ** 4, p.sum() / kib, (p & real).sum() / kib, (p & ~real).sum() / kib))
        assert not (real & ~p).any(), "a real suffix hit does not pass the filter"


if __name__ == "__main__":
    main()
