"""The SCAN filter of a flattened image (image version 19, ImageHeader::off_scan_bloom), restated in Python for the tests and for
tools/experiments/filter_rotated_masks.py: the keys and the hash of tests/filter_keys.py, each key's table mask rotated right by product bits 11..15 (scan_mask of
csrc/am_image.h).  k_sf alone reads this section; the filter at off_bloom keeps the unrotated rule (tests/filter_keys.filter_of).  One place to edit when the
rotation changes."""
import struct

import numpy as np

from tests.filter_keys import MASKS, bloom_hash, tier_key

OFF_SCAN_BLOOM = 352          # byte offset of ImageHeader::off_scan_bloom: the first field behind off_dfa_chain2
ROT_SHIFT = 11                # kScanRotShift


def rotr32(m, r):
    """rotr32 of am_image.h, written the same way: r in 0..31"""
    return ((m >> r) | (m << ((32 - r) & 31))) & 0xFFFFFFFF


def scan_rot(hh):
    return (hh >> ROT_SHIFT) & 31


def scan_mask(hh):
    return rotr32(MASKS[(hh >> 2) & 511], scan_rot(hh))


def scan_filter_of(keys, lw, fold):
    """the scan filter's words of a set of (tier, exact key)"""
    f = np.zeros(1 << lw, np.uint32)
    for t, k in {(t, tier_key(k, t, fold)) for t, k in keys}:
        hh = bloom_hash(k, t)
        f[hh >> (32 - lw)] |= scan_mask(hh)
    return f


def off_scan_bloom(img):
    return struct.unpack_from("<Q", img, OFF_SCAN_BLOOM)[0]


def stored_scan_filter(img, h):
    return np.frombuffer(img, np.uint32, 1 << h["sf_bloom_log2_words"], off_scan_bloom(img))
