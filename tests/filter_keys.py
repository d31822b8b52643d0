"""The suffix filter of a flattened image, restated in Python for the tests and for tools/experiments/filter_fold_keys.py: the header fields up to off_goto, the exact
suffix keys read back out of the tier tables and the cold cuckoo slots, and bloom_key / bloom_hash / bloom_mask_entry of csrc/am_image.h.  One place to edit when the
header or the hash changes."""
import struct

import numpy as np

MUL, SALT = 0x9E3779B1, 0x7F4A7C15
HDR = struct.Struct("<4IQ4I" + "7Q" + "2I" + "4I" + "Q" + "4Q" + "4I" + "8Q")
NAMES = ["magic", "version", "case_mode", "flags", "total_bytes", "n_states", "max_needle_cps", "root_vlen", "ac_chunk",
         "off_transitions", "n_transitions", "off_offsets", "off_root_ascii", "off_canon", "off_vlen", "off_lower",
         "n_lower", "sf_enabled", "sf_tiers", "sf_bloom_log2_words", "sf_n_nodes", "ac_goto_log2_cap",
         "off_bloom", "off_tier0", "off_tier1", "off_tier2", "off_tier3", "cap0", "cap1", "cap2", "cap3",
         "off_nodes", "off_edges", "n_edges", "off_edge_maps", "n_edge_maps", "off_t4_slots", "checksum", "off_goto"]

def mask_entry(i):
    """bloom_mask_entry of am_image.h"""
    x = ((i + 1) * 0x9E3779B1) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x85EBCA6B) & 0xFFFFFFFF; x ^= x >> 13; x = (x * 0xC2B2AE35) & 0xFFFFFFFF; x ^= x >> 16
    m = 0
    for k in range(4):
        b = (x >> (5 * k)) & 31
        while m & (1 << b):
            b = (b + 1) & 31
        m |= 1 << b
    return m


MASKS = [mask_entry(i) for i in range(512)]


def bloom_hash(key, tier):
    return ((key + (4 - tier) * SALT) * MUL) & 0xFFFFFFFF


def tier_key(key, tier, fold):
    """bloom_tier_key of am_image.h: a key of `tier` bytes, modulo the ASCII case bit when `fold`"""
    return key | (0x20202020 >> (8 * (4 - tier))) if fold else key


def header(img):
    return dict(zip(NAMES, HDR.unpack_from(img)))


def image_keys(img, h):
    """{(tier, exact key)} of an image: tiers 1-3 from their open-addressing tables, tier 4 from the cold slots (SfSlot: key, flags, ...; 64 bytes)"""
    keys = set()
    for t in range(3):
        if h["sf_tiers"] & (1 << t):
            tab = np.frombuffer(img, np.uint32, 2 << h["cap%d" % t], h["off_tier%d" % t]).reshape(-1, 2)
            keys |= {(t + 1, int(k)) for k in tab[tab[:, 1] != 0xFFFFFFFF, 0]}
    if h["sf_tiers"] & 8:
        slots = np.frombuffer(img, np.uint32, (2 << h["cap3"]) * 16, h["off_t4_slots"]).reshape(-1, 16)
        keys |= {(4, int(k)) for k in slots[(slots[:, 1] & 1) != 0, 0]}
    return keys


def filter_of(keys, lw, fold):
    """(filter words, distinct filter keys) of a set of (tier, exact key)"""
    fkeys = {(t, tier_key(k, t, fold)) for t, k in keys}
    f = np.zeros(1 << lw, np.uint32)
    for t, k in fkeys:
        hh = bloom_hash(k, t)
        f[hh >> (32 - lw)] |= MASKS[(hh >> 2) & 511]
    return f, len(fkeys)


def stored_filter(img, h):
    return np.frombuffer(img, np.uint32, 1 << h["sf_bloom_log2_words"], h["off_bloom"])


def log2_words(n_keys):
    """the flattener's sizing rule: two keys per word, 2^8 .. 2^15 words"""
    n = (n_keys * 16 + 31) // 32
    lw = 0
    while (1 << lw) < n:
        lw += 1
    return max(8, min(15, lw))
