"""Texts for k_sf's straight path (csrc/am_kernels.hip: the round's bucket request that every chunk issues, survivors or not, and the latch that waits for the
prefetched chunk alone).  Built from tests/sf_chunk_cases.py's filler and run: a chunk "with n survivors" has exactly n positions that pass the filter.  Shared by
tests/test_sf_latch_cpu.py (the host model's count of every chunk, the oracle's records) and tests/test_gpu_sf_latch.py (the kernels).

A batch is `total` bytes cut into work units of `uc` chunks (what the launcher would choose: api.sf_unit_chunks on the device, any value on the host).  One unit
holds one pattern, units without one hold filler only -- so "all zero" units lie between all the others:
  zeros      survivors N in the chunks of 0,N,0 / N,0,0,N, as the first chunks of the batch and of a unit, as the last chunks of a unit and of the batch, and across
             the end of a ring epoch (chunks 14..17 of a unit, where the unit is that long)
  limits     1, 63, 64, 65, 127, 128, 129 and 257 survivors in one chunk, followed by a chunk with 0 and (in another unit) by one with 64
  seam       a haystack that ends in the middle of a chunk, survivors on both sides of the seam, a chunk with N before it and one after it
The batch ends with a partial chunk of `total % 1024` bytes whose last four bytes are the run (a match on the batch's last byte) when there are that many."""
import numpy as np

from tests import sf_chunk_cases as cc

CHUNK = cc.CHUNK
N = 5                                                 # survivors of a pattern's non-empty chunks
LIMITS = (1, 63, 64, 65, 127, 128, 129, 257)
EPOCH = 16


def patterns(uc):
    """[(name, {chunk within the unit: survivors})] -- one unit each, in the order they are laid out; what does not fit a unit of uc chunks is left out"""
    out = []
    if uc >= 3:
        out += [("0,N,0 first", {0: 0, 1: N, 2: 0}), ("0,N,0 last", {uc - 3: 0, uc - 2: N, uc - 1: 0})]
    if uc >= 4:
        out += [("N,0,0,N first", {0: N, 1: 0, 2: 0, 3: N}), ("N,0,0,N last", {uc - 4: N, uc - 3: 0, uc - 2: 0, uc - 1: N})]
    if uc >= EPOCH + 2:
        out += [("N,0,0,N epoch", {EPOCH - 2: N, EPOCH - 1: 0, EPOCH: 0, EPOCH + 1: N}), ("0,N,0 epoch", {EPOCH - 2: 0, EPOCH - 1: N, EPOCH: 0}),
                ("N first of epoch", {EPOCH - 1: 0, EPOCH: N, EPOCH + 1: 0})]
    if uc >= 2:
        for m in LIMITS:
            out += [("%d then 0" % m, {uc - 2: m, uc - 1: 0}), ("%d then 64" % m, {0: m, 1: 64})]
    else:
        out += [("%d alone" % m, {0: m}) for m in LIMITS]
    return out


def latch_batch(fill, case, total, uc):
    """(text, offsets, {chunk: survivors it must have}): see the module's docstring.  Haystacks: one per used unit (so every pattern's candidates lie inside one
    haystack that starts at the unit's first byte), the seam's two, and the rest of the batch in three."""
    n_chunks = (total + CHUNK - 1) // CHUNK
    n_units = (n_chunks + uc - 1) // uc
    text = bytearray(fill * total)
    placed, cuts = {}, {0, total}
    pats = patterns(uc)
    # the batch's first unit takes the first pattern ("0,N,0 first" where it fits), every other pattern a unit of its own with an all-filler unit between
    units = [0] + [1 + 2 * i for i in range(1, len(pats))]
    assert units[-1] + 4 < n_units, (total, uc, len(pats))
    for u, (_, chunks) in zip(units, pats):
        cuts.add(u * uc * CHUNK)
        for c, n in chunks.items():
            placed[u * uc + c] = cc.put(text, u * uc + c, fill, case, n)
    # the seam: unit su, chunks 0..2 (or the one chunk of a one-chunk unit): N | 3 before the seam at +512 and 4 behind it | N
    su = units[-1] + 2
    base = su * uc
    cuts.add(base * CHUNK)
    seam_chunk = base + (1 if uc >= 3 else 0)
    if uc >= 3:
        placed[base] = cc.put(text, base, fill, case, N)
        placed[base + 2] = cc.put(text, base + 2, fill, case, N)
    at = seam_chunk * CHUNK
    text[at + 100:at + 106] = cc.run(6, case)            # three whole windows before the seam ...
    text[at + 512:at + 519] = cc.run(7, case)            # ... and four behind it (the first three windows of this run begin in the haystack before: candidates, no matches)
    text[at + 509:at + 512] = cc.run(3, case, 1)         # (the run goes on across the seam: 3 + 7 bytes, seven windows, of which four lie inside the second haystack)
    placed[seam_chunk] = 3 + 7
    cuts.add(at + 512)
    # the batch's last unit: 0,N,0 before the partial chunk (where the unit has room), the run on the batch's last four bytes
    last = n_chunks - 1
    r = total - last * CHUNK
    if last - 3 > (su + 1) * uc:
        placed[last - 3], placed[last - 2], placed[last - 1] = 0, cc.put(text, last - 2, fill, case, N), 0
    if r >= 4:
        text[total - 4:total] = cc.run(4, case)
        placed[last] = 1
    rest_from = (su + 1) * uc * CHUNK
    third = (total - rest_from) // 3
    cuts |= {rest_from, rest_from + third, rest_from + 2 * third}
    offs = sorted(cuts)
    return bytes(text), np.asarray(offs, np.int64), placed


def expected_matches(placed, uc):
    """matches the oracle must find: every survivor is a match except the seam's three windows that begin before the seam"""
    return sum(placed.values()) - 3


# ---- <ILP 2, LW 0> without child entries: a suffix table beyond 2^15 buckets (more than 49 152 distinct 4-byte suffixes) behind a filter below 2^15 words (at most
# 32 768 distinct FILTER keys).  Under CaseSensitive a suffix is its own filter key, so no image has both; under IgnoreCase the filter hashes the bytes modulo the
# ASCII case bit, which the fold leaves alone in bytes that are no letters: all 4-byte strings over eight pairs of such bytes are 65 536 suffixes on 4 096 filter keys.
PAIRS = "@`[{\\|]}^~0\x101\x112\x12"


def ilp2_lw0_needles():
    import itertools
    return ["".join(t) for t in itertools.product(PAIRS, repeat=4)]


# ---- a needle whose hot entry lies in bucket 0 of the suffix table (am_image.h: t4_hash_a, t4_bucket), the bucket every lane without a probe of its own reads
def t4_bucket_a(word, log2_buckets):
    key = int.from_bytes(word.encode()[-4:], "little")
    return ((key * 0x85EBCA6B) & 0xFFFFFFFF) >> (32 - log2_buckets)


def t4_bucket_b(word, log2_buckets):
    key = int.from_bytes(word.encode()[-4:], "little")
    return (((key ^ (key >> 15)) * 0xC2B2AE35) & 0xFFFFFFFF) >> (32 - log2_buckets)


def bucket0_word(log2_buckets=2):
    """the first four-letter word (a fixed order, no z) BOTH of whose buckets are bucket 0: wherever the cuckoo placement puts its entry, it is in bucket 0"""
    import itertools
    for t in itertools.product("bcdfghjklmnpqrstvwx", repeat=4):
        w = "".join(t)
        if t4_bucket_a(w, log2_buckets) == 0 and t4_bucket_b(w, log2_buckets) == 0:
            return w
    raise AssertionError("no such word")


def bucket0_batch(fill, word, total, straddle):
    """(text, offsets, matches): `word` on the last three bytes of chunk 4 and the first of chunk 5 -- chunk 5's only survivor, at offset 0, the offset every lane
    WITHOUT a survivor computes its window from, so that all 63 of them expect exactly the entry that lies in bucket 0 --; and `word` across a haystack's start in
    chunk 9, `straddle` (1..3) of its bytes in the haystack before: a survivor whose window does not fit (avail < 4: no probe of its own either), no match."""
    text = bytearray(fill * total)
    w = word.encode()
    text[5 * CHUNK - 3:5 * CHUNK + 1] = w
    hs = 9 * CHUNK + 300
    text[hs - straddle:hs - straddle + 4] = w
    return bytes(text), np.asarray([0, hs, total], np.int64), 1
