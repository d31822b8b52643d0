"""Texts at the limits of k_sf's chunk loop (csrc/am_kernels.hip), and the host model of its filter stage that says what they exercise.  Shared by
tests/test_sf_chunk_loop_cpu.py (the model's counts and the oracle's records on these texts, CPU only) and tests/test_gpu_sf_chunk_loop.py (the kernels).

The loop, per 1-KiB chunk: every position whose 4-byte window (and, with short needles, its 1..3-byte tails) passes the scan filter is a CANDIDATE; the candidates
are compacted into a queue of kSfQ1 = 128 positions per sub-pass; a probe round reads two queue entries per lane (64 lanes) and three dwords of the staged chunk
for each.  So the shapes are: the number of candidates of ONE chunk around 64 (one entry per lane | two), 128 (one sub-pass | two, with the first sub-pass's
entries stale behind the second's) and 256, the position of a single candidate inside its lane's 16 bytes, the end of the batch inside a lane's 16 bytes, and the
start of the candidate's haystack 0..5 bytes before its chunk.

Everything is built from a FILLER byte on which the filter passes no position and a RUN of the byte z (needle "zzzz": every window inside a run is a match, a
run of n + 3 bytes gives n candidates in a row); the model counts, the builders assert."""
import numpy as np

from tests.filter_keys import MASKS, MUL, SALT, header
from tests.helpers import sf_family_needles
from tests.scan_filter import ROT_SHIFT, stored_scan_filter

CHUNK = 1024
RUN = "zzzz"
FAMILIES = ("small", "mid", "large", "mid+short", "dict")      # <ILP 1, LW 0>, <ILP 1, LW 15>, <ILP 2, LW 15>, SHORT, CHILDREN (tests/test_sf_variants_cpu.PURPOSE)
QUEUE_NS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257)    # candidates of the chunk; "every" = all 1 024 positions
BIT_LANES = (0, 1, 31, 62, 63)
HAY_INTO = (0, 1, 2, 3, 4, 5)                                  # c0 - hs0: bytes of the haystack before the chunk that holds its first candidates
_MASKS = np.asarray(MASKS, dtype=np.uint64)
_M32 = np.uint64(0xFFFFFFFF)


def needles_of(family):
    return sf_family_needles(family) + [RUN]


class FilterModel:
    """Which positions of a batch's text k_sf's filter stage passes: the 4-byte window that ends at the position (bytes before the batch: zero) against the image's
    scan filter, and the window's top 1..3 bytes for every short tier the image has (sf_filter_short)."""

    def __init__(self, img, case):
        h = header(img)
        assert h["case_mode"] == case
        self.lw, self.tiers, self.fold = h["sf_bloom_log2_words"], h["sf_tiers"], case == 1
        self.filt = stored_scan_filter(img, h).astype(np.uint64)

    def _hit(self, hh):
        v, m, r = self.filt[hh >> np.uint64(32 - self.lw)], _MASKS[(hh >> np.uint64(2)) & np.uint64(511)], (hh >> np.uint64(ROT_SHIFT)) & np.uint64(31)
        mr = ((m >> r) | (m << ((np.uint64(32) - r) & np.uint64(31)))) & _M32
        return (v & mr) == mr

    def passing(self, text):
        b = np.concatenate([np.zeros(3, np.uint64), np.frombuffer(bytes(text), np.uint8).astype(np.uint64)])
        n = len(b) - 3
        w = b[0:n] | (b[1:n + 1] << np.uint64(8)) | (b[2:n + 2] << np.uint64(16)) | (b[3:n + 3] << np.uint64(24))
        if self.fold:
            w = w | np.uint64(0x20202020)
        hit = self._hit((w * np.uint64(MUL)) & _M32)
        for t in (1, 2, 3):
            if self.tiers & (1 << (t - 1)):
                hit |= self._hit((((w >> np.uint64(8 * (4 - t))) + np.uint64(((4 - t) * SALT) & 0xFFFFFFFF)) * np.uint64(MUL)) & _M32)
        return hit

    def per_chunk(self, text):
        p = self.passing(text)
        return np.add.reduceat(p.astype(np.int64), np.arange(0, len(p), CHUNK)) if len(p) else np.zeros(0, np.int64)


def run(n, case, phase=0):
    """n bytes of the run; under IgnoreCase z and Z alternate"""
    return (b"zZ" * (n // 2 + 2))[phase & 1:(phase & 1) + n] if case else b"z" * n


def filler_of(model, case):
    """The first byte of a fixed list on which the filter passes nothing, next to a run either: eight of it, a run of eight, eight of it pass exactly the run's five
    whole windows (and so do the same bytes at the start of a batch, behind three zero bytes)."""
    for c in b"_-#=+;:%&":
        f = bytes([c])
        p = model.passing(f * 8 + run(8, case) + f * 8)
        if p.sum() == 5 and p[11:16].all() and not model.passing(f * 64).any():
            return f
    raise AssertionError("no filler byte for this filter")


def chunk_with(fill, case, n):
    """1 024 bytes with n candidates (a run of n + 3 bytes from offset 8) between filler; n = "every": the run fills the chunk -- its first three positions are
    candidates when the three bytes before the chunk belong to the run too (lead())."""
    if n == "every":
        return run(CHUNK, case, 3)
    L = n + 3 if n else 0
    return fill * 8 + run(L, case) + fill * (CHUNK - 8 - L)


def put(text, chunk_index, fill, case, n):
    """the chunk with n candidates as chunk `chunk_index` of text (a bytearray of filler); returns the candidates it must then have"""
    at = chunk_index * CHUNK
    text[at:at + CHUNK] = chunk_with(fill, case, n)
    if n != "every":
        return n
    if at == 0:
        return CHUNK - 3
    text[at - 3:at] = run(3, case, 0)
    return CHUNK


def queue_batch(fill, case, n, chunks_after):
    """(text, offsets): one chunk of filler, the chunk with n candidates, chunks_after of filler; three haystacks: all but the last 512 bytes, an empty one, the rest"""
    text = bytearray(fill * (CHUNK * (2 + chunks_after)))
    want = put(text, 1, fill, case, n)
    total = len(text)
    return bytes(text), np.asarray([0, total - 512, total - 512, total], np.int64), want


def unit_batch(fill, case, total, uc, ns=QUEUE_NS + ("every",)):
    """(text, offsets, [(chunk, candidates)]): `total` bytes of filler cut into a haystack per work unit of uc chunks for the units that are used and three haystacks
    behind them; n candidates in the FIRST chunk of unit 3 i + 1 and in the LAST chunk of unit 3 i + 2 for the i-th n"""
    text = bytearray(fill * total)
    placed = []
    for i, n in enumerate(ns):
        for chunk in ((3 * i + 1) * uc, (3 * i + 2) * uc + uc - 1):
            placed.append((chunk, put(text, chunk, fill, case, n)))
    used = 3 * len(ns) + 1
    assert (used + 3) * uc * CHUNK < total
    rest = (total - used * uc * CHUNK) // 3
    offs = [u * uc * CHUNK for u in range(used + 1)] + [used * uc * CHUNK + rest, used * uc * CHUNK + 2 * rest, total]
    return bytes(text), np.asarray(offs, np.int64), placed


def single_match_batch(fill, needle, last_byte_at, total):
    """(text, offsets): filler with `needle` (bytes) ending ON byte last_byte_at; two haystacks: everything but the last 256 bytes, and those"""
    text = bytearray(fill * total)
    assert 0 <= last_byte_at + 1 - len(needle) and last_byte_at < total - 256
    text[last_byte_at + 1 - len(needle):last_byte_at + 1] = needle
    return bytes(text), np.asarray([0, total - 256, total], np.int64)


def end_batch(fill, needle, total):
    """(text, offsets): `total` bytes that end with as much of the END of `needle` as fits whole (needle is None or longer than the batch: filler only)"""
    text = bytearray(fill * total)
    if needle is not None and len(needle) <= total:
        text[total - len(needle):] = needle
    return bytes(text), np.asarray([0, total] if total < 64 else [0, total // 2, total], np.int64)


def hay_start_batch(fill, case, long_needle, hs0, what, total):
    """(text, offsets, matches): two haystacks [0, hs0) and [hs0, total).  what = 3: the run's four bytes end 3 bytes after hs0 (one of them lies in the haystack
    before: no match); 4: they end 4 bytes after it (a match, end 4, in the second haystack); "across": long_needle with hs0 in its middle (no match)"""
    text = bytearray(fill * total)
    if what == "across":
        at = hs0 - len(long_needle) // 2
        text[at:at + len(long_needle)] = long_needle
    else:
        text[hs0 + what - 4:hs0 + what] = run(4, case)
    return bytes(text), np.asarray([0, hs0, total], np.int64), 1 if what == 4 else 0


def single_chunk_start_batch(fill, case, long_needle, into, what, total):
    """(text, offsets, matches, last): two haystacks [0, hs0) and [hs0, total) with hs0 = CHUNK - into, so that chunk 1 lies inside the second one and
    c0 - hs0 = into; the only candidate of the batch is IN CHUNK 1, on byte `last`.  what = 0..3: the run's four bytes end on offset `what` of chunk 1 -- a match
    (end what + 1 + into in the second haystack) when they begin at or behind hs0, i.e. what + into >= 3, and no match when one of them lies in the haystack before;
    "across": long_needle from one byte before hs0, ending inside chunk 1 (its last four bytes lie inside the second haystack, the needle does not: no match)"""
    hs0 = CHUNK - into
    text = bytearray(fill * total)
    if what == "across":
        assert len(long_needle) >= into + 2
        last = hs0 - 2 + len(long_needle)
        text[hs0 - 1:last + 1] = long_needle
        want = 0
    else:
        last = CHUNK + what
        text[last - 3:last + 1] = run(4, case)
        want = 1 if what + into >= 3 else 0
    assert last >= CHUNK
    return bytes(text), np.asarray([0, hs0, total], np.int64), want, last


def long_needle_of(needles, machine, case, fill):
    """the first a-z needle of seven to ten bytes that the oracle finds exactly once in itself between filler (upper case under IgnoreCase)"""
    for n in needles:
        if n.isascii() and n.isalpha() and 7 <= len(n) <= 10:
            b = (n.upper() if case else n).encode()
            if len(machine.run_list(case, fill * 8 + b + fill * 8)[0]) == 1:
                return b
    raise AssertionError("no such needle")
