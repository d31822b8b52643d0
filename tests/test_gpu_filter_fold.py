"""k_sf's suffix filter hashes IgnoreCase windows modulo the ASCII case bit (bloom_key, csrc/am_image.h): text that differs from a needle in bit 5 of a byte only
-- `@` for '`', `[ \\ ] ^` for `{ | } ~`, 0x10-0x19 for digits, continuation bytes 0x80-0x9F for 0xA0-0xBF -- now passes the filter and has to be settled by the
exact probe and resolve; real case variants must still be found.  A few hundred needles of 1-20 bytes over an alphabet that holds both members of every such
pair, both case modes, haystacks of 4 KiB at most whose matches are PLACED: at each of the 16 bytes of a lane (the four window positions of each of its dwords,
the windows that cross into the lane below), across a 1-KiB chunk boundary, in the first bytes of a work unit (the carry path), at the first and at the last byte
of a haystack.  Records and counts against the oracle, in order.  The batches are device batches the library borrows, so the layout is the test's own."""
import ctypes as C
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle

pytestmark = pytest.mark.gpu

# both members of pairs that differ in bit 5 of one byte: ASCII punctuation, every control byte 0x10-0x19 with its digit, letters; two-byte code points whose
# continuation bytes differ in bit 5 -- all of U+00C0..DF (C3 80..9F) with U+00E0..FF (C3 A0..BF): case pairs (É é, Ð ð) and two that are none (× ÷, ß ÿ) -- and А а,
# Α α, Đ İ (no case pair); then case pairs that differ elsewhere (ω Ω, р Р) and the three-byte case variants of k and ω (U+212A, U+2126)
PAIRS = (["@`", "[{", "\\|", "]}", "^~", "aA", "kK", "zZ", "аА", "αΑ", "Đİ", "ωΩ", "рР"] + [chr(0x10 + i) + chr(0x30 + i) for i in range(10)] +
         [chr(0xC0 + i) + chr(0xE0 + i) for i in range(32)])
EXTRA = ["\u212a", "\u2126", " ", "語"]
ALPHABET = [c for p in PAIRS for c in p] + EXTRA
FLIP = {a: b for p in PAIRS for a, b in (p, p[::-1])}
CHUNK = 1024


def make_needles(rng, lo, hi, n=300):
    out = set()
    while len(out) < n:
        s = ""
        want = rng.randint(lo, hi)
        while len(s.encode()) < want:
            s += rng.choice(ALPHABET)
        if lo <= len(s.encode()) <= hi:
            out.add(s)
    return sorted(out)


def flipped(rng, needle, p):
    """the needle with some characters replaced by their bit-5 partner: a case variant where the pair is a case pair, a near miss where it is not"""
    return "".join(FLIP[c] if c in FLIP and rng.random() < p else c for c in needle)


def filler(rng, n_bytes):
    """n_bytes bytes of the alphabet, padded to the exact length with one-byte characters"""
    s, n = [], 0
    while n < n_bytes - 3:
        c = rng.choice(ALPHABET)
        s.append(c)
        n += len(c.encode())
    s.append("".join(rng.choice("@`[{^~\x10 ") for _ in range(n_bytes - n)))
    return "".join(s)


def make_haystacks(rng, needles, plantable, unit):
    """Haystacks (bytes, <= 4 KiB each) whose concatenation puts a planted needle's LAST byte at chosen offsets of a lane, of a chunk and of a unit of `unit` bytes,
    and the list of global end offsets that were planted."""
    hays, planted, at = [], [], 0

    def plant(end_mod, modulus, needle, tail):
        nonlocal at
        nb = needle.encode()
        lead = (end_mod - (at + len(nb) - 1)) % modulus
        if modulus > 2048:                                    # a unit of several chunks: a haystack stays below 4 KiB, fillers take the distance
            while lead > 3000:
                h = filler(rng, 3000).encode()
                hays.append(h); at += len(h); lead -= 3000
        h = (filler(rng, lead) + needle + filler(rng, tail)).encode()
        assert len(h) <= 4096
        planted.append(at + lead + len(nb) - 1)
        hays.append(h); at += len(h)

    # `plantable`: needles that match themselves (lower case under IgnoreCase), planted as they are -- a match for certain -- and once more with partners strewn in
    pick = lambda: rng.choice(plantable)
    for r in range(16):                                       # every byte of a lane: window positions 0-3 of its four dwords; 0-2: the window reaches into the lane below
        plant(16 * rng.randint(1, 60) + r, CHUNK, pick(), rng.randint(0, 40))
        plant(16 * rng.randint(1, 60) + r, CHUNK, flipped(rng, pick(), rng.choice((0.3, 1.0))), rng.randint(0, 40))
    for r in (0, 1, 2, 3, CHUNK - 1, CHUNK - 2):              # the suffix window, or the needle before it, crosses a chunk boundary
        plant(r, CHUNK, pick(), rng.randint(0, 40))
    for r in (0, 1, 2, 3, 4, 5, 17):                          # ... and a unit boundary: the first bytes of a work unit (carry)
        plant(r, unit, pick(), rng.randint(0, 40))
    for n in needles[::7]:                                    # a haystack that is a needle (or a variant): first and last byte at once; and needles at either end
        hays.append(n.encode())
        hays.append(flipped(rng, n, 0.5).encode())
        hays.append((flipped(rng, n, 0.5) + filler(rng, rng.randint(1, 900)) + flipped(rng, n, 0.5)).encode())
    hays += [b"", filler(rng, 4096).encode(), "".join(rng.choice(ALPHABET) for _ in range(1200)).encode()[:4096].decode(errors="ignore").encode()]
    for _ in range(12):                                       # random text with needles and near misses strewn in
        parts = []
        while sum(len(p.encode()) for p in parts) < 3500:
            parts.append(flipped(rng, rng.choice(needles), rng.choice((0.0, 0.2, 1.0))) if rng.random() < 0.5 else filler(rng, rng.randint(1, 30)))
        hays.append("".join(parts).encode()[:4096].decode(errors="ignore").encode())
    return hays, planted


def oracle_records(o, case, hays):
    """(haystack, end_pos, n_values) per matching position, in order, and the per-haystack counts"""
    rec, counts = [], []
    for i, h in enumerate(hays):
        pos, _val = o.run_list(case, h)
        pos = np.asarray(pos, np.uint64)
        counts.append(len(pos))
        ends, n = np.unique(pos, return_counts=True)                 # (the fold reports a position's values together, positions ascending)
        rec += [(i, int(e), int(k)) for e, k in zip(ends, n)]
    return np.array(rec, np.int64).reshape(-1, 3), counts


def device_records(a, case, hays, vlen_of):
    """am_run_batch on a borrowed device batch (text contiguous, as make_haystacks laid it out): (haystack, end_pos, n_values) in the order of the result"""
    import torch
    lib = am.api.libam()
    text = np.frombuffer(b"".join(hays) + b"\0" * 16, np.uint8)
    offs = np.zeros(len(hays) + 1, np.int64)
    offs[1:] = np.cumsum([len(h) for h in hays])
    dev = torch.device("cuda:0")
    t, o_ = torch.from_numpy(text.copy()).to(dev), torch.from_numpy(offs).to(dev)
    b, m = C.c_void_p(), C.c_void_p()
    am.api.check(lib.am_batch_from_device(t.data_ptr(), o_.data_ptr(), len(hays), int(offs[-1]), C.byref(b)))
    try:
        am.api.check(lib.am_run_batch(a.device, case, b, C.byref(m)))
        try:
            n = int(lib.am_matches_size(m))
            out = np.zeros(n, am.api.MATCH_DTYPE)
            if n:
                am.api.check(lib.am_matches_copy(m, C.c_uint64(0), C.c_uint64(n), out.ctypes.data))
        finally:
            lib.am_matches_free(m)
    finally:
        lib.am_batch_destroy(b)
    return np.stack([out["haystack"].astype(np.int64), out["end_pos"].astype(np.int64), vlen_of[out["state"]].astype(np.int64)], axis=1)


@pytest.mark.parametrize("case", [am.CASE_SENSITIVE, am.IGNORE_CASE], ids=["CaseSensitive", "IgnoreCase"])
@pytest.mark.parametrize("lengths", [(1, 20), (4, 20)], ids=["1-20 bytes", "4-20 bytes"])      # with and without the short tiers (another k_sf instantiation)
def test_bit5_neighbours_at_every_window_position(case, lengths):
    rng = random.Random(1000 * case + lengths[0])
    needles = make_needles(rng, *lengths)
    if case == am.IGNORE_CASE:                                # lower-case needles, a few left as they are (those can only match themselves where they are lower case)
        needles = sorted({n if i % 10 == 0 else oracle.lower_utf8(n).decode() for i, n in enumerate(needles)})
    plantable = [n for n in needles if len(n.encode()) >= 6 and (case == am.CASE_SENSITIVE or n == oracle.lower_utf8(n).decode())]
    hays, planted = make_haystacks(rng, needles, plantable, CHUNK)
    total = sum(len(h) for h in hays)
    assert all(len(h) <= 4096 for h in hays) and am.api.sf_unit_chunks(total) == 1      # every chunk is a work unit: each starts with the carry
    o = oracle.Machine(needles)
    exp, exp_counts = oracle_records(o, case, hays)
    # the placement is what the docstring says: ends at every byte of a lane, on both sides of a chunk boundary, at the first and last byte of a haystack
    offs = np.concatenate([[0], np.cumsum([len(h) for h in hays])])
    ends = np.array([offs[h] + e - 1 for h, e, _ in exp])
    assert set(ends % 16) == set(range(16)) and {0, 1, 2, 3, 4, 5, 17, CHUNK - 1, CHUNK - 2} <= set(ends % CHUNK)
    assert set(planted) <= set(ends) | set(planted[1:32:2])      # every needle planted as it is was found where it was put (the odd plants are variants or near misses)
    assert sum(1 for h, e, _ in exp if e == len(hays[h]) and hays[h].decode() in needles) >= len(needles[::7]) - 30      # a haystack that is a needle: first byte to last
    assert len(exp) > 300
    a = am.Automaton(needles)
    a.set_kernel(2)                                           # k_sf
    vlen_of = np.diff(o.values_off())
    got = device_records(a, case, hays, vlen_of)
    assert got.shape == exp.shape and np.array_equal(got, exp)
    assert [int(c) for c in a.count_matches(case, hays)] == exp_counts


def test_chunk_boundaries_inside_a_work_unit():
    """The same haystacks repeated until a work unit is two chunks or more: a chunk boundary inside a unit hands the carry on in registers, a unit boundary fetches
    it.  The reference is the oracle's records of one repetition, shifted: the text is the same, only where it lies in chunks and lanes changes from copy to copy."""
    rng = random.Random(77)
    needles = sorted({oracle.lower_utf8(n).decode() for n in make_needles(rng, 4, 20)})      # (no short needles: they end at almost every byte, millions of records)
    base, _ = make_haystacks(rng, needles, [n for n in needles if len(n.encode()) >= 6], 2 * CHUNK)
    if sum(len(h) for h in base) % 16 == 0:
        base.append(b"@")                                    # every copy at another offset in its lane
    n_base, base_bytes = len(base), sum(len(h) for h in base)
    reps = 16 * am.device_info()["n_cu"] * CHUNK // base_bytes + 2          # more than one chunk per wavefront (16 wavefronts per compute unit)
    hays = base * reps
    assert am.api.sf_unit_chunks(base_bytes * reps) >= 2
    o = oracle.Machine(needles)
    one, _ = oracle_records(o, am.IGNORE_CASE, base)
    a = am.Automaton(needles)
    a.set_kernel(2)
    got = device_records(a, am.IGNORE_CASE, hays, np.diff(o.values_off()))
    exp = np.tile(one, (reps, 1))
    exp[:, 0] += np.repeat(np.arange(reps) * n_base, len(one))
    assert len(one) > 300 and got.shape == exp.shape and np.array_equal(got, exp)
