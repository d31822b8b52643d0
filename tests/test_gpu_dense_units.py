"""The empty-needle route (k_sf + k_dense, csrc/am_dense.hip) beyond one-chunk units, against the plain reference of tests/helpers.py (dense_reference, which
tests/test_dense_units_cpu.py holds to the oracle) and against the oracle itself.  A work unit is unit_chunks KiB (am_debug_sf_unit_chunks); how much of k_dense runs
depends on it: words per unit n_words = 32 * unit_chunks, words per thread of the write pass per = ceil(n_words / 256).  The shapes, on 256 compute units:
  one           ~3 MiB        unit_chunks  1   n_words   32  per 1   > 3 000 units
  two           4 MiB + 4 KiB unit_chunks  2   n_words   64  per 1   more than 32 words per unit
  eight         32 MiB        unit_chunks  8   n_words  256  per 1   the last per = 1
  nine          36 MiB        unit_chunks  9   n_words  288  per 2   the first per = 2
  sixty-four    256 MiB       unit_chunks 64   n_words 2048  per 8   kDenseWords, bit 65 535
  thirty-three  256 MiB + 64K unit_chunks 33   n_words 1056  per 5   two units per wavefront (the k = 2 branch of sf_unit_chunks)
Every batch is a device batch the library BORROWS (am_batch_from_device: readable up to round_up(total, 16) only): a few MiB of dense_text tiled to the size, cut by
ragged_cuts.  Every test asserts the geometry it claims and skips where the device's compute units put it beyond 512 MiB."""
import ctypes as C
import random
from concurrent.futures import ThreadPoolExecutor
from contextlib import contextmanager

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests.helpers import DENSE_CHUNK, DENSE_ONLY_SETS, DENSE_SETS, dense_reference, dense_text, ragged_cuts

pytestmark = pytest.mark.gpu

MIB = 1 << 20
# name -> (unit_chunks it reaches, total bytes as a function of the wavefronts W = 16 * compute units); on 256 compute units the sizes of the table above
SHAPES = {"one": (1, lambda w: (3 * w // 4) * 1024 + 77), "two": (2, lambda w: w * 1024 + 4096 + 19), "eight": (8, lambda w: 8 * w * 1024), "nine": (9, lambda w: 9 * w * 1024 - 13),
          "sixty-four": (64, lambda w: 64 * w * 1024), "thirty-three": (33, lambda w: 64 * w * 1024 + 64 * 1024 + 5)}
_BASE = {}


def lib():
    return am.api.libam()


def geometry(shape):
    """(total bytes, unit_chunks) of a shape on this device, read from the library; skips where the shape is out of reach."""
    n_cu = am.device_info()["n_cu"]
    want, total_of = SHAPES[shape]
    total = total_of(16 * n_cu)
    if total > 512 * MIB:
        pytest.skip("%d compute units: unit_chunks = %d needs a batch of %d bytes, beyond 512 MiB" % (n_cu, want, total))
    uc = am.api.sf_unit_chunks(total)
    assert uc == want == am.api.sf_unit_chunks(total, n_cu), (shape, total, uc)
    assert uc * (DENSE_CHUNK // 32) <= 2048
    return total, uc


def base_text(name):
    """2 MiB and a bit of dense_text per alphabet, once per module; "plain": no first code point of {"", "a"} at all."""
    if name not in _BASE:
        alphabet = [("x", 5), ("ü", 2), ("語", 2), ("💩", 1)] if name == "plain" else DENSE_SETS[name][2]
        _BASE[name] = np.frombuffer(dense_text(random.Random(7), 2 * MIB + 12345, alphabet), dtype=np.uint8)
    return _BASE[name]


def host_batch(name, shape):
    """(text np.uint8[total], offsets np.int64, unit bytes): the base text tiled to the size (ragged_cuts' pattern of lengths has another period), a code point the
    end cuts becomes x's."""
    total, uc = geometry(shape)
    base = base_text(name)
    text = np.resize(base, total)
    k = total - 1
    while (text[k] & 0xC0) == 0x80:
        k -= 1
    if text[k] >= 0xC0 and k + (2 if text[k] < 0xE0 else 3 if text[k] < 0xF0 else 4) > total:
        text[k:] = ord("x")
    offs = ragged_cuts(text, random.Random(13), uc * DENSE_CHUNK, big=MIB if shape == "one" else 3 * MIB)
    return text, offs, uc * DENSE_CHUNK


@contextmanager
def device_batch(text, offs):
    """The batch in HBM, borrowed by the library; destroyed (and the tensors dropped) on the way out."""
    import torch
    dev = torch.device("cuda:0")
    t, o = torch.from_numpy(text).to(dev), torch.from_numpy(offs).to(dev)
    b = C.c_void_p()
    am.api.check(lib().am_batch_from_device(t.data_ptr(), o.data_ptr(), len(offs) - 1, len(text), C.byref(b)))
    try:
        yield b
    finally:
        lib().am_batch_destroy(b)
        del t, o
        torch.cuda.empty_cache()


@contextmanager
def run_batch(a, case, b):
    m = C.c_void_p()
    am.api.check(lib().am_run_batch(a.device, case, b, C.byref(m)))
    try:
        yield m
    finally:
        lib().am_matches_free(m)


def records(m, first=0, count=None):
    """Records [first, first + count) of a result, read in pieces of 4 Mi records (am_matches_copy)."""
    n = int(lib().am_matches_size(m)) - first if count is None else count
    out = np.zeros(n, am.api.MATCH_DTYPE)
    step = 4 << 20
    for at in range(0, n, step):
        k = min(step, n - at)
        am.api.check(lib().am_matches_copy(m, C.c_uint64(first + at), C.c_uint64(k), out[at:at + k].ctypes.data))
    return out


def reference(case, needles, text, offs):
    """dense_reference over groups of whole haystacks on a few threads: (haystack u32, end_pos u32, n_values u8) of the whole batch."""
    n_hay = len(offs) - 1
    marks = np.unique(np.searchsorted(offs, np.arange(0, len(text), 4 * MIB), side="left").clip(0, n_hay))
    groups = [(int(i), int(j)) for i, j in zip(np.r_[0, marks], np.r_[marks, n_hay]) if j > i]

    def part(g):
        i, j = g
        h, e, v = dense_reference(case, needles, text[offs[i]:offs[j]], offs[i:j + 1] - offs[i])
        return (h + i).astype(np.uint32), e.astype(np.uint32), v.astype(np.uint8)

    with ThreadPoolExecutor(12) as pool:
        parts = list(pool.map(part, groups))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def check_against(rs, ref, vlen, where):
    hay, end, n_values = ref
    assert len(rs) == len(hay), (where, len(rs), len(hay))
    assert np.array_equal(rs["haystack"], hay) and np.array_equal(rs["end_pos"], end), where
    key = (rs["haystack"].astype(np.uint64) << np.uint64(32)) | rs["end_pos"]
    assert (key[1:] > key[:-1]).all(), where                                    # strictly increasing (haystack, end_pos)
    assert np.array_equal(vlen[rs["state"]], n_values), where


def expand(rs, vo, vals):
    st = rs["state"].astype(np.int64)
    lens = (vo[st + 1] - vo[st]).astype(np.int64)
    start = np.repeat(vo[st].astype(np.int64), lens)
    within = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    return np.repeat(rs["end_pos"], lens), vals[start + within] if len(start) else np.zeros(0, np.uint32)


def spread_of(offs, unit, total):
    """>= 64 haystacks: the first, the last, the largest, every one that straddles a unit boundary among the first and the last 8 units, others evenly spaced."""
    n_hay, n_units = len(offs) - 1, (total + unit - 1) // unit
    idx = {0, n_hay - 1, int(np.argmax(np.diff(offs)))}
    for u in list(range(1, min(9, n_units))) + list(range(max(1, n_units - 8), n_units)):
        h = int(np.searchsorted(offs, u * unit, side="right")) - 1
        if offs[h] < u * unit < offs[h + 1]:
            idx.add(h)
    idx.update(int(x) for x in np.linspace(0, n_hay - 1, 64))
    return sorted(idx)


def records_of_haystacks(m, h0, h1):
    """The records of haystacks h0 .. h1 of a result in one copy."""
    f0, c0, f1, c1 = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    am.api.check(lib().am_matches_haystack_range(m, int(h0), C.byref(f0), C.byref(c0)))
    am.api.check(lib().am_matches_haystack_range(m, int(h1), C.byref(f1), C.byref(c1)))
    return records(m, f0.value, f1.value + c1.value - f0.value)


@pytest.fixture(scope="module", autouse=True)
def _release_at_the_end():
    yield
    _BASE.clear()
    lib().am_release_device_memory()
    lib().am_release_host_memory()


MAIN = [(name, case) for name in DENSE_SETS for case in (0, 1)]


@pytest.mark.parametrize("name,case", MAIN, ids=["%s-case%d" % nc for nc in MAIN])
@pytest.mark.parametrize("shape", ("one", "two", "eight", "nine"))
def test_records_of_the_whole_batch_equal_the_reference(shape, name, case):
    """1. Every record of the batch: (haystack, end_pos) and the number of values of its state against dense_reference, on the suffix-filter route; the library's own
    choice (kernel 0) gives the same bytes; a spread of haystacks against the oracle's (position, value) lists."""
    needles = DENSE_SETS[name][1]
    text, offs, unit = host_batch(name, shape)
    total, n_hay = len(text), len(offs) - 1
    if shape == "one":
        assert (total + unit - 1) // unit >= 3000
    ref = reference(case, needles, text, offs)
    a, o = am.Automaton(needles), oracle.Machine(needles)
    vo, vals = a.values_off(), a.values()
    vlen = np.diff(vo).astype(np.uint8)
    idx = spread_of(offs, unit, total)
    assert len(idx) >= 64
    with device_batch(text, offs) as b:
        a.set_kernel(2)
        with run_batch(a, case, b) as m:
            rs = records(m)
            check_against(rs, ref, vlen, (shape, name, case))
            first, count = C.c_uint64(0), C.c_uint64(0)
            am.api.check(lib().am_matches_haystack_range(m, n_hay - 1, C.byref(first), C.byref(count)))
            assert first.value + count.value == len(rs)
        a.set_kernel(0)
        with run_batch(a, case, b) as m:
            assert np.array_equal(records(m).view(np.uint64), rs.view(np.uint64)), "kernel 0 chose another result"
    bounds = np.searchsorted(rs["haystack"], np.arange(n_hay + 1))
    for i in idx:
        gpos, gval = expand(rs[bounds[i]:bounds[i + 1]], vo, vals)
        pos, val = o.run_list(case, text, int(offs[i]), int(offs[i + 1] - offs[i]))
        assert np.array_equal(gpos, pos) and np.array_equal(gval, val), (shape, name, case, "haystack", i)


@pytest.mark.parametrize("shape,name", (("sixty-four", "sensitive"), ("thirty-three", "ignore")))
def test_the_largest_units_counts_flags_and_sampled_records(shape, name):
    """2. n_words = kDenseWords (bit 65 535, per = 8) and the two-units-per-wavefront geometry: counts and flags of ALL haystacks against the reference, the records of
    every haystack that touches the first 4, the last 4 and 56 evenly spaced units (64 units of ~4 000, ~1.6 %)."""
    case, needles, _ = DENSE_SETS[name]
    text, offs, unit = host_batch(name, shape)
    total, n_hay = len(text), len(offs) - 1
    n_units = (total + unit - 1) // unit
    hay, end, n_values = ref = reference(case, needles, text, offs)
    exp_counts = np.bincount(hay, weights=n_values, minlength=n_hay).astype(np.uint64)
    a = am.Automaton(needles)
    vlen = np.diff(a.values_off()).astype(np.uint8)
    a.set_kernel(2)
    units = sorted(set(list(range(4)) + list(range(n_units - 4, n_units)) + [int(x) for x in np.linspace(4, n_units - 5, 56)]))
    with device_batch(text, offs) as b:
        counts, tot = np.zeros(n_hay, np.uint64), C.c_uint64(0)
        am.api.check(lib().am_count_batch(a.device, case, b, counts.ctypes.data, C.byref(tot)))
        assert np.array_equal(counts, exp_counts) and tot.value == int(exp_counts.sum())
        flags = np.zeros(n_hay, np.uint8)
        am.api.check(lib().am_contains_any_batch(a.device, case, b, flags.ctypes.data))
        assert np.array_equal(flags.astype(bool), exp_counts > 0)
        with run_batch(a, case, b) as m:
            assert int(lib().am_matches_size(m)) == len(hay)
            seen = set()
            for u in units:
                h0 = int(np.searchsorted(offs, u * unit, side="right")) - 1
                h1 = int(np.searchsorted(offs, min((u + 1) * unit, total) - 1, side="right")) - 1
                if (h0, h1) in seen:
                    continue
                seen.add((h0, h1))
                r0, r1 = np.searchsorted(hay, [h0, h1 + 1])
                check_against(records_of_haystacks(m, h0, h1), (hay[r0:r1], end[r0:r1], n_values[r0:r1]), vlen, (shape, "unit", u))
            first, count = C.c_uint64(0), C.c_uint64(0)
            am.api.check(lib().am_matches_haystack_range(m, n_hay - 1, C.byref(first), C.byref(count)))
            assert first.value + count.value == int(lib().am_matches_size(m))
    a.set_kernel(0)


@pytest.mark.parametrize("name", list(DENSE_SETS))
@pytest.mark.parametrize("shape", ("one", "two"))
def test_the_general_kernel_gives_the_same_bytes(shape, name):
    """3. k_ac, the second algorithm: the same record array byte for byte."""
    case, needles, _ = DENSE_SETS[name]
    text, offs, _ = host_batch(name, shape)
    a = am.Automaton(needles)
    with device_batch(text, offs) as b:
        got = []
        for kernel in (2, 1):
            a.set_kernel(kernel)
            with run_batch(a, case, b) as m:
                got.append(records(m).view(np.uint64))
    a.set_kernel(0)
    assert len(got[0]) > len(text) // 4 and np.array_equal(got[0], got[1])


def test_only_the_dense_part():
    """4. No sparse record at all at the 9-chunk shape: {""} alone and {"", "É"} under IgnoreCase (sf_tiers == 0) report nothing, as the reference; {"", "a"} over text
    without an a reports nothing, over a's alone a record at every byte with two values (the closed form of tests/test_gpu_one_large_document.py)."""
    text, offs, _ = host_batch("sensitive", "nine")
    n_hay = len(offs) - 1
    with device_batch(text, offs) as b:
        for case, needles in DENSE_ONLY_SETS.values():
            assert len(dense_reference(case, needles, text[:MIB], [0, MIB])[0]) == 0
            a = am.Automaton(needles)
            a.set_kernel(2)
            with run_batch(a, case, b) as m:
                assert int(lib().am_matches_size(m)) == 0, needles
            counts, tot = np.ones(n_hay, np.uint64), C.c_uint64(1)
            am.api.check(lib().am_count_batch(a.device, case, b, counts.ctypes.data, C.byref(tot)))
            flags = np.ones(n_hay, np.uint8)
            am.api.check(lib().am_contains_any_batch(a.device, case, b, flags.ctypes.data))
            assert tot.value == 0 and not counts.any() and not flags.any(), needles
    a = am.Automaton(["", "a"])
    a.set_kernel(2)
    vlen = np.diff(a.values_off()).astype(np.uint8)
    plain, poffs, _ = host_batch("plain", "nine")
    with device_batch(plain, poffs) as b:
        assert len(dense_reference(0, ["", "a"], plain[:MIB], [0, MIB])[0]) == 0
        with run_batch(a, 0, b) as m:
            assert int(lib().am_matches_size(m)) == 0
    alla = np.full(len(text), ord("a"), dtype=np.uint8)
    with device_batch(alla, offs) as b:
        with run_batch(a, 0, b) as m:
            rs = records(m)
    hay = np.repeat(np.arange(n_hay, dtype=np.uint32), np.diff(offs))
    assert len(rs) == len(alla) and np.array_equal(rs["haystack"], hay) and np.array_equal(rs["end_pos"], np.arange(len(alla), dtype=np.uint64) - offs[hay].astype(np.uint64) + np.uint64(1))
    assert (vlen[rs["state"]] == 2).all()


@pytest.mark.parametrize("name", list(DENSE_SETS))
def test_the_other_entry_points_on_these_records(name):
    """5. The 9-chunk shape through the entry points that consume the records: the fold checksum per haystack against the oracle's, counts per needle (the empty
    needle's is the number of records), containsAll on the record route."""
    case, needles, _ = DENSE_SETS[name]
    text, offs, _ = host_batch(name, "nine")
    n_hay = len(offs) - 1
    o = oracle.Machine(needles)
    with ThreadPoolExecutor(12) as pool:
        lists = list(pool.map(lambda i: o.run_list(case, text, int(offs[i]), int(offs[i + 1] - offs[i])), range(n_hay)))
        hashes = list(pool.map(lambda i: o.fold_hash(case, text, int(offs[i]), int(offs[i + 1] - offs[i])), range(n_hay)))
    by_needle = sum(np.bincount(v, minlength=len(needles)) for _, v in lists)
    n_records = sum(len(np.unique(p)) for p, _ in lists)
    has_all = np.array([o.contains_all(case, text, int(offs[i]), int(offs[i + 1] - offs[i])) for i in range(n_hay)])
    assert np.array_equal(has_all, [len(np.unique(v)) == len(needles) for _, v in lists]) and has_all.any() and not has_all.all()
    a = am.Automaton(needles)
    a.set_kernel(2)
    vt = am.api.ValuesTable(a)
    with device_batch(text, offs) as b:
        with run_batch(a, case, b) as m:
            assert int(lib().am_matches_size(m)) == n_records
            h, c = vt.fold_hash(m, n_hay)
            assert np.array_equal(h, np.array([x[0] for x in hashes], dtype=np.uint64)) and np.array_equal(c, np.array([x[1] for x in hashes], dtype=np.uint64))
        got = vt.count_by_needle_batch(case, b)
        assert np.array_equal(got, by_needle.astype(np.uint64)) and int(got[needles.index("")]) == n_records
        flags = np.zeros(n_hay, np.uint8)
        am.api.check(lib().am_contains_all_batch(vt.handle, case, b, flags.ctypes.data))
        assert np.array_equal(flags.astype(bool), has_all)
    a.set_kernel(0)


def test_one_document_in_uneven_ranges():
    """6. The 9-chunk text as ONE haystack: am_run_range over 7 uneven ranges -- cuts inside code points and on unit boundaries -- concatenates to the whole
    document's records (k_range_bounds / k_range_rebase on dense results), which are the reference's; am_count_range adds up to am_count."""
    case, needles, _ = DENSE_SETS["sensitive"]
    text, _, unit = host_batch("sensitive", "nine")
    n = len(text)
    inside = [int(k) for k in np.flatnonzero((text[:n - 1] & 0xC0) == 0x80)[[1000, 700000, 5000000]]]
    cuts = [0, inside[0], 5 * unit, inside[1], 777 * unit, inside[2], 20 * MIB + 1, n]
    assert cuts == sorted(cuts) and len(cuts) == 8
    a = am.Automaton(needles)
    a.set_kernel(2)
    vlen = np.diff(a.values_off()).astype(np.uint8)
    sl = am.api.Slice(text.ctypes.data, 0, n)
    parts, counted = [], 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        m, c = C.c_void_p(), C.c_uint64(0)
        am.api.check(lib().am_run_range(a.device, case, C.byref(sl), lo, hi, C.byref(m)))
        try:
            parts.append(records(m))
        finally:
            lib().am_matches_free(m)
        am.api.check(lib().am_count_range(a.device, case, C.byref(sl), lo, hi, C.byref(c)))
        assert c.value == int(vlen[parts[-1]["state"]].sum(dtype=np.int64)), (lo, hi)
        counted += c.value
    rs = np.concatenate(parts)
    check_against(rs, reference(case, needles, text, np.array([0, n], dtype=np.int64)), vlen, "ranges")
    whole = np.zeros(1, np.uint64)
    am.api.check(lib().am_count(a.device, case, C.byref(sl), 1, whole.ctypes.data))
    assert counted == int(whole[0])
    a.set_kernel(0)


def test_two_runs_give_identical_bytes():
    """7. The 9-chunk shape twice."""
    case, needles, _ = DENSE_SETS["ignore"]
    text, offs, _ = host_batch("ignore", "nine")
    a = am.Automaton(needles)
    a.set_kernel(2)
    with device_batch(text, offs) as b:
        with run_batch(a, case, b) as m:
            one = records(m).view(np.uint64)
        with run_batch(a, case, b) as m:
            assert np.array_equal(records(m).view(np.uint64), one)
    a.set_kernel(0)
