"""The seven launchers of the postings stage (csrc/am_postings.hip: launch_post_keys, _hist, _scatter, _gather, _offsets, _df, _row_offsets) as a test sees them: the
sizes, the plans and the key patterns at which a radix pass can slip, each launcher's contract from csrc/am_postings.h written in numpy, and the calls into
libam_postcheck.so (tests/native/am_post_check.hip -- am_postings.hip itself, compiled with the product's flags, behind a C interface).  Shared by
tests/test_postings_cases_cpu.py (the definitions against plain Python, the size lists against the seams, the build, what the reporters see) and
tests/test_gpu_postings_sort.py (the kernels).

No definition uses another launcher's output: the bases a scatter is given are numpy's exclusive cumsum of numpy's count table, the keys an offsets call is given are
sorted by numpy.

The seams come from the library (ampc_limits, ampc_plan), never from a literal: a workgroup of `threads` lanes sorts a tile of T keys, each of its wavefronts W = T /
(threads / 64) CONSECUTIVE keys, 64 per round; the row kernels (keys, gather, offsets, df, row_offsets) give a lane one row in workgroups of R."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from alfred_margaret_amd import api, build

WAVE = 64
FILL_BYTE = 0xA5                                           # what every output array (and the guard behind it) holds before a call
MAX_CASE_BYTES = 64 << 20
INVALID_VALUE = 1                                          # hipErrorInvalidValue
SPAN = api.SPAN_DTYPE
assert SPAN.itemsize == 24

Limits = namedtuple("Limits", "tile wave threads row_threads max_spans")
Plan = namedtuple("Plan", "passes bits shift")             # bits and shift: four entries each, as the launchers take them

# the needle counts whose plans the sort tests run, pass by pass, and how each divides its key bits (tests/test_postings_cases_cpu.py holds ampc_plan to these)
PLAN_SPLITS = {2: [1], 4: [2], 8: [3], 16: [4], 32: [5], 64: [6], 128: [7], 256: [8], 257: [5, 4], 65536: [8, 8], 65537: [6, 6, 5], 2 ** 24: [8, 8, 8],
               2 ** 24 + 1: [7, 6, 6, 6], 2 ** 32: [8, 8, 8, 8]}
PLAN_NEEDLES = sorted(PLAN_SPLITS)

_lib = None


def lib():
    """libam_postcheck.so, built on demand; nothing but the tests loads it."""
    global _lib
    if _lib is None:
        path = os.path.join(build.LIB, "libam_postcheck.so")
        if not os.path.exists(path):
            path = build.build_postcheck()
        x = C.CDLL(path)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        x.ampc_guard_items.restype = u64
        x.ampc_limits.argtypes, x.ampc_limits.restype = [C.POINTER(u64)], None
        x.ampc_plan.argtypes, x.ampc_plan.restype = [u64, C.POINTER(u32)], None
        x.ampc_keys.argtypes = [vp, u64, u64, vp, vp]
        x.ampc_hist.argtypes = [C.POINTER(u32), u32, vp, u64, u64, vp, u64]
        x.ampc_scatter.argtypes = [C.POINTER(u32), u32, vp, vp, u64, u64, vp, u64, vp, vp]
        x.ampc_gather.argtypes = [vp, vp, u64, u64, vp, vp]
        x.ampc_offsets.argtypes = [vp, u64, u64, vp]
        x.ampc_df.argtypes = [vp, vp, u64, u64, u64, vp]
        x.ampc_row_offsets.argtypes = [vp, u64, u64, vp]
        x.ampc_bounds.argtypes = [C.POINTER(u32)]
        for f in (x.ampc_bounds, x.ampc_keys,x.ampc_hist, x.ampc_scatter, x.ampc_gather, x.ampc_offsets, x.ampc_df, x.ampc_row_offsets):
            f.restype = C.c_int
        _lib = x
    return _lib


def limits():
    out = (C.c_uint64 * 5)()
    lib().ampc_limits(out)
    return Limits(*[int(v) for v in out])


def guard():
    return int(lib().ampc_guard_items())


def bounds_failed():
    """(failed index assertions in the library's kernels so far, line of the first): zeros unless the library was built with AM_BOUNDS_CHECK and one failed"""
    out = (C.c_uint32 * 2)()
    assert lib().ampc_bounds(out) == 0
    return int(out[0]), int(out[1])


def plan(n_needles):
    """post_plan(n_needles), for a 64-bit n_needles"""
    out = (C.c_uint32 * 9)()
    lib().ampc_plan(n_needles, out)
    return Plan(int(out[0]), [int(v) for v in out[1:5]], [int(v) for v in out[5:9]])


def _plan9(pl):
    return (C.c_uint32 * 9)(pl.passes, *pl.bits, *pl.shift)


# ---- the sizes

def seams(lim):
    """(64, W, T): the keys of a round, of a wavefront's portion, of a tile"""
    return WAVE, lim.wave, lim.tile


def sort_sizes(lim):
    w, t = lim.wave, lim.tile
    return [0, 1, 63, 64, 65, w - 1, w, w + 1, t - 1, t, t + 1, 2 * t + 1, 3 * t + w + 1]


def tiles(lim, n):
    return (n + lim.tile - 1) // lim.tile


def row_sizes(lim):
    """spans of a keys / gather call: the sort's sizes and either side of a workgroup of the row kernels"""
    r = lim.row_threads
    return sorted(set(sort_sizes(lim)) | {r - 1, r, r + 1, 3 * r + 1})


# ---- the key patterns of one pass

def digit(pl, keys, p):
    """post_digit: bits [shift[p], shift[p] + bits[p]) of a key"""
    return (np.asarray(keys, np.uint32) >> np.uint32(pl.shift[p])) & np.uint32((1 << pl.bits[p]) - 1)


def key_bits(pl):
    return sum(pl.bits[:pl.passes])


def top_digit(pl, p, n_needles):
    """the largest digit value of pass p a key below n_needles can have"""
    return min((1 << pl.bits[p]) - 1, (n_needles - 1) >> pl.shift[p])


def seam_changes(lim, n):
    """the positions at which the "seam runs" pattern begins a new run: every round, wavefront and tile seam inside n that the pattern visits, one key before and one
    key after each"""
    at = set()
    for m in range(0, n + 1, lim.wave):                    # every wavefront seam (a tile seam among them), and the first round seam behind it
        for s in (m, m + WAVE):
            at |= {s - 1, s, s + 1}
    return np.asarray(sorted(x for x in at if 0 < x < n), np.int64)


def digit_patterns(lim, bits, n, rng):
    """(name, digit values uint32[n] below 2^bits) of every pattern of one pass"""
    d = 1 << bits
    i = np.arange(n, dtype=np.int64)
    lane = i % WAVE
    yield "one value", np.full(n, d - 1, np.int64)
    yield "top bit alternating", (i & 1) * (d >> 1)
    yield "lowest bit", (d - 2) + rng.integers(0, 2, n)
    blocks = n // d + 1
    yield "every value once per 2^bits", rng.random((blocks, d)).argsort(axis=1).reshape(-1)[:n]
    high = (i // WAVE) % max(d // WAVE, 1) * WAVE          # (7 and 8 bits: the bits above the lane number change from round to round)
    yield "lane", (lane + high) % d
    yield "63 - lane", (WAVE - 1 - lane + high) % d
    hot = np.asarray([7 % d, 8 % d, 40 % d, d - 1], np.int64)
    yield "skewed", np.where(rng.random(n) < 0.5, hot[rng.integers(0, 4, n)], rng.integers(0, d, n))
    step = 37 if bits < 7 else 101                         # (odd: every value is met; neighbouring runs differ in several bits, with 7 and 8 bits in bit 6 too)
    yield "seam runs", np.searchsorted(seam_changes(lim, n), i, side="right") * step % d
    if bits > 6:
        yield "values that differ above bit 5 only", rng.integers(0, d // WAVE, n) * WAVE + 21
    if n > 1 and n % lim.tile == 1:
        x = np.zeros(n, np.int64)
        x[-1] = d - 1
        yield "a lone key in the last tile", x


def sort_patterns(lim, pl, p, n, n_needles):
    """(name, keys uint32[n] below n_needles) for pass p: the digit patterns, with random bits in every other position of the key so that two keys of one digit value
    are seldom equal -- a swap of two of them shows in the keys as well as in the indices.  A digit value that no key below n_needles has is folded onto one that
    some key has (only in the last pass of a plan whose n_needles is not a power of two)."""
    rng = np.random.default_rng(7919 * n + 31 * p + n_needles % 1000003)
    field = ((1 << pl.bits[p]) - 1) << pl.shift[p]
    top = top_digit(pl, p, n_needles)
    for name, d in digit_patterns(lim, pl.bits[p], n, rng):
        d = (np.asarray(d, np.int64) % (top + 1)) << pl.shift[p]
        other = rng.integers(0, 1 << key_bits(pl), n, dtype=np.int64) & ~np.int64(field)
        lower = other & ((1 << (key_bits(pl) - 1)) - 1)    # (n_needles - 1 = 2^k: a key with bit k set has no other bit set)
        keys = np.where((other | d) < n_needles, other | d, np.where((lower | d) < n_needles, lower | d, d))
        assert n == 0 or (int(keys.max()) < n_needles and int(keys.min()) >= 0), name
        yield name, keys.astype(np.uint32)


def permutation(n, seed=0):
    return np.random.default_rng(104729 + seed + n).permutation(n).astype(np.uint32)


def random_spans(n, seed=0):
    """rows whose 24 bytes are all random"""
    rng = np.random.default_rng(15485863 + seed + n)
    return np.frombuffer(rng.bytes(24 * n), SPAN).copy() if n else np.zeros(0, SPAN)


# ---- the definitions

def hist_reference(lim, pl, p, keys):
    """counts[d * n_tiles + t] = keys of tile t whose digit is d: digit-major, every cell"""
    n_tiles, digits, t = tiles(lim, len(keys)), 1 << pl.bits[p], lim.tile
    out = np.zeros(digits * n_tiles, np.uint32)
    for k in range(n_tiles):
        out[k::n_tiles] = np.bincount(digit(pl, keys[k * t:(k + 1) * t], p), minlength=digits)
    return out


def bases(counts):
    """the exclusive sum of a count table, in uint64"""
    out = np.zeros(len(counts), np.uint64)
    if len(counts) > 1:
        np.cumsum(counts[:-1].astype(np.uint64), dtype=np.uint64, out=out[1:])
    return out


def scatter_reference(pl, p, keys, idx):
    order = np.argsort(digit(pl, keys, p), kind="stable")
    return keys[order], idx[order]


def gather_reference(spans, idx):
    return spans[idx], idx.astype(np.uint64)


def offsets_reference(keys, n_needles):
    """offsets[v] = first k with keys[k] >= v, for v <= n_needles; offsets[n_needles] = n"""
    out = np.searchsorted(keys.astype(np.uint64), np.arange(n_needles + 1, dtype=np.uint64), side="left").astype(np.uint64)
    out[n_needles] = len(keys)
    return out


def heads(keys, hay):
    """the first row, and every row whose key or haystack differs from the row before it"""
    h = np.ones(len(keys), bool)
    h[1:] = (keys[1:] != keys[:-1]) | (hay[1:] != hay[:-1])
    return h


def df_reference(keys, hay, n_needles):
    return np.bincount(keys[heads(keys, hay)], minlength=n_needles).astype(np.uint64)


def row_offsets_reference(hay, n_hay):
    out = np.searchsorted(hay.astype(np.uint64), np.arange(n_hay + 1, dtype=np.uint64), side="left").astype(np.uint64)
    out[n_hay] = len(hay)
    return out


# ---- the cases of df and row_offsets

def from_changes(n, changes):
    """0 for the rows before the first change, 1 from there to the second, ..."""
    return np.searchsorted(np.asarray(sorted(set(c for c in changes if 0 < c < n)), np.int64), np.arange(n, dtype=np.int64), side="right")


def lane_seams(lim):
    """where a run begins so that the run before it ends on lane 63, on lane 0, on the last lane of a workgroup of the row kernels and on the first of the next"""
    r = lim.row_threads
    return [WAVE, WAVE + 1, r, r + 1, r + WAVE, r + WAVE + 1, 2 * r, 2 * r + 1]


def run_changes(lengths):
    return np.cumsum(lengths).tolist()


def df_cases(lim):
    """(name, keys uint32[n] ascending, haystacks uint32[n], n_needles).  The key of the k-th needle run is the k-th of a random ascending choice from 0 .. n_needles
    - 1 that always holds n_needles - 1; the haystack number goes up by one at every haystack change and stays across a needle change that is none."""
    r = lim.row_threads
    rng = np.random.default_rng(2750159)
    n = 3 * r + 2
    s = lane_seams(lim)
    every = list(range(1, n))
    block_run = [r - 3, 2 * r + 5]                         # one run over rows r - 3 .. 2 r + 4: a whole workgroup and parts of both neighbours
    cases = [
        ("needle runs end on the lane seams, one haystack", n, s, []),
        ("haystack runs end on the lane seams, one needle", n, [], s),
        ("needle and haystack runs end on the same lane seams", n, s, s),
        ("needle runs on the seams, haystack runs one row later", n, s, [x + 1 for x in s] + [1, n - 1]),
        ("haystack runs on the seams, needle runs one row later", n, [x + 1 for x in s] + [1, n - 1], s),
        ("needle runs of 1, 64 and 65 rows", 2 * r + 200, run_changes([1, 64, 65, 1, 1, 65, 64, 64, 65, 1, 64]), []),
        ("haystack runs of 1, 64 and 65 rows in one needle run", 2 * r + 200, [], run_changes([1, 64, 65, 1, 1, 65, 64, 64, 65, 1, 64])),
        ("runs of 1, 64 and 65 rows, a random haystack change in three rows of ten", 2 * r + 200, run_changes([64, 1, 65, 65, 1, 64, 1]),
         [x for x in range(1, 2 * r + 200) if rng.random() < 0.3]),
        ("one needle run across a whole workgroup, one haystack", n, block_run, []),
        ("one needle run across a whole workgroup, one row per haystack", n, block_run, every),
        ("one needle with one row per haystack over more than a workgroup, then another", r + 70 + 5, [r + 70], every),
        ("a needle change at every row", n, every, []),
        ("random runs", 2 * r + 77, [x for x in range(1, 2 * r + 77) if rng.random() < 0.05], [x for x in range(1, 2 * r + 77) if rng.random() < 0.3]),
        ("one row", 1, [], []),
    ]
    for name, n, needle_changes, hay_changes in cases:
        run = from_changes(n, needle_changes)
        for n_needles in sorted({int(run[-1]) + 1, 1009} - set(range(int(run[-1]) + 1))):
            pick = np.sort(rng.choice(n_needles - 1, int(run[-1]), replace=False)) if run[-1] else np.zeros(0, np.int64)
            values = np.concatenate([pick, [n_needles - 1]])
            yield "%s, N = %d" % (name, n_needles), values[run].astype(np.uint32), from_changes(n, hay_changes).astype(np.uint32), n_needles


def df_rows(keys, hay, seed=0):
    rows = random_spans(len(keys), seed)
    rows["needle"], rows["haystack"] = keys, hay
    return rows


def row_hay_counts(lim):
    r = lim.row_threads
    return [0, 1, r - 1, r, r + 1, 3 * r + 1]


def row_offsets_cases(lim, n_hay):
    """(name, haystacks uint32[n_row] ascending and below n_hay) for one haystack count"""
    rng = np.random.default_rng(32452843 + n_hay)
    yield "no row", np.zeros(0, np.uint32)
    if n_hay == 0:
        return
    h = np.arange(n_hay, dtype=np.int64)
    yield "one row per haystack", h.astype(np.uint32)
    yield "every row in the first haystack", np.zeros(65, np.uint32)
    yield "every row in the last haystack", np.full(65, n_hay - 1, np.uint32)
    per = rng.choice([1, 1, 2, 3, 64, 65], n_hay)           # rows of a haystack that has any: runs of exactly 1, 64 and 65 among them
    yield "no empty haystack", np.repeat(h, per).astype(np.uint32)
    if n_hay >= 3:
        gone = np.zeros(n_hay, bool)
        gone[:max(n_hay // 10, 1)] = True
        gone[n_hay // 2 - n_hay // 20:n_hay // 2 + 1] = True
        gone[n_hay - max(n_hay // 10, 1):] = True
        yield "empty haystacks at the front, in the middle and at the end", np.repeat(h, np.where(gone, 0, per)).astype(np.uint32)
        sparse = rng.random(n_hay) < 0.8
        for s in lane_seams(lim):                          # ... with rows in the haystacks on either side of every lane seam
            if s < n_hay:
                sparse[s - 1:s + 1] = False
        yield "four haystacks of five empty", np.repeat(h, np.where(sparse, 0, per)).astype(np.uint32)


def row_rows(hay, seed=0):
    rows = random_spans(len(hay), seed)
    rows["haystack"] = hay
    return rows


def offsets_cases(lim):
    """(name, keys uint32[n] ascending and below n_needles, n_needles)"""
    r = lim.row_threads
    rng = np.random.default_rng(49979687)
    yield "no key, no needle", np.zeros(0, np.uint32), 0
    for n_needles in (1, 2, r - 2, r - 1, r, r + 1, 65537):  # (n_needles + 1 lanes: either side of a workgroup of the row kernels)
        for n in sort_sizes(lim):
            yield "random, n = %d, N = %d" % (n, n_needles), np.sort(rng.integers(0, n_needles, n)).astype(np.uint32), n_needles
        yield "the last needle alone, N = %d" % n_needles, np.full(65, n_needles - 1, np.uint32), n_needles
        yield "the first needle alone, N = %d" % n_needles, np.zeros(65, np.uint32), n_needles
        if n_needles > 2:
            yield "every needle but the first and the last, N = %d" % n_needles, np.arange(1, n_needles - 1, dtype=np.uint32), n_needles
            yield "every needle once, N = %d" % n_needles, np.arange(n_needles, dtype=np.uint32), n_needles


def case_bytes(lim, n, cells=0, n_needles=0):
    """host bytes of the largest call over n spans: the gather (rows in, rows out and expected, indices, sources and expected), a pass's tables, N + 1 offsets"""
    g = guard()
    return 24 * n + 2 * 24 * (n + g) + 4 * n + 2 * 8 * (n + g) + 3 * 8 * (cells + g) + 2 * 8 * (n_needles + 1 + g)


# ---- the calls: every one returns (launcher's error, outputs with their guards)

def fresh(n, dtype):
    a = np.empty(n + guard(), dtype)
    a.view(np.uint8)[:] = FILL_BYTE
    return a


def untouched(a):
    return bool((a.view(np.uint8) == FILL_BYTE).all())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _in(a, dtype):
    a = np.ascontiguousarray(a)
    assert a.dtype == dtype, (a.dtype, dtype)
    return a


def keys_call(spans, n=None):
    """n: what the launcher is told, when that is not len(spans)"""
    spans = _in(spans, SPAN)
    keys, idx = fresh(len(spans), np.uint32), fresh(len(spans), np.uint32)
    rc = lib().ampc_keys(_ptr(spans), len(spans) if n is None else n, len(spans), _ptr(keys), _ptr(idx))
    return rc, keys, idx


def hist_call(lim, pl, p, keys, n=None, cells=None):
    keys = _in(keys, np.uint32)
    if cells is None:
        cells = (1 << pl.bits[p]) * tiles(lim, len(keys))
    counts = fresh(cells, np.uint32)
    rc = lib().ampc_hist(_plan9(pl), p, _ptr(keys), len(keys) if n is None else n, len(keys), _ptr(counts), cells)
    return rc, counts


def scatter_call(pl, p, keys, idx, base, n=None):
    keys, idx, base = _in(keys, np.uint32), _in(idx, np.uint32), _in(base, np.uint64)
    assert len(idx) == len(keys)
    keys_out, idx_out = fresh(len(keys), np.uint32), fresh(len(keys), np.uint32)
    rc = lib().ampc_scatter(_plan9(pl), p, _ptr(keys), _ptr(idx), len(keys) if n is None else n, len(keys), _ptr(base), len(base), _ptr(keys_out), _ptr(idx_out))
    return rc, keys_out, idx_out


def gather_call(spans, idx, n=None):
    spans, idx = _in(spans, SPAN), _in(idx, np.uint32)
    assert len(idx) == len(spans)
    data, source = fresh(len(spans), SPAN), fresh(len(spans), np.uint64)
    rc = lib().ampc_gather(_ptr(spans), _ptr(idx), len(spans) if n is None else n, len(spans), _ptr(data), _ptr(source))
    return rc, data, source


def offsets_call(keys, n_needles):
    keys = _in(keys, np.uint32)
    out = fresh(n_needles + 1, np.uint64)
    return lib().ampc_offsets(_ptr(keys), len(keys), n_needles, _ptr(out)), out


def df_call(rows, keys, n_needles, n=None):
    """doc_freq goes in as zeros (the launcher adds), the guard behind it filled"""
    rows, keys = _in(rows, SPAN), _in(keys, np.uint32)
    assert len(rows) == len(keys)
    out = fresh(n_needles, np.uint64)
    out[:n_needles] = 0
    return lib().ampc_df(_ptr(rows), _ptr(keys), len(keys) if n is None else n, len(keys), n_needles, _ptr(out)), out


def row_offsets_call(rows, n_hay):
    rows = _in(rows, SPAN)
    out = fresh(n_hay + 1, np.uint64)
    return lib().ampc_row_offsets(_ptr(rows), len(rows), n_hay, _ptr(out)), out


# ---- the reporters: None when an output is what the definition says and the guard behind it is untouched; otherwise a short description

def _compare(out, exp, what, name):
    n = len(exp)
    if len(out) != n + guard():
        return "%s: %d elements of %s came back, %d expected" % (what, len(out), name, n + guard())
    if not untouched(out[n:]):
        return "%s: the guard behind %s[%d] was written" % (what, name, n)
    bad = np.flatnonzero(out[:n] != exp)
    if len(bad):
        i = int(bad[0])
        return "%s: %s[%d] = %s, expected %s (%d of %d differ)" % (what, name, i, out[i], exp[i], len(bad), n)
    return None


def hist_mismatch(lim, pl, p, keys, counts, what):
    return _compare(counts, hist_reference(lim, pl, p, keys), what, "counts")


def scatter_mismatch(pl, p, keys, idx, keys_out, idx_out, what):
    exp_keys, exp_idx = scatter_reference(pl, p, keys, idx)
    return _compare(keys_out, exp_keys, what, "keys_out") or _compare(idx_out, exp_idx, what, "idx_out")


def keys_mismatch(spans, keys, idx, what):
    return _compare(keys, spans["needle"], what, "keys") or _compare(idx, np.arange(len(spans), dtype=np.uint32), what, "idx")


def gather_mismatch(spans, idx, data, source, what):
    exp_data, exp_source = gather_reference(spans, idx)
    n = len(spans)
    if len(data) == n + guard() and untouched(data[n:]) and data[:n].tobytes() != exp_data.tobytes():       # all 24 bytes of every row
        i = int(np.flatnonzero((data[:n].view(np.uint8).reshape(n, 24) != exp_data.view(np.uint8).reshape(n, 24)).any(axis=1))[0])
        return "%s: data[%d] = %s, expected %s" % (what, i, data[i], exp_data[i])
    return _compare(data, exp_data, what, "data") or _compare(source, exp_source, what, "source")


def offsets_mismatch(keys, n_needles, out, what):
    return _compare(out, offsets_reference(keys, n_needles), what, "offsets")


def df_mismatch(keys, hay, n_needles, out, what):
    return _compare(out, df_reference(keys, hay, n_needles), what, "doc_freq")


def row_offsets_mismatch(hay, n_hay, out, what):
    return _compare(out, row_offsets_reference(hay, n_hay), what, "out_off")
