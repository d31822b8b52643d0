"""(CPU) The case list of tests/spans_seam_cases.py can see the faults it is for.  A numpy model of the prefix maximum of csrc/am_spans.hip -- k_spans_tile_max, the
sweeps of k_spans_tiles_max with their carry, and k_spans_heads with its lanes, wavefronts and tile base -- equals the plain running maximum on every case; with
the carry dropped it differs on at least one case, and so it does with the tile base, the wavefronts before a lane's own or the lanes before it dropped.  The
literal rows are also held to the definition: their heads are selected by spans_reference.leftmost_longest, and what a cover covers is not."""
import numpy as np
import pytest

from tests import spans_seam_cases as cases

FAULTS = ("carry", "tile base", "wavefronts before", "lanes before")


def ends(c):
    g = np.arange(c.n, dtype=np.uint64)
    return g, g + c.length


def plain_heads(c):
    """head[i] = i >= the maximum end of every candidate before i"""
    g, e = ends(c)
    before = np.zeros(c.n, np.uint64)
    before[1:] = np.maximum.accumulate(e)[:-1]
    return g >= before


def _exclusive(x, axis):
    """the exclusive running maximum along an axis, 0 before the first element"""
    incl = np.maximum.accumulate(x, axis=axis)
    out = np.zeros_like(x)
    dst = [slice(None)] * x.ndim
    src = list(dst)
    dst[axis], src[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = incl[tuple(src)]
    return out


def model_heads(c, geo, drop=None):
    g, e = ends(c)
    per, waves = geo.tile // geo.threads, geo.threads // cases.WAVE
    nt = (c.n + 1 + geo.tile - 1) // geo.tile                            # (+ 1: the trailing element of kept)
    ee, gg = np.zeros(nt * geo.tile, np.uint64), np.zeros(nt * geo.tile, np.uint64)
    ee[:c.n], gg[:c.n] = e, g
    # k_spans_tile_max
    tile_max = ee.reshape(nt, geo.tile).max(axis=1)
    # k_spans_tiles_max: one workgroup, sweeps of `sweep` tiles
    base, carry = np.zeros(nt, np.uint64), np.uint64(0)
    for i0 in range(0, nt, geo.sweep):
        v = tile_max[i0:i0 + geo.sweep]
        base[i0:i0 + geo.sweep] = np.maximum(np.uint64(0) if drop == "carry" else carry, _exclusive(v, 0))
        carry = max(carry, v.max())
    if drop == "tile base":
        base[:] = 0
    # k_spans_heads: a lane's own candidates, the lanes before it in its wavefront, the wavefronts before its own, the tile's base
    lanes = ee.reshape(nt, waves, cases.WAVE, per)
    mine = lanes.max(axis=3)
    lanes_before = _exclusive(mine, 2)
    waves_before = _exclusive(mine.max(axis=2), 1)[:, :, None]
    if drop == "lanes before":
        lanes_before = np.zeros_like(lanes_before)
    if drop == "wavefronts before":
        waves_before = np.zeros_like(waves_before)
    run = np.maximum(np.maximum(lanes_before, waves_before), base[:, None, None])[:, :, :, None]
    run = np.maximum(run, _exclusive(lanes, 3))
    return (gg.reshape(lanes.shape) >= run).reshape(-1)[:c.n]


@pytest.mark.parametrize("group", cases.GROUPS)
def test_the_model_is_the_running_maximum_and_sees_each_fault(group):
    geo = cases.geometry()
    seen = {f: [] for f in FAULTS}
    for c in cases.all_cases(group):
        want = plain_heads(c)
        assert np.array_equal(model_heads(c, geo), want), c.name
        for f in FAULTS:
            if not np.array_equal(model_heads(c, geo, drop=f), want):
                seen[f].append(c.name)
    # a cover that ends before s or at s is no evidence; one that ends behind s is
    for f in ("tile base", "wavefronts before", "lanes before") + (("carry",) if group == "sweep" else ()):
        assert "end at s + 1" in seen[f] and "end at s + 5" in seen[f], (f, seen[f])
        assert "end at s - 1" not in seen[f] and "end at s" not in seen[f], (f, seen[f])
    # the tile in between has its base from tile_max alone; at the sweep seam from the carry alone
    assert "two tiles and more" in seen["tile base"] and "two tiles, haystack at s" in seen["tile base"]
    assert ("two tiles and more" in seen["carry"]) == (group == "sweep") and "two tiles, haystack at s" not in seen["carry"]      # (ends at the sweep seam: no carry)
    if group == "tiles":
        assert seen["carry"] == []                                       # fewer tiles than a sweep: no carry to lose


def test_the_literal_rows():
    geo = cases.geometry()
    lane = geo.tile // geo.threads
    assert cases.seams(geo, "sweep") == [lane, cases.WAVE * lane, geo.tile, 3 * geo.tile, geo.sweep * geo.tile]
    assert len(set(len(x) for x in cases.needles(geo))) == len(cases.needles(geo)) == 5
    sizes = sorted(c.n for c in cases.all_cases("tiles"))
    assert {4 * geo.tile - 1, 4 * geo.tile, 4 * geo.tile + 1} <= set(sizes)
    sizes = sorted(c.n for c in cases.all_cases("sweep"))
    assert {(geo.sweep + 1) * geo.tile - 1, (geo.sweep + 1) * geo.tile, (geo.sweep + 1) * geo.tile + 1, geo.sweep * geo.tile + 300} <= set(sizes)
    for c in cases.all_cases("tiles"):
        text = b"".join(c.hays)
        assert len(text) == c.n and sum(map(len, c.hays)) == c.n
        assert ("haystack at s" in c.name) == (len(c.hays) > 1)
        for i in np.flatnonzero(c.needle).tolist():                      # a head letter, its c's behind it, inside one haystack
            word = cases.needles(geo)[int(c.needle[i])]
            assert text[i:i + len(word)] == word.encode() and int(c.length[i]) == len(word) and c.haystack[i] == c.haystack[i + len(word) - 1]
        assert text.count(b"c") == c.n - np.count_nonzero(c.needle)
        # the definition over the literal rows keeps exactly: every head of the running maximum, and never a covered candidate
        kept = np.zeros(c.n, bool)
        lo = 0
        for h, row in enumerate(cases.leftmost_longest("tiles", c.name)):
            kept[[lo + s for s, _, _ in row]] = True
            lo += len(c.hays[h])
        assert np.array_equal(kept, plain_heads(c)), c.name
        covered = np.zeros(c.n, bool)
        for i in np.flatnonzero(c.needle).tolist():
            covered[i + 1:i + int(c.length[i])] = True
        assert not (kept & covered).any() and (kept | covered).all()
