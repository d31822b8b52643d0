"""Texts whose leftmost-longest selection depends on the prefix maximum of csrc/am_spans.hip at its seams (k_spans_tile_max, k_spans_tiles_max, k_spans_heads), with
their expected rows written literally.  Shared by tests/test_spans_heads_model_cpu.py (a numpy model of the three passes says these texts can see a lost carry and
a lost tile base) and tests/test_gpu_spans.py (the kernels).

The model is the one tests/test_gpu_near.py uses.  Needle `c` makes every byte a candidate, so the candidate index is the byte index -- in a batch the global byte
index, since haystacks are contiguous.  A HEAD LETTER followed by L c's is a needle of its own whose span starts at the letter and COVERS the next L candidates:
they are heads of no chain and are not selected.  One letter per cover length, so no longer cover matches by accident.  Every byte starts exactly one span: the
letter's needle at a head letter, `c` elsewhere -- that is the AM_SPANS_ALL result as a set, and spans_reference.leftmost_longest over it is the definition.

Candidate i is a head iff i >= the maximum end of the candidates before it.  A lane holds tile / threads candidates, a wavefront 64 lanes, a workgroup one tile;
the tile maxima are combined by one workgroup in sweeps of `sweep` tiles with a carry.  For every seam s of these, a cover that starts before s ends (exclusive)
at s - 1, at s -- where `g >= run` decides --, at s + 1 and at s + 5; a cover of two tiles and a hundred reaches s from a tile that is not its neighbour, so
that the tile in between gets its base from tile_max alone and, at the sweep seam, from the carry alone; the same with a haystack that begins at s; and texts of
k tile - 1, k tile and k tile + 1 candidates, where the last tile holds nothing but the trailing element of `kept`."""
import functools
from collections import namedtuple

import numpy as np

from tests import scan_cases as sc, spans_reference as ref

WAVE = 64
Geometry = namedtuple("Geometry", "tile threads sweep")
Case = namedtuple("Case", "name hays n start length needle haystack")      # the literal AM_SPANS_ALL rows, one per byte: global index = row index; start is local
NAMES = ("end at s - 1", "end at s", "end at s + 1", "end at s + 5", "two tiles and more", "end at s - 1, haystack at s", "end at s, haystack at s",
         "two tiles, haystack at s")
GROUPS = ("tiles", "sweep")


def geometry():
    lim = sc.limits()
    return Geometry(lim.spans_tile, lim.spans_threads, lim.spans_tiles_sweep)


def covers(geo):
    """head letter -> the candidates behind it that its needle covers"""
    return {"a": 1, "b": 5, "d": 2 * geo.tile + 100, "e": 2 * geo.tile - 1}


def needles(geo):
    """handle 0 is `c`; then one needle per head letter"""
    return ["c"] + [k + "c" * n for k, n in sorted(covers(geo).items())]


def seams(geo, group):
    lane = geo.tile // geo.threads
    small = [lane, WAVE * lane, geo.tile, 3 * geo.tile]
    return small if group == "tiles" else small + [geo.sweep * geo.tile]


def _layout(geo, group, name):
    """(bytes of the text, [(position, head letter)], haystack starts behind the first)"""
    ss = seams(geo, group)
    far = ss[-1]                                                          # the seam the long covers reach: 3 tiles | the sweep
    k = far // geo.tile + 1                                               # tiles of the texts whose length sits on a tile seam
    if name.startswith("end at s - 1"):
        n, heads = k * geo.tile - 1, [(s - 3, "a") for s in ss]
    elif name.startswith("end at s + 1"):
        n, heads = k * geo.tile + 1, [(s - 1, "a") for s in ss]
    elif name.startswith("end at s + 5"):
        n, heads = far + 300, [(s - 1, "b") for s in ss]
    elif name.startswith("end at s"):
        n, heads = k * geo.tile, [(s - 2, "a") for s in ss]
    elif name == "two tiles and more":
        n, heads = far + 300, [(far - 2 * geo.tile, "d")]
    else:
        n, heads = far + 300, [(far - 2 * geo.tile, "e")]
    cuts = [] if "haystack at s" not in name else [far] if name.startswith("two tiles") else list(ss)
    return n, heads + [(n - 6, "b")], cuts                                # ... and a cover that ends with the text


@functools.lru_cache(maxsize=None)
def case(group, name):
    geo = geometry()
    n, heads, cuts = _layout(geo, group, name)
    cov = covers(geo)
    handle = {x[0]: v for v, x in enumerate(needles(geo))}
    text = bytearray(b"c" * n)
    length, needle = np.ones(n, np.uint64), np.zeros(n, np.uint32)
    taken = np.zeros(n, bool)
    for at, letter in heads:
        end = at + 1 + cov[letter]
        assert 0 <= at and end <= n and not taken[at:end].any(), (group, name, at, letter)      # the covers are apart, inside the text ...
        assert not any(at < c < end for c in cuts), (group, name, at, letter)                  # ... and inside one haystack
        taken[at:end] = True
        text[at] = ord(letter)
        length[at], needle[at] = cov[letter] + 1, handle[letter]
    bounds = [0] + cuts + [n]
    haystack = np.zeros(n, np.uint32)
    start = np.arange(n, dtype=np.uint64)
    for h, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
        haystack[lo:hi] = h
        start[lo:hi] -= np.uint64(lo)
    hays = [bytes(text[lo:hi]) for lo, hi in zip(bounds, bounds[1:])]
    for arr in (start, length, needle, haystack):
        arr.setflags(write=False)
    return Case(name, hays, n, start, length, needle, haystack)


def all_cases(group):
    return [case(group, name) for name in NAMES]


def rows(c):
    """the literal rows per haystack as tuples (start, len, handle)"""
    flat = list(zip(c.start.tolist(), c.length.tolist(), c.needle.tolist()))
    cut = np.flatnonzero(np.diff(c.haystack)) + 1
    bounds = [0] + cut.tolist() + [c.n]
    return [flat[lo:hi] for lo, hi in zip(bounds, bounds[1:])]


@functools.lru_cache(maxsize=None)
def leftmost_longest(group, name):
    """the definition over the literal rows: per haystack the list of (start, len, handle)"""
    return [ref.leftmost_longest(r) for r in rows(case(group, name))]
