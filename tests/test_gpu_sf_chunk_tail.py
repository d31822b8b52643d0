"""k_sf's chunk loop at the end of the batch and at the edges of a haystack (csrc/am_kernels.hip: the prefetch of the next chunk, the tail mask of the candidates, the
cached haystack bracket and `single`, which the loop decides with compares of chunk numbers inside the work unit, and the ring of deferred positions), against the
oracle.  Every batch is held to it exactly as tests/test_gpu_sf_chunk_loop.py holds its own -- emit, count and containsAny through that module's check(), the
instantiation each call launched held to launch_sf_t's rule --, with the needle families and the filler of tests/sf_chunk_cases.py, in both case modes.
  batch totals   1, 15, 16, 17, 1 023 .. 1 025, 1 039 .. 1 041, 2 047 .. 2 049 bytes (one-chunk units), and batches of work units of two chunks that end on a
                 unit's last byte, +- 1 byte and +- 1 024 +- 1 bytes (the unit size is the launcher's for the shape: asserted)
  needle ends    in each of them the run's four bytes end on the batch's last byte, on the first and the 16th byte of the last chunk and on the last byte of the
                 chunk before it, as far as they fit; each of those that lies inside one haystack must be among the oracle's matches
  haystack edge  a haystack boundary at c0 - 1, c0, c0 + 1 and c0 + 3 of the second and of the last chunk, a run of eight bytes across it (a match that ends on
                 the boundary, one that ends four bytes behind it, none in between): the bracket lookup and `single` flip exactly there; in a 20-KiB batch of
                 one-chunk units (the test at the unit's start) and in a batch of two-chunk units (the test inside the unit)
  ring wrap      100 candidates in the first chunk of a unit and 1 024 in its second: the deferred positions of one epoch pass the ring's 256 entries several
                 times, from a tail that is no multiple of 64"""
import numpy as np
import pytest

import alfred_margaret_amd as am
from tests import sf_chunk_cases as cc
from tests import test_gpu_sf_chunk_loop as loop

pytestmark = pytest.mark.gpu

_k_sf_only = loop._k_sf_only                        # the same fixtures: every call goes to k_sf, the Setups are released at the end of the module
_release_at_the_end = loop._release_at_the_end

PARAMS = loop.PARAMS
UNIT_PARAMS = [(f, c) for f in ("small", "large") for c in (0, 1)]          # <ILP 1, LW 0> (cfg2's instantiation) and <ILP 2, LW 15> (the headline's)
SMALL_TOTALS = (1, 15, 16, 17, 1023, 1024, 1025, 1039, 1040, 1041, 2047, 2048, 2049)
UNIT_DELTAS = (-1025, -1024, -1023, -1, 0, 1, 1023, 1024, 1025)
EDGE_DELTAS = (-1, 0, 1, 3)


def unit_shape():
    """(bytes of a batch that ends on the last byte of a work unit, chunks per unit): five units fewer than wavefronts, two chunks each -- a shape that keeps its
    unit size two chunks either way"""
    uc = 2
    return (16 * am.device_info()["n_cu"] - 5) * uc * cc.CHUNK, uc


def tail_batch(fill, case, total, offs):
    """(text, the global offsets of the last bytes of the runs placed): filler with the run's four bytes ending on the batch's last byte, on the first and the
    16th byte of the last chunk and on the last byte of the chunk before it, as far as they fit (runs that touch continue each other)"""
    text, lc0 = bytearray(fill * total), (total - 1) // cc.CHUNK * cc.CHUNK
    ends = sorted({e for e in (total - 1, lc0, lc0 + 15, lc0 - 1) if 3 <= e < total})
    for e in ends:
        text[e - 3:e + 1] = cc.run(4, case, e - 3)
    return bytes(text), [e for e in ends if np.searchsorted(offs, e - 3, side="right") == np.searchsorted(offs, e, side="right")]


def check_tail(s, case, total, offs):
    _, fill, _, _ = s.case(case)
    text, ends = tail_batch(fill, case, total, offs)
    exp = loop.check(s, case, text, offs)
    got = set((exp[1].astype(np.int64) + offs[exp[0]]).tolist())          # the bytes behind the oracle's matches, in the batch
    assert all(e + 1 in got for e in ends), (total, ends)
    assert len(ends) or total < 4


@pytest.mark.parametrize("family,case", PARAMS)
def test_batches_that_end_around_a_lane_and_a_chunk(family, case):
    s = loop.setup_of(family)
    for total in SMALL_TOTALS:
        check_tail(s, case, total, np.asarray([0, total] if total < 64 else [0, total // 2, total], np.int64))


@pytest.mark.parametrize("delta", UNIT_DELTAS)
@pytest.mark.parametrize("family,case", UNIT_PARAMS)
def test_batches_that_end_around_the_end_of_a_work_unit(family, case, delta):
    base, uc = unit_shape()
    total = base + delta
    assert am.api.sf_unit_chunks(total) == uc and base % (uc * cc.CHUNK) == 0
    check_tail(loop.setup_of(family), case, total, np.asarray([0, total // 2, total], np.int64))


def edge_batch(fill, case, total, edge):
    """(text, offsets): two haystacks [0, edge) and [edge, total), a run of eight bytes with the edge in its middle"""
    text = bytearray(fill * total)
    text[edge - 4:edge + 4] = cc.run(8, case, edge - 4)
    return bytes(text), np.asarray([0, edge, total], np.int64)


def check_edges(s, case, total):
    _, fill, _, _ = s.case(case)
    last_c0 = (total - 1) // cc.CHUNK * cc.CHUNK
    assert total - last_c0 > 8 and last_c0 > 2 * cc.CHUNK
    for c0 in (cc.CHUNK, last_c0):
        for d in EDGE_DELTAS:
            text, offs = edge_batch(fill, case, total, c0 + d)
            exp = loop.check(s, case, text, offs)
            assert exp[0].tolist() == [0, 1] and exp[1].tolist() == [c0 + d, 4]          # the run's first four bytes end the first haystack, its last four begin the second


@pytest.mark.parametrize("family,case", PARAMS)
def test_a_haystack_edge_around_the_start_of_a_chunk_of_one_chunk_units(family, case):
    check_edges(loop.setup_of(family), case, 20 * cc.CHUNK + 19)


@pytest.mark.parametrize("family,case", UNIT_PARAMS)
def test_a_haystack_edge_around_the_start_of_a_chunk_inside_a_unit(family, case):
    """chunk 1 is the second chunk of unit 0; the batch's last chunk, a partial one, is the second chunk of the last unit"""
    base, uc = unit_shape()
    total = base - cc.CHUNK + 19
    assert am.api.sf_unit_chunks(total) == uc and ((total - 1) // cc.CHUNK) % uc == uc - 1
    check_edges(loop.setup_of(family), case, total)


@pytest.mark.parametrize("family,case", UNIT_PARAMS)
def test_the_ring_of_deferred_positions_wraps_inside_an_epoch(family, case):
    s = loop.setup_of(family)
    model, fill, _, _ = s.case(case)
    total, uc = unit_shape()
    assert am.api.sf_unit_chunks(total) == uc
    text = bytearray(fill * total)
    first = 3 * uc                                     # unit 3: 100 candidates in its first chunk, every position of its second
    assert cc.put(text, first, fill, case, 100) == 100 and cc.put(text, first + 1, fill, case, "every") == cc.CHUNK
    counts = model.per_chunk(bytes(text))
    assert counts[first] == 100 and counts[first + 1] == cc.CHUNK and counts.sum() == 100 + cc.CHUNK
    exp = loop.check(s, case, bytes(text), np.asarray([0, total // 2, total], np.int64))
    assert len(exp[0]) == 100 + cc.CHUNK               # every candidate is a match and is deferred first: far more than the ring's 256 entries
