"""The seven launchers of the postings stage on the device (csrc/am_postings.hip), one at a time, each against its contract in csrc/am_postings.h written in numpy
(tests/postings_cases.py; held to plain Python by tests/test_postings_cases_cpu.py).  They are called directly, through libam_postcheck.so
(tests/native/am_post_check.hip: am_postings.hip itself with the product's flags), on what the host sequence of am_postings.cpp never hands them: every pass of every
plan on one to four tiles, 7- and 8-bit digits whose values fill a round of 64 lanes or differ above bit 5 only, keys of 25 to 32 bits, bases and index arrays that
are numpy's and not another launcher's, n == 0.  Every call hands its outputs back with a guard behind them: nothing beyond what the launcher owns is written, and a
refused call writes nothing at all."""
import numpy as np
import pytest

from tests import postings_cases as pc

pytestmark = pytest.mark.gpu

LIM = pc.limits()
SIZES = pc.sort_sizes(LIM)


@pytest.fixture(autouse=True)
def _no_index_assertion_failed():
    """In an AM_BOUNDS_CHECK build the kernels in the test library count their own failed index assertions (a product build has none to count)."""
    yield
    assert pc.bounds_failed() == (0, 0)


# ---- launch_post_hist / launch_post_scatter: every pass of the plan, every pattern

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("n_needles", pc.PLAN_NEEDLES)
def test_hist_of_every_pass(n_needles, n):
    pl = pc.plan(n_needles)
    bad = []
    for p in range(pl.passes):
        for name, keys in pc.sort_patterns(LIM, pl, p, n, n_needles):
            rc, counts = pc.hist_call(LIM, pl, p, keys)
            why = "error %d" % rc if rc != 0 else pc.hist_mismatch(LIM, pl, p, keys, counts, name)
            if why:
                bad.append("pass %d: %s" % (p, why))
    assert bad == []


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("n_needles", pc.PLAN_NEEDLES)
def test_scatter_of_every_pass(n_needles, n):
    pl = pc.plan(n_needles)
    idx = pc.permutation(n)
    bad = []
    for p in range(pl.passes):
        for name, keys in pc.sort_patterns(LIM, pl, p, n, n_needles):
            base = pc.bases(pc.hist_reference(LIM, pl, p, keys))
            rc, keys_out, idx_out = pc.scatter_call(pl, p, keys, idx, base)
            why = "error %d" % rc if rc != 0 else pc.scatter_mismatch(pl, p, keys, idx, keys_out, idx_out, name)
            if why:
                bad.append("pass %d: %s" % (p, why))
    assert bad == []


def test_a_pass_over_nothing_writes_nothing():
    pl = pc.plan(256)
    none32, none64 = np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    rc, counts = pc.hist_call(LIM, pl, 0, none32)
    assert rc == 0 and pc.untouched(counts)
    rc, counts = pc.hist_call(LIM, pl, 0, none32, cells=256)
    assert rc == 0 and pc.untouched(counts)
    rc, keys_out, idx_out = pc.scatter_call(pl, 0, none32, none32, none64)
    assert rc == 0 and pc.untouched(keys_out) and pc.untouched(idx_out)


def test_two_scatters_give_the_same_bytes():
    for n_needles in (256, 2 ** 24 + 1):
        pl = pc.plan(n_needles)
        for n in SIZES[-2:]:
            idx = pc.permutation(n)
            for p in (0, pl.passes - 1):
                for name, keys in pc.sort_patterns(LIM, pl, p, n, n_needles):
                    base = pc.bases(pc.hist_reference(LIM, pl, p, keys))
                    (r1, k1, i1), (r2, k2, i2) = pc.scatter_call(pl, p, keys, idx, base), pc.scatter_call(pl, p, keys, idx, base)
                    assert r1 == 0 and r2 == 0 and k1.tobytes() == k2.tobytes() and i1.tobytes() == i2.tobytes(), (n_needles, n, p, name)


# ---- the refusals: before any launch, the outputs as they went in

def refused(rc, *outs):
    return rc == pc.INVALID_VALUE and all(pc.untouched(o) for o in outs)


def test_a_pass_the_plan_does_not_have_is_refused():
    for n_needles, p in ((256, 1), (65537, 3), (2 ** 32, 4), (1, 0)):
        pl = pc.plan(n_needles)
        assert p >= pl.passes
        keys = next(iter(pc.sort_patterns(LIM, pc.plan(256), 0, 65, 256)))[1]
        rc, counts = pc.hist_call(LIM, pl, p, keys, cells=256)
        assert refused(rc, counts), (n_needles, p)
        rc, keys_out, idx_out = pc.scatter_call(pl, p, keys, pc.permutation(65), np.zeros(256, np.uint64))
        assert refused(rc, keys_out, idx_out), (n_needles, p)


@pytest.mark.parametrize("bits", [0, 9, 32])
def test_a_digit_of_no_bits_or_of_more_than_eight_is_refused(bits):
    pl = pc.Plan(1, [bits, 0, 0, 0], [0, 0, 0, 0])
    keys = np.arange(65, dtype=np.uint32)
    rc, counts = pc.hist_call(LIM, pl, 0, keys, cells=512)
    assert refused(rc, counts)
    rc, keys_out, idx_out = pc.scatter_call(pl, 0, keys, pc.permutation(65), np.zeros(512, np.uint64))
    assert refused(rc, keys_out, idx_out)
    good = pc.Plan(2, [8, bits, 0, 0], [0, 8, 0, 0])       # ... while a pass of the same plan that is well-formed runs
    rc, counts = pc.hist_call(LIM, good, 0, keys)
    assert rc == 0 and pc.hist_mismatch(LIM, good, 0, keys, counts, "pass 0") is None
    rc, counts = pc.hist_call(LIM, good, 1, keys, cells=512)
    assert refused(rc, counts)


def test_a_span_count_the_index_arrays_cannot_hold_is_refused():
    """The count alone, with arrays of 64 elements: the launcher must turn it away before it touches them."""
    pl = pc.plan(256)
    spans, keys, idx = pc.random_spans(64), np.arange(64, dtype=np.uint32), pc.permutation(64)
    for n in (LIM.max_spans, LIM.max_spans + 1, 1 << 40):
        assert refused(*pc.keys_call(spans, n=n)), n
        assert refused(*pc.hist_call(LIM, pl, 0, keys, n=n, cells=256)), n
        assert refused(*pc.scatter_call(pl, 0, keys, idx, np.zeros(256, np.uint64), n=n)), n
        assert refused(*pc.gather_call(spans, idx, n=n)), n
        rc, out = pc.df_call(spans, keys, 256, n=n)
        assert rc == pc.INVALID_VALUE and not out[:256].any() and pc.untouched(out[256:]), n


# ---- launch_post_keys / launch_post_gather

@pytest.mark.parametrize("n", pc.row_sizes(LIM))
def test_keys_and_the_identity(n):
    spans = pc.random_spans(n)
    rc, keys, idx = pc.keys_call(spans)
    assert rc == 0 and pc.keys_mismatch(spans, keys, idx, n) is None


@pytest.mark.parametrize("n", pc.row_sizes(LIM))
def test_gather_moves_whole_rows(n):
    spans = pc.random_spans(n, seed=1)
    for seed in (0, 1):
        idx = pc.permutation(n, seed)
        rc, data, source = pc.gather_call(spans, idx)
        assert rc == 0 and pc.gather_mismatch(spans, idx, data, source, (n, seed)) is None
    if n:
        idx = np.full(n, n - 1, np.uint32)                 # every posting from one row
        rc, data, source = pc.gather_call(spans, idx)
        assert rc == 0 and pc.gather_mismatch(spans, idx, data, source, (n, "one row")) is None


# ---- launch_post_offsets

def test_offsets_are_the_lower_bounds():
    bad = []
    for name, keys, n_needles in pc.offsets_cases(LIM):
        rc, out = pc.offsets_call(keys, n_needles)
        why = "error %d" % rc if rc != 0 else pc.offsets_mismatch(keys, n_needles, out, name)
        if why:
            bad.append(why)
    assert bad == []


def test_offsets_without_a_key():
    for n_needles in (0, 1, LIM.row_threads, LIM.row_threads + 1):
        rc, out = pc.offsets_call(np.zeros(0, np.uint32), n_needles)
        assert rc == 0 and not out[:n_needles + 1].any() and pc.untouched(out[n_needles + 1:]), n_needles


# ---- launch_post_df

def test_document_frequencies_at_the_lane_seams():
    bad = []
    for name, keys, hay, n_needles in pc.df_cases(LIM):
        rows = pc.df_rows(keys, hay)
        rc, out = pc.df_call(rows, keys, n_needles)
        why = "error %d" % rc if rc != 0 else pc.df_mismatch(keys, hay, n_needles, out, name)
        if why:
            bad.append(why)
        rc2, again = pc.df_call(rows, keys, n_needles)     # integer adds commute: the same bytes
        if rc2 != rc or again.tobytes() != out.tobytes():
            bad.append("%s: two runs differ" % name)
    assert bad == []


def test_document_frequencies_of_no_row():
    rc, out = pc.df_call(np.zeros(0, pc.SPAN), np.zeros(0, np.uint32), 5)
    assert rc == 0 and not out[:5].any() and pc.untouched(out[5:])


# ---- launch_post_row_offsets

@pytest.mark.parametrize("n_hay", pc.row_hay_counts(LIM))
def test_row_offsets_per_haystack(n_hay):
    bad = []
    for name, hay in pc.row_offsets_cases(LIM, n_hay):
        rc, out = pc.row_offsets_call(pc.row_rows(hay), n_hay)
        why = "error %d" % rc if rc != 0 else pc.row_offsets_mismatch(hay, n_hay, out, name)
        if why:
            bad.append(why)
    assert bad == []
