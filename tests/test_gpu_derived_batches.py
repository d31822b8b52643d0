"""The batches the library derives in HBM (csrc/am_fold.h DerivedBatch) at the builder's edges: am_batch_from_selection, am_batch_from_fragments and
am_batch_substitute producing 0, 1, 15, 16, 17 and 33 bytes -- every residue class the zero tail distinguishes, and the empty batch -- in 0, 1 and 3 haystacks, one
of them empty, in the middle and at the end; and the sub-batch that the group loop of the per-needle counts refills group after group.  A produced batch must hold
the offsets and bytes of the Python references, count like any other batch (am_count_batch against the oracle), and give back every device byte."""
import ctypes as C
import gc

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import select_reference as sel, substitute_reference as subref
from tests.test_gpu_needle_counts import Batch, hist_launches, oracle_counts
from tests.test_gpu_splitter_device import expected as split_expected

pytestmark = pytest.mark.gpu

TOTALS = (0, 1, 15, 16, 17, 33)
COUNTED = ["ab", "b", "c"]                                 # what am_count_batch looks for in a produced batch
SUBST = (["#", "@", "%%"], ["", "ab", "c"])                 # needles and their replacements: one deletes, one grows, one shrinks


def shapes(total):
    """The haystack lengths of the produced batches of `total` bytes: none at all (the empty batch), one, and three with an empty one in the middle / at the end."""
    if total == 0:
        return [[], [0], [0, 0, 0]]
    a = total // 2
    return [[total], [a, 0, total - a], [a, total - a, 0]]


def produced_texts(lens):
    out = []
    for i, n in enumerate(lens):
        out.append((b"abcb xcab"[i:] * (n // 4 + 1))[:n])
    return out


def device_bytes():
    gc.collect()
    lib = am.api.libam()
    am.api.check(lib.am_release_device_memory())
    return int(lib.am_debug_device_buffer_bytes())


def from_selection(want):
    """grep -v '#': the wanted texts between haystacks that are dropped.  -> (source haystacks, the reference's texts, produce(batch) -> am_batch*)"""
    src = [b"#dropped"]
    for t in want:
        src += [t, b"x#"]
    if not want:
        src = []                                           # (a source without haystacks; from_selection_all_dropped is the other way to nothing)
    kept = sel.keep(sel.pred_any(["#"], 0), True, src)[1]
    a = am.Automaton(["#"])

    def produce(b):
        s = am.api._select(lambda out: am.api.libam().am_select_any_batch(a.device, 0, 1, b, out))
        assert s.size == len(kept)
        return s.batch(b)
    return src, kept, produce


def from_selection_all_dropped(want):
    assert not want
    a = am.Automaton(["#"])
    return [b"#", b"a#"], [], lambda b: am.api._select(lambda out: am.api.libam().am_select_any_batch(a.device, 0, 1, b, out)).batch(b)


def from_fragments(want):
    """document -> lines: the wanted texts joined by the separator, the last one a document of its own."""
    src = [b",".join(want[:-1]), want[-1]] if len(want) > 1 else list(want)
    frags = [bytes(h)[s:s + n] for h, row in zip(src, split_expected(",", False, src)) for s, n in row]
    sp = am.Splitter(",")

    def produce(b):
        nb, _ = sp.lines_batch(b)
        return nb
    return src, frags, produce


def from_substitute(want):
    """Every wanted text with its "ab" and "c" written as the needles that are replaced by them, behind a needle that is deleted; an empty one at the end stays empty."""
    needles, repls = SUBST
    src = [b"" if (not t and i == len(want) - 1) else b"#" + t.replace(b"ab", b"@").replace(b"c", b"%%") for i, t in enumerate(want)]
    exp = subref.substitute(oracle.Machine(needles, list(range(len(needles)))), 0, needles, src, repls)
    a = am.Automaton(needles)
    table = am.SubstTable(am.SpanTable(a), repls)
    return src, exp, lambda b: table.substitute_batch(0, b, raw=True)


PRODUCERS = {"selection": from_selection, "fragments": from_fragments, "substitute": from_substitute}


def check_produced(make, want):
    lib = am.api.libam()
    src, exp, produce = make(want)
    assert exp == want                                     # the input was chosen to produce exactly these
    counter, o = am.Automaton(COUNTED), oracle.Machine(COUNTED)
    with Batch(src) as b:
        nb = produce(b)
        try:
            assert int(lib.am_batch_haystacks(nb)) == len(exp) and int(lib.am_batch_total_bytes(nb)) == sum(map(len, exp))
            offs, texts = am.api.batch_to_bytes(nb)
            assert offs.tolist() == sel.offsets(exp).tolist() and texts == exp
            counts, total = np.full(len(exp) + 1, 99, np.uint64), C.c_uint64(99)
            am.api.check(lib.am_count_batch(counter.device, 0, nb, counts.ctypes.data, C.byref(total)))
            assert counts[:len(exp)].tolist() == [o.count_matches(0, t) for t in exp] and int(total.value) == int(counts[:len(exp)].sum())
        finally:
            lib.am_batch_destroy(nb)


def check_groups():
    """AM_HIST_RECORDS_MIB = 1: 65 536 records at a time.  Every 70 000-byte haystack is a group of one, and what lies between two of them is a group of its own, copied
    into the one sub-batch: 1, 15 (7 + 0 + 8), 16, 17 (17 + 0) and 33 bytes, from starts that are not 16-byte aligned in the source."""
    big = 70000
    lens = [big, 1, big, 7, 0, 8, big + 3, 16, big, 17, 0, big + 5, 33]
    hays = [np.full(n, ord("a"), np.uint8) for n in lens]
    needles = ["a", "aa", "aaa"]
    exp = oracle_counts(oracle.Machine(needles), 0, hays, 3)
    assert exp.tolist() == [sum(max(0, n - d) for n in lens) for d in range(3)]
    t = am.ValuesTable(am.Automaton(needles))
    with Batch(hays) as b:
        free, n_free = hist_launches(lambda: t.count_by_needle_batch(0, b))
        am.debug_set("AM_HIST_RECORDS_MIB", 1)
        try:
            forced, n_forced = hist_launches(lambda: t.count_by_needle_batch(0, b))
        finally:
            am.debug_set("AM_HIST_RECORDS_MIB", -1)
    assert forced.tolist() == free.tolist() == exp.tolist()
    assert (n_free, n_forced) == (1, 10)                   # one fold of the whole batch; five groups of one and the five between them


CASES = [(p, t) for p in sorted(PRODUCERS) for t in TOTALS] + [("fold_groups", None)]


@pytest.mark.parametrize("producer,total", CASES, ids=["%s-%s" % c for c in CASES])
def test_derived_batch(producer, total):
    start = device_bytes()
    if producer == "fold_groups":
        check_groups()
    else:
        for lens in shapes(total):
            check_produced(PRODUCERS[producer], produced_texts(lens))
        if producer == "selection" and total == 0:
            check_produced(from_selection_all_dropped, [])
    assert device_bytes() == start
