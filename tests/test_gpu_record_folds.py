"""The folds over the sorted records of a scan, held to EACH OTHER on one record set: per-needle counts, the needle matrix, scores, spans, the whole-word forms, the
slot rows behind the rule sets, containsAll's record route and the fold checksum all expand a record through the same flat value lists (csrc/am_records.h), so on one
batch their results are tied together by identities, whatever the table.  The other suites hold each stage to its oracle; this one sits on the sizes where a shared
tile loader can go wrong: record counts around a wavefront, around a wavefront's share of k_score's tile, around the tile and around the matrix's records per flush
(both read from the library, never written down here), in batches whose runs of equal haystacks are one long run, all of length 1, or end at, before and after a
wavefront's edge.  The dictionary a / aa / aaa gives states that carry 1, 2 and 3 values: a text of n `a`s leaves exactly n records.  Every quantity is an integer and
is compared exactly, against the host mirrors the stages' own suites use."""
import ctypes as C
import functools

import numpy as np
import pytest

import alfred_margaret_amd as am

pytestmark = pytest.mark.gpu

# needles and their value handles: the plain dictionary, and one where handle 1 is given to two equal needles (the value list of state `aa` carries it twice)
DICTS = {"plain": (["a", "aa", "aaa"], [0, 1, 2]), "shared": (["a", "aa", "aaa", "aa"], [0, 1, 2, 1])}
LENGTHS = ([1, 2, 3], [1, 2, 3])                            # bytes and code points per HANDLE, in both dictionaries
TABLES = (3, 2)                                             # n_needles; with 2, handle 2 is beyond the table
WORD_CLASS = b"aA"                                          # every byte of the texts is a word byte: only a haystack that IS a needle holds a whole word
SHAPES = ("one", "bytes", "wave")


def record_counts():
    tile, _ = am.api.score_geometry()
    chunk = am.api.needle_matrix_limits()["chunk_records"]
    return sorted({1, 63, 64, 65, tile // 4 - 1, tile // 4 + 1, tile - 1, tile, tile + 1, chunk - 1, chunk, chunk + 1})


def texts_of(shape, n, case):
    """n bytes of `a` (under IgnoreCase every other one `A`) as one haystack, as n haystacks of one byte, or as haystacks of 63, 64, 65, 63, ... bytes."""
    text = (b"aA" * n)[:n] if case else b"a" * n
    if shape == "one":
        return [text]
    if shape == "bytes":
        return [text[i:i + 1] for i in range(n)]
    out, at, k = [], 0, 0
    while at < n:
        out.append(text[at:at + 63 + k % 3])
        at += 63 + k % 3
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def automaton(name):
    needles, values = DICTS[name]
    return am.Automaton(needles, values)


@functools.lru_cache(maxsize=None)
def tables(name, nn):
    """Of a dictionary cut at nn handles: the values table, the span table, the whole-word span table, two weight columns (the first all ones), and as Weights the
    first column and both over the span table's values and both over the whole-word table's."""
    a = automaton(name)
    lengths = (LENGTHS[0][:nn], LENGTHS[1][:nn])
    plain = am.SpanTable(a, nn, lengths=lengths)
    words = am.SpanTable(a, nn, lengths=lengths, word_bytes=WORD_CLASS)
    columns = [[1] * nn, [3, -5, 7][:nn]]
    return am.ValuesTable(a, nn), plain, words, columns, am.Weights(plain.values, columns[:1]), am.Weights(plain.values, columns), am.Weights(words.values, columns)


@functools.lru_cache(maxsize=None)
def rule_per_needle(name, nn, case):
    """Rule r fires where slot r is set: the slot rows, read back bit by bit."""
    needles, values = DICTS[name]
    one = list(range(nn + 1))
    return am.RuleSet.from_program(case, needles, values, nn, one, one, list(range(nn)))


class Batch:
    """am_batch_upload of some texts, destroyed on exit."""

    def __init__(self, hays):
        self.s = am.api._Slices(hays)
        self.h = C.c_void_p()

    def __enter__(self):
        am.api.check(am.api.libam().am_batch_upload(self.s.arr, self.s.n, C.byref(self.h)))
        return self.h

    def __exit__(self, *exc):
        am.api.libam().am_batch_destroy(self.h)


@pytest.fixture(autouse=True)
def record_route():
    """containsAll and the slot rows folded from the records (k_idset), not set inside the scan."""
    am.debug_set("AM_NO_IDS_SCAN", 1)
    yield
    am.debug_set("AM_NO_IDS_SCAN", -1)


def same_csr(got, exp, what):
    assert got[0].tolist() == exp[0].tolist(), what
    assert got[1].dtype == exp[1].dtype and got[1].tobytes() == exp[1].tobytes(), what


def test_mirror_counts_records_and_values():
    """What the sizes below rest on, on the host mirror: a text of n `a`s gives n records and, for n >= 2, 3n - 3 values."""
    a = automaton("plain")
    for n in (1, 2, 3, 64, 65):
        _, pos, val = a.run_batch_with_case(0, [b"a" * n])
        assert len(np.unique(pos)) == n and len(val) == (3 * n - 3 if n >= 2 else 1)


@pytest.mark.parametrize("n", record_counts())
@pytest.mark.parametrize("shape", SHAPES)
def test_folds_agree(shape, n):
    lib = am.api.libam()
    for case in (0, 1):
        hays = texts_of(shape, n, case)
        n_hay = len(hays)
        assert sum(len(h) for h in hays) == n
        with Batch(hays) as b:
            for name in DICTS:
                a = automaton(name)
                hay, pos, val = a.run_batch_with_case(case, hays)
                assert len(np.unique(hay.astype(np.uint64) << np.uint64(32) | pos)) == n          # n records
                m = C.c_void_p()
                am.api.check(lib.am_run_batch(a.device, case, b, C.byref(m)))
                try:
                    assert int(lib.am_matches_size(m)) == n
                    for nn in TABLES:
                        check_table(name, nn, case, hays, b, m, (hay, pos, val), (shape, n, case, name, nn))
                finally:
                    lib.am_matches_free(m)


def check_table(name, nn, case, hays, b, m, steps, what):
    lib = am.api.libam()
    a = automaton(name)
    n_hay = len(hays)
    hay, pos, val = steps
    t, st, wt, columns, w1, w2, ww = tables(name, nn)
    kept = int((val < nn).sum())

    # ---- each stage against its host mirror
    counts = t.count_by_needle_batch(case, b)
    assert counts.tolist() == a.count_by_needle_host_mirror(case, hays, nn).tolist() == t.count_by_needle(m).tolist(), what
    matrix = t.count_matrix_batch(case, b)
    same_csr(matrix, a.count_matrix_host_mirror(case, hays, nn), what)
    same_csr(t.count_matrix(m, n_hay), matrix, what)
    exp_scores = a.score_host_mirror(case, hays, columns, nn)
    scores = w2.score_batch(case, b).scores
    assert scores.dtype == np.int64 and scores.tolist() == exp_scores.tolist(), what
    assert w2.score_matches(m, n_hay).scores.tolist() == exp_scores.tolist(), what
    ones = w1.score_batch(case, b).scores
    assert ones.tolist() == exp_scores[:1].tolist(), what
    spans = st.spans_batch(case, b, am.SPANS_ALL)
    same_csr(spans, a.spans_host_mirror(case, hays, n_values=nn, lengths=LENGTHS), what)
    rs = rule_per_needle(name, nn, case)
    hits = rs.eval_batch(b)
    fired, labels, rule_counts = rs.eval_host_mirror(hays)
    assert np.array_equal(hits.fired, fired) and np.array_equal(hits.labels, labels) and np.array_equal(hits.counts, rule_counts), what
    flags = np.zeros(max(n_hay, 1), np.uint8)
    am.api.check(lib.am_contains_all_batch(t.handle, case, b, flags.ctypes.data))
    present = np.zeros((n_hay, nn), bool)
    present[hay[val < nn], val[val < nn]] = True
    assert flags[:n_hay].astype(bool).tolist() == present.all(axis=1).tolist(), what
    sel = st.select_batch(case, b)
    assert sel.indices.tolist() == np.flatnonzero(present.any(axis=1)).tolist(), what

    # ---- the stages against each other
    assert int(counts.sum()) == int(matrix[1]["count"].sum()) == len(spans[1]) == int(ones.sum()) == kept, what
    assert counts.tolist() == np.bincount(spans[1]["needle"], minlength=nn).tolist(), what
    _, fold_counts = t.fold_hash(m, n_hay)
    assert int(fold_counts.sum()) == len(val), what         # every value, whatever the table keeps
    assert fold_counts.tolist() == np.bincount(hay, minlength=n_hay).tolist(), what
    pairs = np.zeros((nn, n_hay), bool)
    pairs[matrix[1]["needle"], matrix[1]["haystack"]] = True
    assert np.array_equal(hits.fired, pairs), what          # the slot rows' set bits = the matrix's non-empty (haystack, needle) pairs

    # ---- the whole-word forms: one span where the haystack is a needle of the table, nothing elsewhere
    exp_words = am.api.spans_fold_host(case, am.SPANS_ALL, steps, hays, LENGTHS[0][:nn], LENGTHS[1][:nn], word_bytes=WORD_CLASS)
    word_spans = wt.spans_batch(case, b, am.SPANS_ALL)
    same_csr(word_spans, exp_words, what)
    whole = [h for h, x in enumerate(hays) if 1 <= len(x) <= nn]
    twice = 2 if name == "shared" else 1                    # (the needle given twice reports its handle twice)
    assert word_spans[1]["haystack"].tolist() == [h for h in whole for _ in range(twice if len(hays[h]) == 2 else 1)], what
    word_counts = wt.count_by_needle_batch(case, b)
    assert word_counts.tolist() == np.bincount(word_spans[1]["needle"], minlength=nn).tolist(), what
    word_scores = wt.score_batch(case, b, ww).scores
    exp_word_scores = am.api.score_host(word_spans[1]["haystack"], word_spans[1]["needle"], n_hay, nn, columns)
    assert word_scores.tolist() == exp_word_scores.tolist() and int(word_scores[0].sum()) == len(word_spans[1]), what
    assert wt.select_batch(case, b).indices.tolist() == whole, what
