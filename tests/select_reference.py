"""The definition of select (include/am.h "select") in Python: which haystacks a predicate keeps, and the batch they form.  The predicates are built over
oracle.Machine.run_list (containsAny: the fold meets a value; containsAll: it meets every needle id) and over tests/spans_reference.py / tests/words_reference.py
(a non-empty AM_SPANS_ALL row).  What the select tests expect -- never another path of the library."""
import numpy as np

from oracle import oracle
from tests import spans_reference as sref
from tests import words_reference as wref


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def keep(pred, invert, hays):
    """keep[i] = pred(haystack i) != invert: (indices, texts) of the kept haystacks, in order."""
    idx = [i for i, h in enumerate(hays) if bool(pred(_b(h))) != bool(invert)]
    return idx, [_b(hays[i]) for i in idx]


def offsets(texts):
    """The offsets of the batch the kept texts form: the running sum of their lengths."""
    return np.cumsum([0] + [len(_b(t)) for t in texts]).astype(np.uint64)


def pred_any(needles, case):
    """Searcher.containsAny (Searcher.hs:156-164): the fold over the haystack meets a value."""
    m = oracle.Machine(list(needles))
    return lambda h: len(m.run_list(case, h)[0]) > 0


def pred_all(needles, case):
    """Searcher.containsAll (Searcher.hs:173-187): the fold deletes every needle id it meets from [0 .. n - 1]; true iff nothing is left.  Zero needles: true (IS.null
    of the empty set).  An automaton of [""] alone has no transition and its fold meets nothing: never contained (AhoCorasickSpec.hs:196-200)."""
    needles = list(needles)
    if not needles:
        return lambda h: True
    m = oracle.Machine(needles, list(range(len(needles))))
    return lambda h: set(range(len(needles))) <= set(int(v) for v in m.run_list(case, h)[1])


def pred_spans(needles, case, cls=None, n=None):
    """Row i of AM_SPANS_ALL is not empty: a span of a needle with handle < n, with a word class `cls` (a set of byte values) a whole-word one."""
    needles = list(needles)
    m = oracle.Machine(needles, list(range(len(needles))))
    if cls is None:
        return lambda h: len(sref.all_spans(m, case, needles, h, n)) > 0
    return lambda h: len(wref.all_spans(m, case, needles, h, cls, n)) > 0
