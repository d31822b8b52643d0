"""The definition of am_postings (include/am.h "postings") in plain Python over per-haystack (start, len, handle) rows: sorted() by needle, which is stable, Python
integers, no library call.  The rows come from tests/spans_reference.py (the oracle's fold steps, all of them or leftmost-longest) or tests/words_reference.py.  What
the postings tests expect -- never another path of the library."""
from oracle import oracle
from tests import spans_reference as sref

ALL, LEFTMOST_LONGEST = sref.ALL, sref.LEFTMOST_LONGEST


def machine(needles, values=None):
    return oracle.Machine(list(needles), values)


def rows_of(needles, case, hays, mode=ALL, values=None, n=None):
    """Per haystack the (start, len, handle) rows, in fold order or the leftmost-longest selection."""
    return sref.spans(machine(needles, values), case, mode, needles, hays, n)


def flat(rows):
    """The data array of a spans result: (start, len, haystack, needle) in row order."""
    return [(s, n, h, v) for h, r in enumerate(rows) for s, n, v in r]


def postings(rows, n_needles):
    """(offsets [n_needles + 1], data [(start, len, haystack, needle)], source [row of the spans], doc_freq [n_needles]) of per-haystack rows."""
    s = flat(rows)
    assert all(x[3] < n_needles for x in s)
    perm = sorted(range(len(s)), key=lambda i: s[i][3])     # (stable)
    data = [s[i] for i in perm]
    offsets = [sum(1 for x in s if x[3] < v) for v in range(n_needles + 1)] if n_needles <= 64 else _offsets(data, n_needles)
    doc_freq = [0] * n_needles
    for k, x in enumerate(data):
        if k == offsets[x[3]] or data[k - 1][2] != x[2]:
            doc_freq[x[3]] += 1
    return offsets, data, perm, doc_freq


def postings_sparse(rows):
    """The same for a needle count too large to walk in Python: (data, source, {needle: doc_freq of a row that is not empty}).  The offsets of such a table are
    the lower bounds of 0 .. n_needles in data's needle column, which ascends."""
    s = flat(rows)
    perm = sorted(range(len(s)), key=lambda i: s[i][3])     # (stable)
    data = [s[i] for i in perm]
    doc_freq = {}
    for k, x in enumerate(data):
        if k == 0 or data[k - 1][3] != x[3] or data[k - 1][2] != x[2]:
            doc_freq[x[3]] = doc_freq.get(x[3], 0) + 1
    return data, perm, doc_freq


def _offsets(data, n_needles):
    out, k = [], 0
    for v in range(n_needles + 1):
        while k < len(data) and data[k][3] < v:
            k += 1
        out.append(k)
    return out


def spans_of(rows, needle):
    """Row `needle` as per-haystack rows: (offsets [n_hay + 1], [(start, len, haystack, needle)]), and the filtered per-haystack rows themselves."""
    kept = [[x for x in r if x[2] == needle] for r in rows]
    offsets = [0]
    for r in kept:
        offsets.append(offsets[-1] + len(r))
    return offsets, flat(kept), kept
