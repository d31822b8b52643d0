"""The definition of scores (include/am.h "scores") in Python.  score[c][i] = the sum of W[c][v] over the fold steps `Match _ v` of runWithCase over haystack i with
v < n -- oracle.Machine(needles, values).run_list(case, h)[1] -- in Python integers, wrapped to int64 at the end (modulo 2^64, two's complement: what the reference's
Int does).  The whole-word form sums over the rows of tests/words_reference.py.  Top-k is sorted() with the key the header states.  What the score tests expect --
never another path of the library."""
import numpy as np

from oracle import oracle
from tests import words_reference as wref

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def wrap(x):
    """A Python integer modulo 2^64 as the int64 with that bit pattern."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= 1 << 63 else x


def machine(needles, values=None):
    needles = list(needles)
    return oracle.Machine(needles, None if values is None else list(values)) if needles else None


def steps(m, case, hay):
    """The values of the fold steps over one haystack, in fold order."""
    return [int(v) for v in m.run_list(case, _b(hay))[1]] if m is not None else []


def of_steps(rows, weights, n):
    """np.int64[n_cols, n_hay] of per-haystack value lists: values >= n are skipped."""
    out = np.zeros((len(weights), len(rows)), np.int64)
    for i, vs in enumerate(rows):
        for c, col in enumerate(weights):
            out[c, i] = wrap(sum(int(col[v]) for v in vs if v < n))
    return out


def expect(needles, values, n, case, weights, hays):
    """The scores of weights (a list of columns of n Python integers) over hays."""
    m = machine(needles, values)
    return of_steps([steps(m, case, h) for h in hays], weights, n)


def expect_words(needles, n, case, weights, hays, cls):
    """... over the whole-word rows only (handle = needle index)."""
    m = machine(needles)
    rows = wref.spans(m, case, wref.ALL, needles, hays, cls, n) if m is not None else [[] for _ in hays]
    return of_steps([[v for _, _, v in row] for row in rows], weights, n)


def top_k(column, k, largest=True):
    """[(score, haystack)]: the first min(k, n) of (score descending, haystack ascending), or of (score ascending, haystack ascending)."""
    order = sorted(range(len(column)), key=lambda i: ((-int(column[i])) if largest else int(column[i]), i))
    return [(int(column[i]), i) for i in order[:max(0, min(int(k), len(column)))]]


def in_range(column, lo, hi, invert=False):
    """The ascending haystacks with lo <= score <= hi, or -- invert -- the others."""
    return [i for i in range(len(column)) if (lo <= int(column[i]) <= hi) != bool(invert)]


def random_weights(rng, n, n_cols, big=3):
    """n_cols columns of n weights in +-2^20 with a few at +-2^62 and one at -2^63."""
    cols = []
    for _ in range(n_cols):
        col = [rng.randint(-2 ** 20, 2 ** 20) for _ in range(n)]
        for _ in range(min(big, n)):
            col[rng.randrange(n)] = rng.choice([2 ** 62, -2 ** 62, INT64_MIN, INT64_MAX])
        cols.append(col)
    return cols
