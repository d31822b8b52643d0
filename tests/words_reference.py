"""The definition of whole-word matching (include/am.h "whole words") in Python: spans_reference.all_spans filtered by the whole-word rule, THEN
spans_reference.leftmost_longest; substitute on top as substitute_reference does it; the term counts as a bincount of the filtered rows.  What the whole-word tests
expect -- never another path of the library.  regex_spans / regex_substitute are an independent second check for AM_CASE_SENSITIVE and the default class with Python's
`re` over bytes."""
import re

from tests import spans_reference as ref
from tests import substitute_reference as sref

ALL, LEFTMOST_LONGEST = ref.ALL, ref.LEFTMOST_LONGEST

DEFAULT_CLASS = frozenset(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_") | frozenset(range(0x80, 0x100))
LOWER_CLASS = frozenset(b"abcdefghijklmnopqrstuvwxyz")               # a-z only: digits, capitals and non-ASCII bytes separate
EMPTY_CLASS = frozenset()                                            # nothing is a word byte: every span is a whole word
FULL_CLASS = frozenset(range(256))                                   # everything is: only a span that is its whole haystack is one
CLASSES = {"default": DEFAULT_CLASS, "lower": LOWER_CLASS, "empty": EMPTY_CLASS, "full": FULL_CLASS}


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def flags(cls):
    """The class as the 256 flags of the C ABI."""
    return bytes(1 if b in cls else 0 for b in range(256))


def whole_word(text, start, n, cls):
    """(start == 0 or hay[start - 1] not in W) and (start + len == L or hay[start + len] not in W); the span's own bytes are not looked at."""
    return (start == 0 or text[start - 1] not in cls) and (start + n == len(text) or text[start + n] not in cls)


def all_spans(machine, case, needles, text, cls, n=None):
    text = _b(text)
    return [s for s in ref.all_spans(machine, case, needles, text, n) if whole_word(text, s[0], s[1], cls)]


def spans(machine, case, mode, needles, hays, cls, n=None):
    """Per haystack, the list of (start, len, handle): filter, then select."""
    rows = [all_spans(machine, case, needles, h, cls, n) for h in hays]
    return [ref.leftmost_longest(r) for r in rows] if mode == LEFTMOST_LONGEST else rows


def select_then_filter(machine, case, needles, hays, cls, n=None):
    """The WRONG order -- the plain leftmost-longest selection filtered afterwards -- for tests that show the two differ."""
    out = []
    for h in hays:
        t = _b(h)
        out.append([s for s in ref.leftmost_longest(ref.all_spans(machine, case, needles, t, n)) if whole_word(t, s[0], s[1], cls)])
    return out


def substitute(machine, case, needles, hays, replacements, cls, n=None):
    rows = spans(machine, case, LEFTMOST_LONGEST, needles, hays, cls, n)
    return [sref.splice(h, r, replacements) for h, r in zip(hays, rows)]


def counts(machine, case, needles, hays, cls, n=None):
    """counts[v] = the AM_SPANS_ALL rows with needle v over the whole batch."""
    n = len(needles) if n is None else n
    out = [0] * n
    for row in spans(machine, case, ALL, needles, hays, cls, n):
        for _, _, v in row:
            out[v] += 1
    return out


# ---- Python's re: AM_CASE_SENSITIVE, the default class, handle = needle index

WORD = rb"[0-9A-Za-z_\x80-\xff]"


def _regex(needles):
    nb = [_b(x) for x in needles]
    order = sorted((v for v in range(len(nb)) if nb[v]), key=lambda v: (-len(nb[v]), v))
    first = {}
    for v in range(len(nb)):
        first.setdefault(nb[v], v)
    if not order:
        return None, first
    return re.compile(rb"(?<!" + WORD + rb")(?:" + b"|".join(re.escape(nb[v]) for v in order) + rb")(?!" + WORD + rb")", re.S), first


def regex_spans(needles, hays):
    """Leftmost-longest whole-word rows per haystack: at a start `re` tries the alternatives longest first and backtracks into a shorter one when the look-ahead
    fails -- the longest WHOLE-WORD needle of that start, which is filter-then-select."""
    rx, first = _regex(needles)
    if rx is None:
        return [[] for _ in hays]
    return [[(m.start(), m.end() - m.start(), first[m.group(0)]) for m in rx.finditer(_b(h))] for h in hays]


def regex_substitute(needles, hays, replacements):
    rx, first = _regex(needles)
    if rx is None:
        return [_b(h) for h in hays]
    return [rx.sub(lambda m: _b(replacements[first[m.group(0)]]), _b(h)) for h in hays]
