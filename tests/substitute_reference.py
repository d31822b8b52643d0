"""The definition of am_substitute (include/am.h "substitute") in Python: spans_reference.spans(..., LEFTMOST_LONGEST, ...) over the oracle, then the splice
`replace` (Replacer.hs:163-180) -- what the substitute tests expect.  Never another path of the library.  regex_substitute is an independent second check for
AM_CASE_SENSITIVE with Python's `re` over bytes."""
import re

from tests import spans_reference as ref


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def splice(text, row, replacements):
    """out = hay[0, s_1) ++ repl[v_1] ++ hay[s_1 + l_1, s_2) ++ ... ++ repl[v_k] ++ hay[s_k + l_k, len) for the (start, len, handle) rows of one haystack."""
    text, parts, cursor = _b(text), [], 0
    for start, n, v in row:
        assert start >= cursor and n > 0 and start + n <= len(text)
        parts += [text[cursor:start], _b(replacements[v])]
        cursor = start + n
    parts.append(text[cursor:])
    return b"".join(parts)


def substitute(machine, case, needles, hays, replacements, n=None):
    """Per haystack, the rewritten bytes; `machine` = oracle.Machine(needles, values) whose handle v stands for needles[v] and is replaced by replacements[v]."""
    rows = ref.spans(machine, case, ref.LEFTMOST_LONGEST, needles, hays, n)
    return [splice(h, r, replacements) for h, r in zip(hays, rows)]


def regex_substitute(needles, hays, replacements):
    """AM_CASE_SENSITIVE, handle = needle index: the alternation of the escaped non-empty needles ordered by (-len, handle) -- at a start `re` takes the first
    alternative that matches, the longest -- and the replacement of a match is that of the smallest handle with those bytes."""
    nb = [_b(x) for x in needles]
    order = sorted((v for v in range(len(nb)) if nb[v]), key=lambda v: (-len(nb[v]), v))
    if not order:
        return [_b(h) for h in hays]
    first = {}
    for v in range(len(nb)):
        first.setdefault(nb[v], v)
    rx = re.compile(b"|".join(re.escape(nb[v]) for v in order), re.S)
    return [rx.sub(lambda m: _b(replacements[first[m.group(0)]]), _b(h)) for h in hays]
