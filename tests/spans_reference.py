"""The definition of am_spans (include/am.h "match spans") in Python over oracle.Machine.run_list and oracle.skip_code_points_backwards: what the span tests expect.
Never another path of the library."""
from oracle import oracle

ALL, LEFTMOST_LONGEST = 0, 1


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def all_spans(machine, case, needles, text, n=None):
    """One (start, len, handle) per fold step `Match pos v` with v < n, in fold order: makeMatch (Replacer.hs:264-274) with the needle's own lengths."""
    text, nb = _b(text), [_b(x) for x in needles]
    n = len(nb) if n is None else n
    out = []
    for pos, v in zip(*(a.tolist() for a in machine.run_list(case, text))):
        if v >= n:
            continue                                       # the am_needle_ids convention: skipped
        if not nb[v]:
            start = pos                                    # a needle of length 0: start = pos, len = 0
        elif case == 0:
            start = pos - len(nb[v])
        else:
            start = oracle.skip_code_points_backwards(text, pos - 1, len(nb[v].decode("utf-8")) - 1)
        out.append((start, pos - start, v))
    return out


def leftmost_longest(spans):
    """cursor = 0; take the smallest start >= cursor, then the largest len, then the smallest handle; cursor = start + len.  Zero-length spans are never selected."""
    out, cursor = [], 0
    for s in sorted((s for s in spans if s[1] > 0), key=lambda s: (s[0], -s[1], s[2])):      # in this order the first span at or after the cursor is the one to take
        if s[0] >= cursor:
            out.append(s)
            cursor = s[0] + s[1]
    return out


def spans(machine, case, mode, needles, hays, n=None):
    """Per haystack, the list of (start, len, handle); `machine` = oracle.Machine(needles, values) whose handle v stands for needles[v]."""
    rows = [all_spans(machine, case, needles, h, n) for h in hays]
    return [leftmost_longest(r) for r in rows] if mode == LEFTMOST_LONGEST else rows
