"""The definition of am_substitute with TEMPLATES (include/am.h "substitute templates") in Python: spans_reference.spans(..., LEFTMOST_LONGEST, ...) over the oracle
-- with a word class: words_reference.spans -- then the splice with T(v, m) in the place of repl[v]: the segments of template v in order, a literal's bytes, or the
matched bytes m for a MATCH segment.  What the template tests expect; never another path of the library.  A segment is bytes / str (a literal) or anything else (the
MATCH marker: the tests pass am.MATCH); a template is a list or tuple of segments, a plain bytes / str the template of that one literal.  regex_substitute is an
independent second check with Python's `re` over bytes and the template translated to \\g<0>."""
import re

from tests import spans_reference as ref


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def is_literal(seg):
    return isinstance(seg, (bytes, bytearray, str))


def segments(template):
    return list(template) if isinstance(template, (list, tuple)) else [template]


def expand(template, matched):
    """T(v, m): the segments in order, a literal's bytes or m."""
    return b"".join(_b(seg) if is_literal(seg) else matched for seg in segments(template))


def splice(text, row, templates):
    """out = hay[0, s_1) ++ T(v_1, hay[s_1, s_1 + l_1)) ++ hay[s_1 + l_1, s_2) ++ ... ++ hay[s_k + l_k, len) for the (start, len, handle) rows of one haystack."""
    text, parts, cursor = _b(text), [], 0
    for start, n, v in row:
        assert start >= cursor and n > 0 and start + n <= len(text)
        parts += [text[cursor:start], expand(templates[v], text[start:start + n])]
        cursor = start + n
    parts.append(text[cursor:])
    return b"".join(parts)


def substitute(machine, case, needles, hays, templates, n=None, cls=None):
    """Per haystack, the rewritten bytes; `machine` = oracle.Machine(needles, values) whose handle v stands for needles[v] and has templates[v].  cls: a word class as
    words_reference takes it (None: no class)."""
    if cls is None:
        rows = ref.spans(machine, case, ref.LEFTMOST_LONGEST, needles, hays, n)
    else:
        from tests import words_reference as wref
        rows = wref.spans(machine, case, ref.LEFTMOST_LONGEST, needles, hays, cls, n)
    return [splice(h, r, templates) for h, r in zip(hays, rows)]


def regex_template(template):
    """The template as a replacement string of re.sub over bytes: literals escaped, MATCH = \\g<0>."""
    return b"".join(_b(seg).replace(b"\\", b"\\\\") if is_literal(seg) else b"\\g<0>" for seg in segments(template))


def regex_substitute(needles, hays, templates, ignore_case=False):
    """Handle = needle index: the alternation of the escaped non-empty needles ordered by (-len, handle) -- at a start `re` takes the first alternative that matches,
    the longest -- and the template of a match is that of the smallest handle with those bytes (lower-cased under ignore_case: ASCII-only texts and needles)."""
    nb = [_b(x) for x in needles]
    order = sorted((v for v in range(len(nb)) if nb[v]), key=lambda v: (-len(nb[v]), v))
    if not order:
        return [_b(h) for h in hays]
    key = (lambda x: x.lower()) if ignore_case else (lambda x: x)
    first = {}
    for v in range(len(nb)):
        first.setdefault(key(nb[v]), v)
    rx = re.compile(b"|".join(re.escape(nb[v]) for v in order), re.S | (re.I if ignore_case else 0))
    return [rx.sub(lambda m: m.expand(regex_template(templates[first[key(m.group(0))]])), _b(h)) for h in hays]
