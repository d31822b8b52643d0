"""The definition of extract (include/am.h "extract") in Python, a byte at a time, over the rows of tests/spans_reference.py and tests/words_reference.py: what the
extract tests expect -- never another path of the library.  regex_snippets is an independent second opinion for valid UTF-8 under AM_CASE_SENSITIVE leftmost-longest
with Python's `re` over `str`, whose slices count code points."""
import re

from tests import spans_reference as ref
from tests import words_reference as wref

EACH, MERGED = 0, 1


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def is_start(b):
    return (b & 0xC0) != 0x80


def window(text, s, l, before, after):
    """[ws, we) of the span (s, l): ws = the before-th START byte among the indices < s, counted leftwards (fewer: 0; before == 0: s); we = the after-th START byte
    among the indices > s + l, counted rightwards (fewer: len(text); after == 0: s + l)."""
    e = s + l
    assert 0 <= s <= e <= len(text)
    ws, we = s, e
    if before > 0:
        ws, seen = 0, 0
        for i in range(s - 1, -1, -1):
            if is_start(text[i]):
                seen += 1
                if seen == before:
                    ws = i
                    break
    if after > 0:
        we, seen = len(text), 0
        for i in range(e + 1, len(text)):
            if is_start(text[i]):
                seen += 1
                if seen == after:
                    we = i
                    break
    return ws, we


def windows(text, spans, before, after):
    """One (start, len) per span, in the spans' order (AM_EXTRACT_EACH); spans = rows (start, len, ...) of one haystack."""
    text = _b(text)
    out = []
    for sp in spans:
        ws, we = window(text, sp[0], sp[1], before, after)
        out.append((ws, we - ws))
    return out


def merged(text, spans, before, after):
    """The union of the windows of one haystack as disjoint ascending (start, len) pieces (AM_EXTRACT_MERGED): window i joins the piece of window i - 1 iff
    ws_i <= we_{i-1}; spans = leftmost-longest rows (ascending, not overlapping)."""
    text = _b(text)
    pieces, cursor = [], 0
    for sp in spans:
        assert sp[0] >= cursor, "merged takes rows that ascend and do not overlap"
        cursor = sp[0] + sp[1]
        ws, we = window(text, sp[0], sp[1], before, after)
        if pieces and ws <= pieces[-1][1]:
            assert we >= pieces[-1][1]
            pieces[-1][1] = we
        else:
            pieces.append([ws, we])                        # (the first span of a haystack always opens a piece: `pieces` is this haystack's own)
    return [(a, z - a) for a, z in pieces]


def fragments(hays, rows, before, after, mode):
    """(offsets, [(start, len)], [snippet bytes]) over a batch: rows[i] = the spans of hays[i]."""
    offs, frags, texts = [0], [], []
    for h, r in zip(hays, rows):
        h = _b(h)
        fr = merged(h, r, before, after) if mode == MERGED else windows(h, r, before, after)
        frags.extend(fr)
        texts.extend(h[a:a + n] for a, n in fr)
        offs.append(len(frags))
    return offs, frags, texts


def extract(machine, case, spans_mode, needles, hays, before, after, mode, cls=None, n=None):
    """fragments() over the definition's own rows: spans_reference.spans, or words_reference.spans with a word class."""
    rows = ref.spans(machine, case, spans_mode, needles, hays, n) if cls is None else wref.spans(machine, case, spans_mode, needles, hays, cls, n)
    return fragments(hays, rows, before, after, mode)


def new_batch(texts):
    """(offsets, concatenated bytes) of the batch with one haystack per snippet."""
    offs = [0]
    for t in texts:
        offs.append(offs[-1] + len(t))
    return offs, b"".join(texts)


# ---- Python's re over str: AM_CASE_SENSITIVE, leftmost-longest, valid UTF-8, AM_EXTRACT_EACH

def _regex(needles, whole_words=False):
    """The alternation as words_reference._regex builds it -- the non-empty needles, longest first, then by handle -- over str."""
    ns = [x if isinstance(x, str) else bytes(x).decode("utf-8") for x in needles]
    order = sorted((v for v in range(len(ns)) if ns[v]), key=lambda v: (-len(ns[v].encode("utf-8")), v))
    if not order:
        return None
    alt = "(?:" + "|".join(re.escape(ns[v]) for v in order) + ")"
    if whole_words:                                        # the default class on str: ASCII word characters and every non-ASCII code point
        word = r"[0-9A-Za-z_\u0080-\U0010ffff]"
        alt = "(?<!" + word + ")" + alt + "(?!" + word + ")"
    return re.compile(alt, re.S)


def regex_snippets(needles, hays, before, after, whole_words=False):
    """Per haystack (str), the snippets of the leftmost-longest matches: text[max(0, m.start() - before) : m.end() + after], encoded."""
    rx = _regex(needles, whole_words)
    out = []
    for h in hays:
        h = h if isinstance(h, str) else bytes(h).decode("utf-8")
        out.append([] if rx is None else [h[max(0, m.start() - before):m.end() + after].encode("utf-8") for m in rx.finditer(h)])
    return out
