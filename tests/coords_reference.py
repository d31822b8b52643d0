"""The definition of the coordinates stage (include/am.h "coordinates") as the tests hold it: byte loops over one haystack, a numpy form of the same counts for the
long texts, and -- for valid UTF-8 at code point boundaries -- Python's own str operations.  Nothing here calls the library.

A haystack is `bytes`; a position p is relative to it, 0 <= p <= len(hay).  Bytes outside hay[:p] never count: the caller cuts the haystack out of its batch."""
import numpy as np

BYTES, CODE_POINTS, UTF16 = 0, 1, 2
UNITS = (BYTES, CODE_POINTS, UTF16)


# ---- the byte loops

def cp_loop(hay, p):
    return sum(1 for b in hay[:p] if (b & 0xC0) != 0x80)


def u16_loop(hay, p):
    return cp_loop(hay, p) + sum(1 for b in hay[:p] if b >= 0xF0)


def line_loop(hay, p):
    return sum(1 for b in hay[:p] if b == 0x0A)


def linestart_loop(hay, p):
    at = 0
    for i in range(p):
        if hay[i] == 0x0A:
            at = i + 1
    return at


# ---- the same counts without a Python loop per byte (the long lines of the binary-search tests); tests/test_coords_cpu.py holds them to the loops

def _arr(hay):
    return hay if isinstance(hay, np.ndarray) else np.frombuffer(hay, np.uint8)


def cp(hay, p):
    return int(np.count_nonzero((_arr(hay)[:p] & 0xC0) != 0x80))


def u16(hay, p):
    return cp(hay, p) + int(np.count_nonzero(_arr(hay)[:p] >= 0xF0))


def line(hay, p):
    return int(np.count_nonzero(_arr(hay)[:p] == 0x0A))


def linestart(hay, p):
    at = np.flatnonzero(_arr(hay)[:p] == 0x0A)
    return int(at[-1]) + 1 if len(at) else 0


def units(hay, p, unit):
    return p if unit == BYTES else cp(hay, p) if unit == CODE_POINTS else u16(hay, p)


def col(hay, p, unit):
    return units(hay, p, unit) - units(hay, linestart(hay, p), unit)


def span(hay, start, length, unit):
    """(U(start), U(start + len) - U(start))"""
    return units(hay, start, unit), units(hay, start + length, unit) - units(hay, start, unit)


def span_range(hay, start, length, unit):
    """(start_line, start_col, end_line, end_col) of a span, the columns in `unit`"""
    return line(hay, start), col(hay, start, unit), line(hay, start + length), col(hay, start + length, unit)


def convert_rows(hays, rows, unit):
    """rows: per haystack a list of (start, len, ...) in bytes -> (offsets, [(start, len)] in unit, [(sl, sc, el, ec)])"""
    offs, spans, ranges = [0], [], []
    for h, r in zip(hays, rows):
        h = h.encode("utf-8") if isinstance(h, str) else bytes(h)
        for row in r:
            spans.append(span(h, row[0], row[1], unit))
            ranges.append(span_range(h, row[0], row[1], unit))
        offs.append(len(spans))
    return offs, spans, ranges


class Table:
    """The same definition for MANY positions of one long haystack: running counts once, then a lookup per position (numpy arrays of positions in, arrays out)."""

    def __init__(self, hay):
        a = _arr(hay)
        self.n = len(a)
        self.start = np.concatenate([[0], np.cumsum((a & 0xC0) != 0x80, dtype=np.int64)])
        self.four = np.concatenate([[0], np.cumsum(a >= 0xF0, dtype=np.int64)])
        self.newline = np.concatenate([[0], np.cumsum(a == 0x0A, dtype=np.int64)])
        self.newline_at = np.flatnonzero(a == 0x0A).astype(np.int64)

    def units(self, p, unit):
        p = np.asarray(p, np.int64)
        return p if unit == BYTES else self.start[p] if unit == CODE_POINTS else self.start[p] + self.four[p]

    def line(self, p):
        return self.newline[np.asarray(p, np.int64)]

    def linestart(self, p):
        k = self.line(p)                                    # the newlines before p: the last of them is newline_at[k - 1]
        return np.where(k > 0, self.newline_at[np.maximum(k, 1) - 1] + 1, 0) if len(self.newline_at) else np.zeros_like(k)

    def col(self, p, unit):
        return self.units(p, unit) - self.units(self.linestart(p), unit)

    def spans(self, start, length, unit):
        """(start, len) columns in unit and the four range columns, for arrays of byte spans"""
        start, end = np.asarray(start, np.int64), np.asarray(start, np.int64) + np.asarray(length, np.int64)
        us, ue = self.units(start, unit), self.units(end, unit)
        return us, ue - us, self.line(start), self.col(start, unit), self.line(end), self.col(end, unit)


# ---- valid text: Python's own opinion.  s is a str, i an index into it (a code point boundary); p the byte position of that boundary

def str_cp(s, i):
    return i


def str_u16(s, i):
    return len(s[:i].encode("utf-16-le")) // 2


def str_line(s, i):
    return s.count("\n", 0, i)


def str_col(s, i, unit):
    at = s.rfind("\n", 0, i) + 1
    return {BYTES: len(s[at:i].encode("utf-8")), CODE_POINTS: i - at, UTF16: len(s[at:i].encode("utf-16-le")) // 2}[unit]
