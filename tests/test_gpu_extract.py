"""Extract on the device (am_fragments_from_spans / am_extract_batch / am_extract, csrc/am_extract.hip) against the definition.  Every check compares the fragments,
their offsets, every byte of the new batch and its zero padding up to round_up(total, 16) with what tests/extract_reference.py says -- a byte at a time over the
oracle's rows, Python slices or literals -- never with another path of the library.  Shapes sit on the real seams: every residue of a haystack's base and of a match's
start modulo the 16-byte group of the walk, the exclusive sum's block and its one-launch limit, byte 2^32."""
import ctypes as C
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import extract_reference as xref, spans_reference as ref, words_reference as wref

pytestmark = pytest.mark.gpu

ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}
KELVIN = "\u212a"
EACH, MERGED = xref.EACH, xref.MERGED
ALL, LL = ref.ALL, ref.LEFTMOST_LONGEST


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield ROUTES[request.param]
    am.debug_set("AM_DFA", -1)


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def lib():
    return am.api.libam()


class Batch:
    def __init__(self, hays):
        self.s = am.api._Slices(hays)
        self.h = C.c_void_p()

    def __enter__(self):
        am.api.check(lib().am_batch_upload(self.s.arr, self.s.n, C.byref(self.h)))
        return self.h

    def __exit__(self, *exc):
        lib().am_batch_destroy(self.h)


class Borrowed:
    """am_batch_from_device over a torch tensor whose bytes from total to round_up(total, 16) are `pad`, not zero."""

    def __init__(self, hays, pad=0x41):
        import torch
        hays = [_b(h) for h in hays]
        text = b"".join(hays)
        padded = (len(text) + 15) // 16 * 16
        self.text = torch.full((max(padded, 16),), pad, dtype=torch.uint8, device="cuda:0")
        if text:
            self.text[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
        self.offs = torch.tensor(np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.int64), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        self.n, self.total = len(hays), len(text)
        self.h = C.c_void_p()

    def __enter__(self):
        am.api.check(lib().am_batch_from_device(self.text.data_ptr(), self.offs.data_ptr(), self.n, self.total, C.byref(self.h)))
        return self.h

    def __exit__(self, *exc):
        lib().am_batch_destroy(self.h)


def read_batch(nb):
    """(offsets, text) of a batch handle; the text is read to round_up(total, 16) -- through a borrowed batch of one haystack over the same memory -- and the bytes
    beyond total must be zero."""
    import torch
    offs = am.api.batch_offsets(nb)
    total = int(offs[-1])
    assert lib().am_batch_total_bytes(nb) == total and lib().am_batch_haystacks(nb) == len(offs) - 1
    padded = (total + 15) // 16 * 16
    if padded == 0:
        return offs, b""
    text_ptr = lib().am_batch_device_text(nb)
    assert text_ptr and text_ptr % 16 == 0
    o = torch.tensor([0, padded], dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    x = C.c_void_p()
    am.api.check(lib().am_batch_from_device(text_ptr, o.data_ptr(), 1, padded, C.byref(x)))
    try:
        whole = am.api.batch_read_text(x, 0, padded)
    finally:
        lib().am_batch_destroy(x)
    assert whole[total:] == bytes(padded - total), ("padding", whole[total:])
    return offs, whole[:total]


def table(needles, cls=None, route=0, n=None):
    a = am.Automaton(needles)
    a.set_kernel(route)
    return am.api.SpanTable(a, n, word_bytes=None if cls is None else sorted(cls))


class Spans:
    """am_spans_batch, raw: one spans call serves many (before, after, mode)."""

    def __init__(self, t, case, spans_mode, b):
        self.t, self.b = t, b
        self.h = t.spans_batch(case, b, spans_mode, raw=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        lib().am_spans_free(self.h)

    def stage(self, before, after, mode):
        """am_fragments_from_spans, then am_batch_from_fragments: (offsets, [(start, len)], new offsets, new text)."""
        f = self.t.fragments_from_spans(self.b, self.h, before, after, mode == MERGED, raw=True)
        try:
            offs, frags = am.api.fragments_to_numpy(f)
            assert lib().am_fragments_size(f) == len(frags) and lib().am_fragments_haystacks(f) == len(offs) - 1
            nb = C.c_void_p()
            am.api.check(lib().am_batch_from_fragments(self.b, f, C.byref(nb)))
        finally:
            lib().am_fragments_free(f)
        try:
            new_offs, new_text = read_batch(nb)
        finally:
            lib().am_batch_destroy(nb)
        return offs, frags, new_offs, new_text


def same(got, want_offs, want_frags, want_texts, what):
    """The fragments, their offsets, the new batch's offsets, every byte of it (read_batch has looked at the padding)."""
    offs, frags, new_offs, new_text = got
    assert np.array_equal(np.asarray(offs, np.int64), np.asarray(want_offs, np.int64)), (what, "offsets", np.asarray(offs)[:12].tolist(), list(want_offs)[:12])
    got_frags = list(zip(frags["start"].tolist(), frags["len"].tolist()))
    if got_frags != list(want_frags):
        k = next((j for j in range(min(len(got_frags), len(want_frags))) if got_frags[j] != want_frags[j]), min(len(got_frags), len(want_frags)))
        raise AssertionError((what, "fragment", k, len(got_frags), len(want_frags), got_frags[k:k + 3], list(want_frags)[k:k + 3]))
    e_offs, e_text = xref.new_batch(want_texts)
    assert np.array_equal(np.asarray(new_offs, np.int64), np.asarray(e_offs, np.int64)), (what, "new offsets")
    if new_text != e_text:
        k = next((j for j in range(min(len(new_text), len(e_text))) if new_text[j] != e_text[j]), min(len(new_text), len(e_text)))
        raise AssertionError((what, "byte", k, new_text[max(0, k - 8):k + 24], e_text[max(0, k - 8):k + 24]))


def check(sp, hays, rows, before, after, mode, what=None):
    same(sp.stage(before, after, mode), *xref.fragments(hays, rows, before, after, mode), (what, before, after, mode))


def x_rows(hays):
    """The spans of the one needle x, by the definition: every x, one byte."""
    return [[(i, 1, 0) for i, c in enumerate(_b(h)) if c == 0x78] for h in hays]


# ---- 1. the group walk: every residue of the base and of the match's start, every width around the group, both clamps

WIDTHS = (0, 1, 2, 15, 16, 17, 33)
FILLERS = {"1 byte": ["a"], "2 bytes": ["é"], "3 bytes": ["€"], "4 bytes": ["\U0001f600"], "mixture": ["a", "é", "€", "\U0001f600", "b", KELVIN]}
# code points before and after the x: a window of 15 / 16 / 17 is one short of the haystack's end, reaches it exactly, goes beyond
AROUND = [(16, 16), (1, 17), (17, 2), (20, 15), (0, 33), (33, 0), (15, 1), (2, 34)]


def residue_case(filler):
    rng = random.Random(len(filler))
    hays = []
    for pad in range(16):
        hays.append("A" * pad)                             # a pad haystack of every length 0 .. 15, all START bytes
        nb, na = AROUND[pad % len(AROUND)]
        hays.append("".join(rng.choice(filler) for _ in range(nb)) + "x" + "".join(rng.choice(filler) for _ in range(na)))
    return hays


@pytest.mark.parametrize("name", sorted(FILLERS))
def test_group_walk_at_every_residue(name):
    hays = residue_case(FILLERS[name])
    rows = x_rows(hays)
    bases = np.concatenate([[0], np.cumsum([len(_b(h)) for h in hays])])
    starts = {int(bases[i] + r[0][0]) % 16 for i, r in enumerate(rows) if r}
    if len(FILLERS[name]) == 1:
        assert len({int(bases[i]) % 16 for i, r in enumerate(rows) if r}) >= 8 and len(starts) >= 8, "the bases and the starts spread over the residues"
    t = table(["x"])
    with Batch(hays) as b, Spans(t, 0, LL, b) as sp:
        for before in WIDTHS:
            for after in WIDTHS:
                check(sp, hays, rows, before, after, EACH, name)
        for before, after in ((0, 0), (16, 17), (33, 33)):
            check(sp, hays, rows, before, after, MERGED, name)      # one span per haystack: the same windows, a piece each


def test_group_walk_hits_all_sixteen_residues():
    """One x at every offset 0 .. 15 of a group behind a base at every residue: 256 (base, start) pairs in one batch, three-byte filler."""
    hays = []
    for base in range(16):
        for at in range(16):
            hays.append("A" * ((base - sum(len(_b(h)) for h in hays)) % 16))
            hays.append("€" * 6 + "a" * at + "x" + "€" * 6)
    rows = x_rows(hays)
    bases = np.concatenate([[0], np.cumsum([len(_b(h)) for h in hays])])
    assert {(int(bases[i]) % 16, int(bases[i] + r[0][0]) % 16) for i, r in enumerate(rows) if r} == {(p, q) for p in range(16) for q in range(16)}
    t = table(["x"])
    with Batch(hays) as b, Spans(t, 0, LL, b) as sp:
        for before, after in ((1, 1), (5, 6), (6, 5), (7, 7), (22, 21)):
            check(sp, hays, rows, before, after, EACH)


# ---- 2. seams: the neighbours' START bytes, the end of the text, padding that is not zero

def test_neighbours_are_never_counted_or_included():
    """The haystack before ends in START bytes right up to the base, the next one begins with START bytes; the middle one has fewer code points than asked for."""
    t = table(["x"])
    for mid in ("x", "éxé", "€x", "x\U0001f600", b"\x80" * 3 + b"x" + b"\xbf" * 3):
        for lead in range(0, 16, 3):
            hays = ["B" * lead + "AAAAAAAAAAAAAAAAAAAA", mid, "AAAAAAAAAAAAAAAAAAAAAAAA", "", mid, mid, "A"]
            rows = x_rows(hays)
            with Batch(hays) as b, Spans(t, 0, LL, b) as sp:
                for before, after in ((1, 1), (2, 2), (3, 3), (5, 0), (0, 5), (17, 17), (1000, 1000)):
                    check(sp, hays, rows, before, after, EACH, (mid, lead))
                    check(sp, hays, rows, before, after, MERGED, (mid, lead))


@pytest.mark.parametrize("borrowed", [False, True])
def test_the_last_haystack_ends_at_every_residue(borrowed):
    """total % 16 in 0 .. 15; in the borrowed batch the bytes from total to round_up(total, 16) are 0x41 -- START bytes that a walk beyond `total` would count."""
    t = table(["x"])
    for r in range(16):
        tail = b"x" + b"\x80" * ((r - 36) % 16)             # continuation bytes up to the end: the walk to the right finds no START byte before `total`
        hays = [b"A" * 19, b"\xc3\xa9" * 8 + tail]
        assert sum(len(h) for h in hays) % 16 == r
        rows = x_rows(hays)
        with (Borrowed(hays) if borrowed else Batch(hays)) as b, Spans(t, 0, LL, b) as sp:
            for before, after in ((0, 1), (1, 1), (2, 3), (8, 16), (9, 17)):
                check(sp, hays, rows, before, after, EACH, (r, borrowed))
            check(sp, hays, rows, 3, 3, MERGED, (r, borrowed))
    # one x as the very last byte of the text, and as the only byte
    for hays in ([b"A" * 31 + b"x"], [b"x"], [b"", b"x"], [b"A" * 16, b"\x80" * 15 + b"x"]):
        with (Borrowed(hays) if borrowed else Batch(hays)) as b, Spans(t, 0, LL, b) as sp:
            for before, after in ((0, 0), (1, 1), (40, 40)):
                check(sp, hays, x_rows(hays), before, after, EACH, (hays, borrowed))


# ---- 3. groups without a START byte

@pytest.mark.parametrize("run", [17, 32, 40])
def test_runs_of_continuation_bytes(run):
    cont = b"\x80\xbf" * 20
    hays = [b"ab" + cont[:run] + b"x" + cont[:run] + b"cd", cont[:run] + b"x" + cont[:run], b"A" * 5 + cont[:run] + b"x", b"x" + cont[:run] + b"A" * 5,
            b"a" + cont[:run] + b"b" + cont[:run] + b"x" + cont[:run] + b"c" + cont[:run] + b"d"]
    rows = x_rows(hays)
    t = table(["x"])
    with Batch(hays) as b, Spans(t, 0, LL, b) as sp:
        for before in (0, 1, 2, 3):
            for after in (0, 1, 2, 3):
                check(sp, hays, rows, before, after, EACH, run)
        check(sp, hays, rows, 2, 2, MERGED, run)


def test_haystacks_of_continuation_bytes_only_around_the_match():
    """A needle of valid UTF-8 holds a START byte, so a scan finds no span in a haystack of continuation bytes only (tests/test_extract_cpu.py gives such a haystack
    spans by hand).  Here every byte but the one-byte match is a continuation byte: no walk ever meets a START byte, every window with context on a side reaches that
    end of the haystack -- and the haystacks of continuation bytes only that lie between them are never read into a window."""
    cont = b"\x80" * 40
    hays = [cont, cont + b"x" + cont, cont, b"x" + cont, b"", cont[:33] + b"x", cont[:15], b"x", cont[:16] + b"xx" + cont[:16]]
    rows = x_rows(hays)
    t = table(["x"])
    with Batch(hays) as b, Spans(t, 0, LL, b) as sp:
        for before, after in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 5), (33, 33)):
            check(sp, hays, rows, before, after, EACH)
            check(sp, hays, rows, before, after, MERGED)
    assert xref.fragments(hays, rows, 1, 1, EACH)[1][:2] == [(0, 81), (0, 41)]


# ---- 4. EACH over both span modes, IgnoreCase, a word class

def test_each_over_all_spans_and_leftmost_longest():
    needles = ["b", "abc", "abcd"]
    hays = ["abcd b", "", "xabcdabcabcdb", "b", "éabcébé"]
    o = oracle.Machine(needles)
    t = table(needles)
    with Batch(hays) as b:
        for spans_mode in (ALL, LL):
            rows = ref.spans(o, 0, spans_mode, needles, hays)
            with Spans(t, 0, spans_mode, b) as sp:
                for before, after in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 3), (16, 16)):
                    check(sp, hays, rows, before, after, EACH, spans_mode)
    assert [s[:2] for s in ref.spans(o, 0, ALL, needles, hays[:1])[0]] == [(1, 1), (0, 3), (0, 4), (5, 1)]


def test_zero_length_spans_become_empty_haystacks():
    needles = ["", "b", "ab"]
    hays = ["abab", "", "b", "cab"]
    o = oracle.Machine(needles)
    a = am.Automaton(needles)
    t = am.api.SpanTable(a)
    for case in (0, 1):
        rows = ref.spans(o, case, ALL, needles, hays)
        assert any(s[1] == 0 for r in rows for s in r)
        with Batch(hays) as b, Spans(t, case, ALL, b) as sp:
            check(sp, hays, rows, 0, 0, EACH, case)        # zero-length fragments: empty haystacks of the new batch
            check(sp, hays, rows, 1, 1, EACH, case)
            check(sp, hays, rows, 0, 2, EACH, case)


def test_ignore_case_with_the_kelvin_sign():
    needles = ["k", "ok"]
    hays = ["é" + KELVIN + "éké", "O" + KELVIN + "!", KELVIN, "look " + KELVIN * 3 + " ok"]
    o = oracle.Machine(needles)
    t = table(needles)
    with Batch(hays) as b:
        for spans_mode in (ALL, LL):
            rows = ref.spans(o, 1, spans_mode, needles, hays)
            if spans_mode == LL:
                assert [s[:2] for s in rows[0]] == [(2, 3), (7, 1)] and [s[:2] for s in rows[1]] == [(0, 4)]
            with Spans(t, 1, spans_mode, b) as sp:
                for before, after in ((0, 0), (1, 1), (2, 1), (5, 5)):
                    check(sp, hays, rows, before, after, EACH)
                    if spans_mode == LL:
                        check(sp, hays, rows, before, after, MERGED)


def test_a_table_with_a_word_class_extracts_whole_words():
    needles = ["he", "the"]
    hays = ["the he she", "he said (he) ache he", "", "hehe he"]
    o = oracle.Machine(needles)
    t = table(needles, wref.DEFAULT_CLASS)
    with Batch(hays) as b:
        for spans_mode in (ALL, LL):
            rows = wref.spans(o, 0, spans_mode, needles, hays, wref.DEFAULT_CLASS)
            assert [s[:2] for s in rows[0]] == [(0, 3), (4, 2)]
            with Spans(t, 0, spans_mode, b) as sp:
                for before, after in ((0, 0), (1, 1), (3, 3)):
                    check(sp, hays, rows, before, after, EACH)
                    if spans_mode == LL:
                        check(sp, hays, rows, before, after, MERGED)
        assert xref.regex_snippets(needles, hays, 3, 3, whole_words=True) == [xref.fragments([h], [r], 3, 3, EACH)[2] for h, r in zip(hays, wref.spans(o, 0, LL, needles, hays, wref.DEFAULT_CLASS))]


# ---- 5. MERGED

def test_merged_by_hand():
    t = table(["ab"])
    cases = [
        (["ab.ab", "ab..ab"], 0, 1),                        # touching windows join, a gap of one byte separates
        (["ab..ab.ab...ab"], 1, 0),
        (["abababab", "ab ab ab ab"], 0, 0),                # all spans of a haystack in one piece; every span its own piece
        (["ab.ab.ab....ab.ab.....ab....ab.ab.ab"], 1, 1),   # alternating runs
        (["..ab", "ab..", "", "ab", "ab", "....", "ab"], 1000, 1000),      # ends in a match / begins with a match: both windows clamp to the shared boundary
        (["", "", "ab", "", "cd", "ab"], 2, 2),             # empty haystacks and haystacks without spans in between
        (["cd", ""], 3, 3),                                 # no spans at all: n_hay empty rows
    ]
    o = oracle.Machine(["ab"])
    for hays, before, after in cases:
        rows = ref.spans(o, 0, LL, ["ab"], hays)
        with Batch(hays) as b, Spans(t, 0, LL, b) as sp:
            check(sp, hays, rows, before, after, MERGED, hays)
            check(sp, hays, rows, before, after, EACH, hays)
    hays = ["..ab", "ab..", "", "ab", "ab", "....", "ab"]
    assert xref.fragments(hays, ref.spans(o, 0, LL, ["ab"], hays), 1000, 1000, MERGED)[:2] == ([0, 1, 2, 2, 3, 4, 4, 5], [(0, 4), (0, 4), (0, 2), (0, 2), (0, 2)])


def merged_ascii(hays, before, after):
    """The definition for ASCII haystacks and the needle x, closed form: a window is [max(p - before, 0), min(p + 1 + after, L)); numpy instead of a byte loop."""
    offs, frags, texts = [0], [], []
    for h in hays:
        p = np.flatnonzero(np.frombuffer(h, np.uint8) == 0x78).astype(np.int64)
        if len(p):
            ws, we = np.maximum(p - before, 0), np.minimum(p + 1 + after, len(h))
            head = np.ones(len(p), bool)
            head[1:] = ws[1:] > we[:-1]
            last = np.ones(len(p), bool)
            last[:-1] = head[1:]
            for a, z in zip(ws[head].tolist(), we[last].tolist()):
                frags.append((a, z - a))
                texts.append(h[a:z])
        offs.append(len(frags))
    return offs, frags, texts


SPAN_COUNTS = ["block - 1", "block", "block + 1", "2 * block + 1", 65535, 65536, 65537]


@pytest.mark.parametrize("pattern", ["heads everywhere", "a single head", "seeded"])
@pytest.mark.parametrize("n", SPAN_COUNTS)
def test_merged_span_counts(n, pattern):
    """Span counts around the exclusive sum's block (am_select_geometry) and around the single-launch limit of launch_scan_jobs, with one code point of context:
    x's four bytes apart are a piece each, x's up to three bytes apart join."""
    _, block = am.api.select_geometry()
    n = n if isinstance(n, int) else {"block - 1": block - 1, "block": block, "block + 1": block + 1, "2 * block + 1": 2 * block + 1}[n]
    rng = random.Random(n)
    sep = {"heads everywhere": lambda: "...", "a single head": lambda: "." * rng.randint(0, 2), "seeded": lambda: "." * rng.choice((0, 1, 2, 3, 3, 4))}[pattern]
    if pattern == "a single head":
        cuts = [n]                                          # one haystack: the last span looks for its head across all the others
    else:
        cuts = [n // 3, n // 3, n // 3, 2 * (n // 3), n]     # five haystacks: spans, none (empty), none (text), spans, spans
    hays, done = [], 0
    for k, c in enumerate(cuts):
        if k == 2:
            hays.append(b"......")
            continue
        hays.append(("x" + "".join(sep() + "x" for _ in range(c - done - 1))).encode() if c > done else b"")      # (ends in a match, begins with a match)
        done = c
    assert sum(h.count(b"x") for h in hays) == n
    want = merged_ascii(hays, 1, 1)
    if pattern == "heads everywhere":
        assert len(want[1]) == n
    if pattern == "a single head":
        assert len(want[1]) == 1 and want[1][0] == (0, len(hays[0]))
    t = table(["x"])
    with Batch(hays) as b, Spans(t, 0, LL, b) as sp:
        same(sp.stage(1, 1, MERGED), *want, (n, pattern))
    if n < 3000:
        assert want == xref.fragments(hays, x_rows(hays), 1, 1, MERGED)      # the closed form is the definition


def test_merged_refuses_all_spans_and_another_source():
    t = table(["ab", "b"])
    out = C.c_void_p(1)
    with Batch(["ab", "c", "abc"]) as b, Batch(["ab", "c"]) as fewer, Batch(["ab", "c", "abcd"]) as longer, Batch(["abc", "", "abc"]) as same_shape:
        every, ll = t.spans_batch(0, b, ALL, raw=True), t.spans_batch(0, b, LL, raw=True)
        try:
            assert lib().am_fragments_from_spans(b, every, 1, 1, MERGED, C.byref(out)) == am.AM_ERR_INVALID and not out.value
            assert b"AM_SPANS_LEFTMOST_LONGEST" in lib().am_last_error()
            for other in (fewer, longer):
                for mode in (EACH, MERGED):
                    out.value = 1
                    assert lib().am_fragments_from_spans(other, ll, 1, 1, mode, C.byref(out)) == am.AM_ERR_INVALID and not out.value
                    assert b"haystack count and size" in lib().am_last_error()
            out.value = 1
            assert lib().am_fragments_from_spans(b, ll, 1, 1, 2, C.byref(out)) == am.AM_ERR_INVALID and not out.value
            out.value = 1
            assert lib().am_extract_batch(t.handle, 0, ALL, 1, 1, MERGED, b, C.byref(out), None) == am.AM_ERR_INVALID and not out.value
            am.api.check(lib().am_fragments_from_spans(same_shape, ll, 0, 0, EACH, C.byref(out)))      # (the same count and total: the am_batch_from_fragments rule)
            assert lib().am_fragments_size(out) == 2
            lib().am_fragments_free(out)
            am.api.check(lib().am_fragments_from_spans(b, every, 0, 0, EACH, C.byref(out)))
            assert lib().am_fragments_size(out) == lib().am_spans_size(every) == 4
            lib().am_fragments_free(out)
        finally:
            lib().am_spans_free(every)
            lib().am_spans_free(ll)


# ---- 6. beyond 2^32

def test_positions_beyond_4_gib():
    """A borrowed batch of 2^32 + 64 KiB bytes of the letter a in two haystacks whose seam lies beyond byte 2^32; an x just before 2^32, one just after it, two at the
    seam.  The expectation is the definition over the planted regions: a hundred bytes either side of an x, cut at the haystack's ends -- the rest is filler."""
    import torch
    edge = 1 << 32
    total = edge + (64 << 10)
    seam = edge + (32 << 10) + 5
    plants = [edge - 3, edge + 9, seam - 1, seam, seam + 40]
    dev = torch.device("cuda:0")
    text = torch.full((total,), 0x61, dtype=torch.uint8, device=dev)
    for p in plants:
        text[p] = 0x78
    cuts = [0, seam, total]
    offs = torch.tensor(cuts, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def region(lo, hi):
        return bytes(0x78 if p in plants else 0x61 for p in range(lo, hi))

    def want(before, after, mode):
        w_offs, w_frags, w_texts = [0], [], []
        for h in range(2):
            base, length = cuts[h], cuts[h + 1] - cuts[h]
            wins = []
            for p in (p for p in plants if cuts[h] <= p < cuts[h + 1]):
                lo, hi = max(base, p - 100), min(base + length, p + 101)
                ws, we = xref.window(region(lo, hi), p - lo, 1, before, after)
                assert (ws > 0 or lo == base) and (we < hi - lo or hi == base + length)
                ws, we = ws + lo - base, we + lo - base
                if mode == MERGED and wins and ws <= wins[-1][1]:
                    wins[-1][1] = we
                else:
                    wins.append([ws, we])
            for ws, we in wins:
                w_frags.append((ws, we - ws))
                w_texts.append(region(base + ws, base + we))
            w_offs.append(len(w_frags))
        return w_offs, w_frags, w_texts

    t = table(["x"])
    b = C.c_void_p()
    am.api.check(lib().am_batch_from_device(text.data_ptr(), offs.data_ptr(), 2, total, C.byref(b)))
    try:
        with Spans(t, 0, LL, b) as sp:
            assert lib().am_spans_size(sp.h) == len(plants)
            for before, after, mode in ((33, 33, EACH), (33, 33, MERGED), (5, 6, MERGED), (0, 0, EACH), (16, 17, EACH), (20, 20, MERGED)):
                same(sp.stage(before, after, mode), *want(before, after, mode), (before, after, mode))
        assert want(33, 33, EACH)[1][0] == (edge - 3 - 33, 67) and want(33, 33, MERGED)[1][:2] == [(edge - 36, 79), (seam - 1 - 33, 34)]
    finally:
        lib().am_batch_destroy(b)
    del text


# ---- 7. the routes: am_extract_batch and am_extract

def pool_case(seed, n_hay=120, max_frags=12):
    """Needles and haystacks from a shared fragment pool, some haystacks empty."""
    from tests import helpers
    rng = random.Random(seed)
    alphabet = helpers.ALPHABETS[seed % len(helpers.ALPHABETS)]
    frags = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 5))) for _ in range(rng.randint(3, 8))]
    needles = ["".join(rng.choice(frags) for _ in range(rng.randint(1, 3))) for _ in range(rng.randint(1, 12))]
    hays = ["".join(rng.choice(frags) for _ in range(rng.randint(0, max_frags))) for _ in range(n_hay)]
    for k in range(0, n_hay, 37):
        hays[k] = ""
    return needles, hays


def extract_batch(t, case, spans_mode, before, after, mode, b, with_frags=True):
    """am_extract_batch: (offsets, fragments, new offsets, new text); offsets and fragments None without frags_out."""
    nb, fr = C.c_void_p(), C.c_void_p()
    am.api.check(lib().am_extract_batch(t.handle, case, spans_mode, before, after, mode, b, C.byref(nb), C.byref(fr) if with_frags else None))
    try:
        offs, frags = am.api.fragments_to_numpy(fr) if with_frags else (None, None)
        new_offs, new_text = read_batch(nb)
    finally:
        lib().am_batch_destroy(nb)
        if with_frags:
            lib().am_fragments_free(fr)
    return offs, frags, new_offs, new_text


def extract_oneshot(t, case, spans_mode, before, after, mode, hays, with_frags=True):
    s = am.api._Slices(hays)
    nb, fr = C.c_void_p(), C.c_void_p()
    am.api.check(lib().am_extract(t.handle, case, spans_mode, before, after, mode, s.arr, s.n, C.byref(nb), C.byref(fr) if with_frags else None))
    try:
        offs, frags = am.api.fragments_to_numpy(fr) if with_frags else (None, None)
        new_offs, new_text = read_batch(nb)
    finally:
        lib().am_batch_destroy(nb)
        if with_frags:
            lib().am_fragments_free(fr)
    return offs, frags, new_offs, new_text


@pytest.mark.parametrize("seed", range(2))
def test_extract_on_every_route(route, seed):
    needles, hays = pool_case(50 + seed)
    for case in (0, 1):
        ns = [oracle.lower_utf8(x).decode() for x in needles] if case else needles
        o = oracle.Machine(ns)
        t = table(ns, route=route)
        with Batch(hays) as b:
            for spans_mode, mode, before, after in ((LL, EACH, 3, 4), (LL, MERGED, 3, 4), (ALL, EACH, 1, 0), (LL, MERGED, 0, 0)):
                want = xref.extract(o, case, spans_mode, ns, hays, before, after, mode)
                got = extract_batch(t, case, spans_mode, before, after, mode, b)
                same(got, *want, (case, spans_mode, mode))
                again = extract_batch(t, case, spans_mode, before, after, mode, b, with_frags=False)      # frags_out NULL; two runs give identical bytes
                assert again[0] is None and np.array_equal(again[2], got[2]) and again[3] == got[3]
                if mode == MERGED or spans_mode == ALL:
                    same(extract_oneshot(t, case, spans_mode, before, after, mode, hays), *want, ("one-shot", case, spans_mode, mode))
            one = extract_oneshot(t, case, LL, 3, 4, EACH, hays, with_frags=False)
            assert one[3] == b"".join(xref.extract(o, case, LL, ns, hays, 3, 4, EACH)[2])


def test_no_haystacks_and_no_matches():
    t = table(["ab"])
    for mode in (EACH, MERGED):
        same(extract_oneshot(t, 0, LL, 2, 2, mode, []), [0], [], [], "n_hay == 0")
        got = extract_oneshot(t, 0, LL, 2, 2, mode, [], with_frags=False)
        assert got[2].tolist() == [0] and got[3] == b""
        hays = ["cd", "", "ef"]
        same(extract_oneshot(t, 1, LL, 2, 2, mode, hays), [0, 0, 0, 0], [], [], "an automaton that matches nothing")
        with Batch(hays) as b:
            same(extract_batch(t, 0, LL, 2, 2, mode, b), [0, 0, 0, 0], [], [], "nothing, batch form")
    with Batch([]) as b:
        same(extract_batch(t, 0, ALL, 1, 1, EACH, b), [0], [], [], "the empty batch")
        sp = t.spans_batch(0, b, LL, raw=True)
        try:
            offs, frags = t.fragments_from_spans(b, sp, 1, 1, True)
            assert offs.tolist() == [0] and len(frags) == 0
        finally:
            lib().am_spans_free(sp)
    none = table([])                                        # no needles: n_hay empty rows
    same(extract_oneshot(none, 0, LL, 1, 1, MERGED, ["ab", "c"]), [0, 0, 0], [], [], "no needles")


PARAGRAPH = ("The naïve café in Αθήνα sold 東京 postcards; Москва and Αθήνα were sold out. \U0001f600 "
             "A second café, the Café Москва, kept 東京タワー prints — and one of Αθήνα.\n")


def test_the_front_end_equals_the_regex_opinion_on_mixed_scripts():
    needles = ["café", "Αθήνα", "東京", "東京タワー", "Москва", "sold", "\U0001f600", "a"]
    texts = [PARAGRAPH, PARAGRAPH[40:120], "", "東京" * 5, PARAGRAPH * 3]
    a = am.Automaton(needles)
    for before, after in ((0, 0), (1, 1), (5, 7), (40, 40)):
        assert a.extract(0, texts, before, after) == xref.regex_snippets(needles, texts, before, after), (before, after)
    assert a.extract(0, texts, 4, 4, whole_words=True) == xref.regex_snippets(needles, texts, 4, 4, whole_words=True)
    o = oracle.Machine(needles)
    merged = a.extract(0, texts, 5, 5, merged=True)
    assert merged == [xref.fragments([h], [r], 5, 5, MERGED)[2] for h, r in zip(texts, ref.spans(o, 0, LL, needles, texts))]
    every = a.extract(1, texts, 2, 2, leftmost_longest=False)
    assert every == [xref.fragments([h], [r], 2, 2, EACH)[2] for h, r in zip(texts, ref.spans(o, 1, ALL, needles, texts))]


def test_the_launches_have_names():
    t = table(["ab"])
    am.api.check(lib().am_profile_reset())
    am.api.check(lib().am_profile_enable(1))
    try:
        with Batch(["ab.ab", "ab"]) as b:
            nb, _, _ = t.extract_batch(0, b, 1, 1, merged=True)
            lib().am_batch_destroy(nb)
    finally:
        am.api.check(lib().am_profile_enable(0))
    for k in (b"extract_windows", b"extract_heads", b"extract_emit", b"split_gather"):
        ms, n = C.c_double(0), C.c_uint64(0)
        am.api.check(lib().am_profile_read(k, C.byref(ms), C.byref(n)))
        assert n.value == 1, k
