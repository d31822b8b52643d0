"""Match coordinates on the device (am_coords_* / am_ranges_*, csrc/am_coords.hip) against the definition.  Every check compares start, len, haystack, needle, the
offsets and all four fields of every range with tests/coords_reference.py -- the byte definition, which tests/test_coords_cpu.py holds to byte loops and to Python's
str operations -- over spans that come from the oracle or from a literal rule (every byte x is a span), never from another path of the library.  Shapes sit on the
real seams: every residue of a haystack's base and of a match's start modulo the 16-byte group and the 128-byte tile, a match that ends on a tile edge and at the end
of the text, haystack seams, lines of 1 to 70 000 tiles, padding that is not zero, the exclusive sum's block and its second level, byte 2^32."""
import ctypes as C
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import coords_reference as cref, spans_reference as ref
from tests.test_gpu_extract import ROUTES, Batch, Borrowed, _b, lib, table

pytestmark = pytest.mark.gpu

UNITS = cref.UNITS
ALL, LL = ref.ALL, ref.LEFTMOST_LONGEST
KELVIN = "\u212a"
FACE = "\U0001f600"
TILE = 128


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)
    yield ROUTES[request.param]
    am.debug_set("AM_DFA", -1)


def x_rows(hays):
    """The spans of the one needle x, by the definition: every byte x, one byte long."""
    return [[(int(i), 1, 0) for i in np.flatnonzero(np.frombuffer(_b(h), np.uint8) == 0x78)] for h in hays]


def expected(hays, rows, unit, tables=None):
    """offsets and the eight columns (start, len, start_line, start_col, end_line, end_col, haystack, needle) the definition gives for byte rows (start, len, needle);
    tables: the running counts of the haystacks, kept from unit to unit"""
    tables = {} if tables is None else tables
    offs, cols = [0], [[] for _ in range(8)]
    for h, (hay, r) in enumerate(zip(hays, rows)):
        if r:
            if h not in tables:
                tables[h] = cref.Table(_b(hay))
            got = tables[h].spans([x[0] for x in r], [x[1] for x in r], unit)
            for k in range(6):
                cols[k].append(np.asarray(got[k], np.int64))
            cols[6].append(np.full(len(r), h, np.int64))
            cols[7].append(np.array([x[2] for x in r], np.int64))
        offs.append(offs[-1] + len(r))
    return offs, [np.concatenate(c) if c else np.zeros(0, np.int64) for c in cols]


NAMES = ("start", "len", "start_line", "start_col", "end_line", "end_col", "haystack", "needle")


def compare(got, want, what):
    (offs, spans), (roffs, ranges) = got
    w_offs, w = want
    assert np.asarray(offs, np.int64).tolist() == list(w_offs) == np.asarray(roffs, np.int64).tolist(), (what, "offsets")
    assert len(spans) == len(ranges) == len(w[0]), (what, len(spans), len(ranges), len(w[0]))
    have = [spans["start"], spans["len"], ranges["start_line"], ranges["start_col"], ranges["end_line"], ranges["end_col"], spans["haystack"], spans["needle"]]
    for name, g, e in zip(NAMES, have, w):
        g = np.asarray(g).astype(np.int64)
        if not np.array_equal(g, e):
            k = int(np.flatnonzero(g != e)[0])
            raise AssertionError((what, name, "row", k, "got", g[k:k + 4].tolist(), "want", e[k:k + 4].tolist()))


def convert(b, raw, unit, lines=True):
    c = am.Coords(b, lines=lines, utf16=unit == am.UTF16)
    return c.spans(raw, unit), c.ranges(raw, unit)


def check(hays, rows, t=None, case=0, mode=LL, batch=Batch, what=None, units=UNITS, **kw):
    """spans of `hays` under table t (default: the needle x), converted in every unit, against the definition over `rows`; returns the converted bytes"""
    t = t or table(["x"])
    out, tables = [], {}
    with batch(hays, **kw) as b:
        raw = t.spans_batch(case, b, mode, raw=True)
        try:
            assert lib().am_spans_size(raw) == sum(len(r) for r in rows), (what, "the scan's span count", lib().am_spans_size(raw), sum(len(r) for r in rows))
            for unit in units:
                got = convert(b, raw, unit)
                compare(got, expected(hays, rows, unit, tables), (what, "unit", unit))
                out.append(b"".join(np.asarray(a).tobytes() for pair in got for a in pair))
        finally:
            lib().am_spans_free(raw)
    return out


# ---- 1. residues: the base and the match's start at every residue of the group and of the tile; ends on a tile edge and at the end of the text

POOL = ["a", "b", "é", "€", FACE, "\n", "x", "x", " "]


def body(seed, n):
    rng = random.Random(seed)
    return "".join(rng.choice(POOL) for _ in range(n))


def test_every_residue_of_the_base_and_of_the_start():
    starts16, starts128 = set(), set()
    for filler in range(17):
        hays = ["A" * filler, body(filler, 420), "A", body(100 + filler, 60)]
        rows = x_rows(hays)
        bases = np.concatenate([[0], np.cumsum([len(_b(h)) for h in hays])])
        assert int(bases[1]) == filler
        for i, r in enumerate(rows):
            starts16 |= {(int(bases[i]) + s[0]) % 16 for s in r}
            starts128 |= {(int(bases[i]) + s[0]) % TILE for s in r}
        check(hays, rows, what=("filler", filler))
    assert starts16 == set(range(16)) and starts128 == set(range(TILE)), "the match starts cover every residue"


@pytest.mark.parametrize("borrowed", [False, True])
def test_a_match_that_ends_on_a_tile_edge_and_at_the_end_of_the_text(borrowed):
    """total % 128 == 0 and the last byte is a match: the lookup at base + p == total takes prefix[n_tiles] and must load no text (in the borrowed batch nothing
    readable lies behind `total`)."""
    for filler in (0, 1, 16, 17):
        for tiles in (1, 2, 3):
            n = tiles * TILE - filler
            text = ("é\n" + FACE + "x") * 40
            hay = _b(text)[:n - 1]
            while len(hay) < n - 1:
                hay += b"a"
            hay = hay[:TILE - filler - 1] + b"x" + hay[TILE - filler:] if tiles > 1 else hay      # an x whose end is the first tile's edge
            hay += b"x"
            hays = [b"A" * filler, hay]
            assert sum(len(h) for h in hays) % TILE == 0
            rows = x_rows(hays)
            assert rows[1][-1][0] + 1 == len(hay) and (tiles == 1 or any((filler + r[0] + 1) % TILE == 0 for r in rows[1][:-1]))
            check(hays, rows, batch=Borrowed if borrowed else Batch, what=(filler, tiles, borrowed))


# ---- 2. seams

def test_haystack_seams():
    long_last_line = "p\n" + "é" * 300 + "x"
    hays = ["", "", "x\n", "no newline x here", "", long_last_line, "x and no newline", "x", "", "\n", "x", "\nx\n\n", "xx", ""]
    check(hays, x_rows(hays), what="seams")
    # line 0 and the column are measured from the haystack's own base: after a haystack that ends in a newline, and after one whose last line is long
    with Batch(hays) as b:
        raw = table(["x"]).spans_batch(0, b, LL, raw=True)
        try:
            offs, ranges = am.Coords(b, lines=True).ranges(raw, am.CODE_POINTS)
        finally:
            lib().am_spans_free(raw)
    row = lambda h: tuple(int(v) for v in ranges[int(offs[h])])
    assert row(3) == (0, 11, 0, 12) and row(6) == (0, 0, 0, 1) and row(5) == (1, 300, 1, 301) and row(11) == (1, 0, 1, 1)


@pytest.mark.parametrize("split", [1, 2, 3])
def test_a_four_byte_code_point_across_a_tile_seam(split):
    for filler in (0, 5):
        hays = ["A" * filler, "a" * (TILE - filler - split) + FACE + "x" + FACE + "\nx", "x" + FACE]
        rows = x_rows(hays)
        assert (filler + rows[1][0][0]) == TILE + 4 - split
        check(hays, rows, what=(split, filler))


def test_a_newline_as_the_last_byte_of_a_tile_and_as_the_first_of_the_next():
    for at in (TILE - 1, TILE, 2 * TILE - 1, 2 * TILE):
        for filler in (0, 3):
            hays = ["A" * filler, "é" * 20 + "a" * (at - filler - 40) + "\n" + "x" + "é" * 70 + "x\nx"]
            assert _b(hays[1])[at - filler] == 0x0A
            check(hays, x_rows(hays), what=(at, filler))


# ---- 3. the binary search: long lines

@pytest.mark.parametrize("tiles", [1, 2, 300, 70000])
def test_a_long_line_before_the_match(tiles):
    run = np.frombuffer(b"\xc3\xa9" * (tiles * TILE // 2), np.uint8)
    head, tail = np.frombuffer(b"ab\nq", np.uint8), np.frombuffer(b"x" + "€x\nyx".encode() + b"\xc3\xa9" * 70 + b"x", np.uint8)
    inside = np.concatenate([head, run, tail])              # the line start lies `tiles` tiles before the match, inside the haystack
    cut = len(head) + (len(run) // 2 | 1)                   # ... and here the haystack begins in the middle of that run, in the middle of an é
    hays = [b"A" * 7, inside, inside[:cut].copy(), inside[cut:].copy(), np.concatenate([np.frombuffer(b"\n\n", np.uint8), run, tail])]
    rows = x_rows(hays)
    assert len(rows[1]) == 4 and len(rows[3]) == 4 and rows[2] == []
    check(hays, rows, what=tiles)


# ---- 4. padding that is not zero

def test_the_padding_of_a_borrowed_batch_never_counts():
    results = []
    for pad in (0x0A, 0xF0, 0x41):
        per_pad = []
        for r in range(16):
            hays = [b"A" * 19, ("é\n" + FACE).encode() * 6 + b"x" + b"\x80" * ((r - 19 - 44) % 16) + b"x"]      # the last byte of the text is a match
            assert sum(len(h) for h in hays) % 16 == r
            per_pad.append(check(hays, x_rows(hays), batch=Borrowed, pad=pad, what=(pad, r)))
        results.append(per_pad)
    assert results[0] == results[1] == results[2]
    for hays in ([b"x"], [b"", b"\nx"], [b"A" * 16, b"\xf0" * 15 + b"x"]):
        for pad in (0x0A, 0xF0, 0x41):
            check(hays, x_rows(hays), batch=Borrowed, pad=pad, what=(hays, pad))


# ---- 5. the scan's limits

TILE_COUNTS = ["block - 1", "block", "block + 1", "2 * block + 3", 65535, 65536, 65537]


@pytest.mark.parametrize("n_tiles", TILE_COUNTS)
def test_tile_counts_around_the_scan_s_blocks(n_tiles):
    """The prefix arrays have n_tiles + 1 entries: around one workgroup of the exclusive sum (am_select_geometry), two of them, and 65 536.  Every 997 bytes an é, a
    newline and an x: a multi-byte character and a newline in every scan block, the spans in every tile region."""
    _, block = am.api.select_geometry()
    n_tiles = n_tiles if isinstance(n_tiles, int) else {"block - 1": block - 1, "block": block, "block + 1": block + 1, "2 * block + 3": 2 * block + 3}[n_tiles]
    total = n_tiles * TILE - 5
    text = np.full(total, 0x61, np.uint8)
    for k, byte in enumerate(b"\xc3\xa9\n" + FACE.encode() + b"x"):
        text[100 + k:total - 16:997] = byte
    text[total - 1] = 0x78
    cuts = [0, 3, total // 3 + 1, total // 3 + 1, total]
    hays = [text[cuts[i]:cuts[i + 1]].copy() for i in range(4)]
    rows = x_rows(hays)
    assert sum(len(r) for r in rows) >= total // 997
    check(hays, rows, what=n_tiles)


# ---- 6. byte 2^32

PERIOD = b"ab\xc3\xa9\n" + FACE.encode() + b"cdefghi"            # 16 bytes: 12 START bytes, one byte >= 0xF0, one newline (at 4)
assert len(PERIOD) == 16


def periodic(g, cls):
    """the class count of the bytes [0, g) of PERIOD repeated: closed form"""
    per = [sum(1 for b in PERIOD[:r] if ((b & 0xC0) != 0x80 if cls == 0 else b >= 0xF0 if cls == 1 else b == 0x0A)) for r in range(17)]
    return (g // 16) * per[16] + per[g % 16]


def periodic_units(g, unit):
    return g if unit == am.BYTES else periodic(g, 0) if unit == am.CODE_POINTS else periodic(g, 0) + periodic(g, 1)


def periodic_linestart(base, g):
    at = (g - 5) // 16 * 16 + 5 if g >= 5 else 0            # one past the last newline (offset 4 of a period) below g
    return max(at, base) if g >= 5 else base


def test_positions_and_a_match_beyond_byte_2_32():
    import torch
    edge = 1 << 32
    total = edge + (64 << 10)
    dev = torch.device("cuda:0")
    text = torch.frombuffer(bytearray(PERIOD), dtype=torch.uint8).to(dev).repeat(total // 16)
    plant = edge + 4096 + 11                                # a letter of a period beyond 2^32 becomes the needle
    assert 0x61 <= PERIOD[plant % 16] <= 0x69
    text[plant] = 0x78
    cuts = [0, total - 1000, total - 990, total - 990, total]      # one haystack across byte 2^32, then three short ones (one of them empty)
    offs = torch.tensor(cuts, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    b = C.c_void_p()
    am.api.check(lib().am_batch_from_device(text.data_ptr(), offs.data_ptr(), 4, total, C.byref(b)))
    try:
        c = am.Coords(b, lines=True, utf16=True)
        assert c.index_bytes == 3 * 8 * (total // TILE + 1)
        hay = [0] * 10 + [1, 1, 2, 3, 3, 3]
        pos = [0, 1, edge - 129, edge - 1, edge, edge + 1, edge + 127, edge + 128, edge + 4107, cuts[1], 0, 10, 0, 0, 7, 990]
        d_hay = torch.tensor(hay, dtype=torch.int32, device=dev)
        d_pos = torch.tensor(pos, dtype=torch.int64, device=dev)
        d_out = torch.zeros(len(pos), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for unit in UNITS:
            am.api.check(lib().am_coords_positions_device(c.handle, d_hay.data_ptr(), d_pos.data_ptr(), len(pos), unit, d_out.data_ptr()))
            want = [periodic_units(cuts[h] + p, unit) - periodic_units(cuts[h], unit) for h, p in zip(hay, pos)]
            assert d_out.cpu().tolist() == want, unit
        assert (periodic_units(edge, am.CODE_POINTS), periodic_units(edge, am.UTF16)) == (12 << 28, 13 << 28)
        raw = table(["x"]).spans_batch(0, b, LL, raw=True)
        try:
            assert lib().am_spans_size(raw) == 1
            for unit in UNITS:
                (so, sp), (ro, rg) = c.spans(raw, unit), c.ranges(raw, unit)
                assert so.tolist() == ro.tolist() == [0, 1, 1, 1, 1]
                u = lambda g: periodic_units(g, unit)
                assert (int(sp[0]["start"]), int(sp[0]["len"]), int(sp[0]["haystack"]), int(sp[0]["needle"])) == (u(plant), 1, 0, 0), unit
                ls = periodic_linestart(0, plant)
                assert tuple(int(v) for v in rg[0]) == (periodic(plant, 2), u(plant) - u(ls), periodic(plant + 1, 2), u(plant + 1) - u(ls)), unit
        finally:
            lib().am_spans_free(raw)
        del c
    finally:
        lib().am_batch_destroy(b)
    del text


# ---- 7. the scan routes, both case modes, both span modes

@pytest.mark.parametrize("seed", range(2))
def test_converted_spans_on_every_route(route, seed):
    from tests.test_gpu_extract import pool_case
    needles, hays = pool_case(70 + seed, n_hay=60)
    hays = [h + ("\n" if k % 3 == 0 else "") + h for k, h in enumerate(hays)]
    for case in (0, 1):
        ns = [oracle.lower_utf8(x).decode() for x in needles] if case else needles
        o = oracle.Machine(ns)
        t = table(ns, route=route)
        for mode in (ALL, LL):
            check(hays, ref.spans(o, case, mode, ns, hays), t=t, case=case, mode=mode, what=(case, mode))


def test_ignore_case_spans_have_the_needle_s_code_points_and_the_text_s_bytes():
    a = am.Automaton(["nike"])
    texts = ["é NIKE", "é ni" + KELVIN + "e\n" + FACE + " NI" + KELVIN + "E nike"]
    offs, spans = a.spans(am.IGNORE_CASE, texts, unit=am.CODE_POINTS)
    assert offs.tolist() == [0, 1, 4]
    assert [(int(s["start"]), int(s["len"])) for s in spans] == [(2, 4), (2, 4), (9, 4), (14, 4)]
    _, in_bytes = a.spans(am.IGNORE_CASE, texts)
    assert [int(s["len"]) for s in in_bytes] == [4, 6, 6, 4]
    _, in_utf16 = a.spans(am.IGNORE_CASE, texts, unit=am.UTF16)
    assert [(int(s["start"]), int(s["len"])) for s in in_utf16] == [(2, 4), (2, 4), (10, 4), (15, 4)]
    for (s, t) in zip(spans, [texts[0]] + [texts[1]] * 3):
        assert oracle.lower_utf8(t[int(s["start"]):int(s["start"]) + int(s["len"])]).decode() == "nike"      # a str slice: what the unit is for
    o = oracle.Machine(["nike"])
    check(texts, ref.spans(o, 1, ALL, ["nike"], texts), t=table(["nike"]), case=1, mode=ALL, what="kelvin")


# ---- 8. fragments and positions

@pytest.mark.parametrize("sep", ["\n", ","])
def test_fragments_of_a_split(sep):
    texts = ["é,x\n" + FACE + ",,\n€a", "", sep, "no separator " + FACE, (FACE + sep) * 40 + "é", "a" * 200 + sep + "é" * 100]
    sp = am.Splitter(sep)
    want_offs, want = [0], {u: [] for u in UNITS}
    for t in texts:
        at = 0
        for piece in t.split(sep):                          # Python's opinion of the fragments, in code points; the definition turns them into units
            s, n = len(t[:at].encode()), len(piece.encode())
            for u in UNITS:
                want[u].append(cref.span(t.encode(), s, n, u))
            at += len(piece) + len(sep)
        want_offs.append(len(want[am.BYTES]))
    with Batch(texts) as b:
        f = sp.split_fragments(b)
        try:
            c = am.Coords(b, utf16=True)
            for u in UNITS:
                offs, frags = c.fragments(f, u)
                assert offs.tolist() == want_offs and list(zip(frags["start"].tolist(), frags["len"].tolist())) == want[u], (sep, u)
        finally:
            lib().am_fragments_free(f)


def test_positions_of_every_byte_and_the_front_end():
    hays = ["", "é\n" + FACE + "x", "A" * 130 + "\n" + FACE * 40, "", "x"]
    with Batch(hays) as b:
        c = am.Coords(b, utf16=True)
        hay = [h for h, t in enumerate(hays) for _ in range(len(_b(t)) + 1)]
        pos = [p for t in hays for p in range(len(_b(t)) + 1)]
        for unit in UNITS:
            assert c.positions(hay, pos, unit).tolist() == [cref.units(_b(hays[h]), p, unit) for h, p in zip(hay, pos)], unit
        assert c.positions([], [], am.UTF16).tolist() == []
    a = am.Automaton(["x", "é"])
    for case in (0, 1):
        h0, p0, v0 = a.run_batch_with_case(case, hays)
        assert [np.array_equal(x, y) for x, y in zip(a.run_batch_with_case(case, hays, unit=am.BYTES), (h0, p0, v0))] == [True] * 3
        for unit in (am.CODE_POINTS, am.UTF16):
            h1, p1, v1 = a.run_batch_with_case(case, hays, unit=unit)
            assert np.array_equal(h0, h1) and np.array_equal(v0, v1)
            assert p1.tolist() == [cref.units(_b(hays[h]), int(p), unit) for h, p in zip(h0, p0)]


def test_locate_gives_line_and_column():
    text = "first line\nthe " + FACE + " Nike shoe\n\nnike"
    a = am.Automaton(["nike", "shoe"])
    offs, spans, ranges = a.locate(am.IGNORE_CASE, [text, "", "shoe"])
    assert offs.tolist() == [0, 3, 3, 4] and ranges.dtype == am.api.SPAN_RANGE_DTYPE
    assert [tuple(int(v) for v in r) for r in ranges] == [(1, 6, 1, 10), (1, 11, 1, 15), (3, 0, 3, 4), (0, 0, 0, 4)]
    assert [text[int(s["start"]):int(s["start"]) + int(s["len"])].lower() for s in spans[:3]] == ["nike", "shoe", "nike"]
    _, _, lsp = a.locate(am.IGNORE_CASE, [text], unit=am.UTF16)      # a Language-Server range: the face is a surrogate pair
    assert [tuple(int(v) for v in r) for r in lsp] == [(1, 7, 1, 11), (1, 12, 1, 16), (3, 0, 3, 4)]
    lines = text.split("\n")
    for r in ranges[:3]:
        assert lines[int(r["start_line"])][int(r["start_col"]):int(r["end_col"])].lower() in ("nike", "shoe")


# ---- 9. refusals, defaults, determinism, empties, names

def test_refusals_on_the_device():
    t = table(["ab", "b"])
    out = C.c_void_p(1)

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and word in lib().am_last_error(), (rc, lib().am_last_error())

    with Batch(["ab", "c", "éabc"]) as b, Batch(["ab", "c"]) as fewer, Batch(["ab", "c", "éabcd"]) as longer:
        c, plain, other = am.Coords(b, lines=True, utf16=True), am.Coords(b), am.Coords(fewer, lines=True)
        ll = t.spans_batch(0, b, LL, raw=True)
        conv = c.spans(ll, am.CODE_POINTS, raw=True)
        copy = c.spans(ll, am.BYTES, raw=True)
        sp = am.Splitter("b")
        f = sp.split_fragments(b)
        fconv = c.fragments(f, am.UTF16, raw=True)
        try:
            # a position one beyond its haystack; hay == n_hay
            for hay, pos in (([0, 2], [2, 6]), ([0, 3], [0, 0]), ([1], [2])):
                with pytest.raises(am.AmError) as e:
                    c.positions(hay, pos, am.CODE_POINTS)
                assert e.value.code == am.AM_ERR_INVALID and "beyond its haystack" in str(e.value)
            assert c.positions([0, 2, 1], [2, 5, 1], am.CODE_POINTS).tolist() == [2, 4, 1]      # ... and exactly at the end is a position
            # a converted result handed to the stages that read byte spans, and to the index itself
            r = am.api.SubstTable(t, ["X", "Y"])
            nb = C.c_void_p(1)
            refused(lib().am_batch_substitute(b, conv, r.handle, C.byref(nb)), b"converted units")
            assert not nb.value
            refused(lib().am_fragments_from_spans(b, conv, 1, 1, 0, C.byref(out)), b"converted units")
            near = am.api.Near(t, [1, 2], [(0, 1, 5)])
            refused(lib().am_near_spans(near.handle, conv, C.byref(out)), b"converted units")
            refused(lib().am_coords_spans(c.handle, conv, am.UTF16, C.byref(out)), b"converted units")
            refused(lib().am_coords_ranges(c.handle, conv, am.BYTES, C.byref(out)), b"converted units")
            refused(lib().am_batch_from_fragments(b, fconv, C.byref(nb)), b"converted units")
            refused(lib().am_coords_fragments(c.handle, fconv, am.BYTES, C.byref(out)), b"converted units")
            assert not out.value
            # AM_UNIT_BYTES gives a plain copy that is not marked: every stage takes it
            am.api.check(lib().am_batch_substitute(b, copy, r.handle, C.byref(nb)))
            assert am.api.batch_to_bytes(nb)[1] == [b"X", b"c", "éXc".encode()]
            lib().am_batch_destroy(nb)
            assert np.array_equal(am.api.spans_to_numpy(copy)[1], am.api.spans_to_numpy(ll)[1])
            # an index that lacks what the call needs names the flag
            refused(lib().am_coords_ranges(plain.handle, ll, am.CODE_POINTS, C.byref(out)), b"AM_COORDS_LINES")
            refused(lib().am_coords_spans(plain.handle, ll, am.UTF16, C.byref(out)), b"AM_COORDS_UTF16")
            refused(lib().am_coords_ranges(other.handle, ll, am.UTF16, C.byref(out)), b"haystack count and size")
            # spans from another batch
            for idx in (am.Coords(fewer), am.Coords(longer)):
                refused(lib().am_coords_spans(idx.handle, ll, am.CODE_POINTS, C.byref(out)), b"haystack count and size")
                refused(lib().am_coords_fragments(idx.handle, f, am.CODE_POINTS, C.byref(out)), b"haystack count and size")
            assert not out.value
        finally:
            for s in (ll, conv, copy):
                lib().am_spans_free(s)
            for x in (f, fconv):
                lib().am_fragments_free(x)


def test_the_default_is_unchanged_and_two_calls_agree():
    needles = ["nike", "é", "x", "shoe"]
    texts = ["é nike x\nshoe " + FACE + "x", "", "xxé", "NIKE " + KELVIN]
    a = am.Automaton(needles)
    o = oracle.Machine(needles)
    for case in (0, 1):
        for ll in (False, True):
            rows = ref.spans(o, case, LL if ll else ALL, needles, texts)
            flat = [(s, n, h, v) for h, r in enumerate(rows) for s, n, v in r]
            o0, s0 = a.spans(case, texts, leftmost_longest=ll)
            o1, s1 = a.spans(case, texts, leftmost_longest=ll, unit=am.BYTES)
            assert o0.tobytes() == o1.tobytes() and s0.tobytes() == s1.tobytes()
            assert [tuple(int(x) for x in s) for s in s0] == flat
            for unit in (am.CODE_POINTS, am.UTF16):
                first, again = a.spans(case, texts, leftmost_longest=ll, unit=unit), a.spans(case, texts, leftmost_longest=ll, unit=unit)
                assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
                assert [(int(s["start"]), int(s["len"])) for s in first[1]] == [cref.span(_b(texts[h]), s, n, unit) for s, n, h, _ in flat]
    hays = [body(5, 3000), body(6, 10)]
    assert check(hays, x_rows(hays)) == check(hays, x_rows(hays))      # byte-identical from call to call: spans, ranges and their offsets


def test_no_haystacks_no_rows_and_an_index_that_carries_nothing():
    t = table(["x"])
    with Batch([]) as b:
        c = am.Coords(b, lines=True, utf16=True)
        raw = t.spans_batch(0, b, LL, raw=True)
        try:
            for unit in UNITS:
                (so, sp), (ro, rg) = c.spans(raw, unit), c.ranges(raw, unit)
                assert so.tolist() == ro.tolist() == [0] and len(sp) == len(rg) == 0
        finally:
            lib().am_spans_free(raw)
        assert c.positions([], [], am.CODE_POINTS).tolist() == []
    hays = ["abc", "", "é"]
    check(hays, [[], [], []], what="no rows")
    with Batch(hays) as b:
        h = C.c_void_p()
        am.api.check(lib().am_coords_create(b, 0, C.byref(h)))      # what == 0: serves AM_UNIT_BYTES only, keeps nothing
        try:
            assert lib().am_coords_index_bytes(h) == 0
            out = np.zeros(2, np.uint64)
            hay, pos = np.array([0, 2], np.uint32), np.array([3, 2], np.uint64)
            am.api.check(lib().am_coords_positions(h, hay.ctypes.data, pos.ctypes.data, 2, am.BYTES, out.ctypes.data))
            assert out.tolist() == [3, 2]
            assert lib().am_coords_positions(h, hay.ctypes.data, pos.ctypes.data, 2, am.CODE_POINTS, out.ctypes.data) == am.AM_ERR_INVALID
            assert b"AM_COORDS_CODE_POINTS" in lib().am_last_error()
        finally:
            lib().am_coords_destroy(h)
        assert am.Coords(b).index_bytes == 8 * 2 and am.Coords(b, lines=True, utf16=True).index_bytes == 3 * 8 * 2


def test_the_launches_have_names():
    t = table(["x"])
    am.api.check(lib().am_profile_reset())
    am.api.check(lib().am_profile_enable(1))
    try:
        with Batch(["x\nx", "éx"]) as b:
            raw = t.spans_batch(0, b, LL, raw=True)
            try:
                c = am.Coords(b, lines=True, utf16=True)
                c.spans(raw, am.UTF16)
                c.ranges(raw, am.UTF16)
                c.positions([0], [1], am.UTF16)
            finally:
                lib().am_spans_free(raw)
    finally:
        am.api.check(lib().am_profile_enable(0))
    for k, launches in ((b"coords_tiles", 1), (b"coords_scan", 3), (b"coords_spans", 1), (b"coords_ranges", 1), (b"coords_positions", 1)):
        ms, n = C.c_double(0), C.c_uint64(0)
        am.api.check(lib().am_profile_read(k, C.byref(ms), C.byref(n)))
        assert n.value == launches, k
